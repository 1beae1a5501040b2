// Schedule of the LDS sweep: the one definition that lds_sweep_kernel
// (probe_kernels.h) runs, that lds_sweep and lds_sweep_reference
// (health_probe.hip) state their results in and that
// tests/native/lds_march_check.cpp runs against a faulty-LDS model.
// Plain C++17, no HIP: constexpr functions, usable from device and host
// code alike.
//
// One block of 256 threads (4 waves, one per SIMD) owns lds_bytes of LDS,
// a multiple of 16: elems = lds_bytes / 16 elements of 16 bytes.  Data
// comes from hbm_march.h: element e of block b holds
// hbmmarch::pattern(p, seed, b * elems + e), so every block holds other
// data.  (The dma path's image is indexed by e alone: one image for all.)
//
//   path  what runs                                  bytes covered
//   b128  the 4 march steps of hbm_march.h, 16-byte  all
//         loads and stores
//   b64   the same march, 8-byte accesses            all
//   b32   the same march, 4-byte accesses            all
//   dma   0 poison (16-byte stores)                  whole KiB of lds_bytes
//         1 fill from a global image, LDS-DMA
//         2 read-verify (16-byte loads)
//   tr16  0 write (16-byte stores)                   lds_bytes / 2048 * 2048
//         1 transposed read, 8 bytes per lane
//
// An ACCESS is one load and/or store of access_bytes(path); access a of a
// path covers bytes a * access_bytes .. + access_bytes - 1.
//
// Wave rotation.  In step s access a is handled by thread
// ((a % 256) + 64 * s) % 256, so the wave that reads a cell in step s + 1
// is the one after the wave that wrote it in step s: a different SIMD, and
// over the four steps all four.  Work item j of a step is access j, in the
// descending step (hbmmarch::step_descends) access n - 1 - j.  The rotation
// is taken on the ACCESS, not on j: taken on j, the descending step would
// hand half of the cells back to the wave that wrote them ((n-1-a) % 256
// mirrors the wave index, which undoes a shift by one or three waves for
// two of the four).
//
// The march paths prove the cells: every bit holds 0 and 1 and is read back
// both times.  dma and tr16 hold one value per cell and read it once: they
// prove the route, and a bit stuck at the value it was given passes them.
//
// Mismatches are counted per access, and one flipped bit is one mismatch on
// every path.  A mismatch is named by the 16-byte element and the word of
// its lowest differing 32-bit word; on tr16 by the source of the lowest
// differing 16-bit value.
#pragma once

#include <cstdint>

#include "hbm_march.h"
#include "hbm_pattern.h"

namespace ldsmarch {

constexpr int kThreads = 256;
constexpr int kWaveSize = 64;
constexpr int kWaves = kThreads / kWaveSize;

enum Path { kB128 = 0, kB64 = 1, kB32 = 2, kDma = 3, kTr16 = 4 };
constexpr int kPaths = 5;
constexpr const char *kPathNames[kPaths] = {"b128", "b64", "b32", "dma", "tr16"};

// Rounds of all selected paths that one launch runs when the caller passes
// reps = 0; the measurements behind it: profiles/lds_sweep_mi355x.md.
constexpr int kDefaultReps = 2;

constexpr bool is_march(int path) { return path <= kB32; }

constexpr uint32_t access_bytes(int path) {
    return path == kB128 || path == kDma ? 16u : path == kB32 ? 4u : 8u;
}

constexpr int path_steps(int path) {
    return is_march(path) ? hbmmarch::kSteps : path == kDma ? 3 : 2;
}

constexpr uint32_t kDmaBytes = 1024;   // one wave-instruction: 64 lanes x 16
constexpr uint32_t kTr16Bytes = 2048;  // one round: 256 threads x 8

constexpr uint32_t covered_bytes(int path, uint32_t lds_bytes) {
    return path == kDma    ? lds_bytes / kDmaBytes * kDmaBytes
           : path == kTr16 ? lds_bytes / kTr16Bytes * kTr16Bytes
                           : lds_bytes;
}

// accesses of the path's reading step(s)
constexpr uint32_t accesses(int path, uint32_t lds_bytes) {
    return covered_bytes(path, lds_bytes) / access_bytes(path);
}

constexpr uint32_t pattern_bit(int p) { return 1u << p; }

// bit p set: pattern p runs on this path when the caller names none
constexpr uint32_t default_patterns(int path) {
    return path == kB128  ? (1u << hbmmarch::kPatterns) - 1
           : path == kDma ? pattern_bit(hbmmarch::kRandom)
                          : pattern_bit(hbmmarch::kAddress);
}

// dma and tr16 are defined with one pattern each
constexpr bool pattern_is_fixed(int path) { return !is_march(path); }

constexpr bool step_reads(int path, int step) {
    return is_march(path) ? hbmmarch::step_reads(step)
                          : step == path_steps(path) - 1;
}
constexpr bool step_writes(int path, int step) {
    return is_march(path) ? hbmmarch::step_writes(step)
                          : step < path_steps(path) - 1;
}
constexpr bool step_descends(int path, int step) {
    return is_march(path) && hbmmarch::step_descends(step);
}
// a corruption after this step is seen by the step that follows
constexpr bool step_is_followed_by_read(int path, int step) {
    return step >= 0 && step + 1 < path_steps(path) && step_reads(path, step + 1);
}

// ---------------- work assignment ----------------

// The access that work item j of a step over n accesses handles.
constexpr uint32_t step_access(int path, int step, uint32_t n, uint32_t j) {
    return step_descends(path, step) ? n - 1 - j : j;
}

constexpr uint32_t rotation(int step) {
    return (uint32_t)(kWaveSize * step) % kThreads;
}

// The thread that handles access a in step `step`.
constexpr uint32_t thread_of_access(int step, uint32_t a) {
    return (a % kThreads + rotation(step)) % kThreads;
}

// The thread that handles work item j in step `step`.
constexpr uint32_t thread_of_item(int path, int step, uint32_t n, uint32_t j) {
    return thread_of_access(step, step_access(path, step, n, j));
}

// Thread t handles the accesses lane_residue(step, t) + 256 * k below n.
constexpr uint32_t lane_residue(int step, uint32_t t) {
    return (t + kThreads - rotation(step)) % kThreads;
}

// The 16-byte element and first word that access a of a path touches.
constexpr uint32_t access_element(int path, uint32_t a) {
    return a * access_bytes(path) / 16;
}
constexpr uint32_t access_word(int path, uint32_t a) {
    return a * access_bytes(path) % 16 / 4;
}

// ---------------- dma ----------------

// The fill: wave w's instruction k writes KiB number 4k + w, lane l its
// element l, from element 64 * (4k + w) + l of the image.
constexpr uint32_t dma_kib(uint32_t wave, uint32_t k) { return kWaves * k + wave; }
constexpr uint32_t dma_instructions(uint32_t lds_bytes, uint32_t wave) {
    const uint32_t kib = lds_bytes / kDmaBytes;
    return kib > wave ? (kib - wave + kWaves - 1) / kWaves : 0;
}

// ---------------- tr16 ----------------

// Thread t of round k gives the transposed read this byte address.
constexpr uint32_t tr16_address(uint32_t t, uint32_t k) {
    return kTr16Bytes * k + 8 * t;
}
constexpr uint32_t tr16_rounds(uint32_t lds_bytes) { return lds_bytes / kTr16Bytes; }

// The known answer: the byte offset inside round k's 2048 bytes that
// element q (0..3) of thread t's result comes from.  The 16 lanes 16g ..
// 16g + 15 address one contiguous 128-byte block, 4 rows of 16 16-bit
// values with a 32-byte row stride (lane 4q + p: row q, columns 4p..4p+3);
// lane i of the group receives column i, row q in its element q.
constexpr uint32_t tr16_source(uint32_t t, uint32_t q) {
    return 128 * (t / 16) + 32 * q + 2 * (t % 16);
}

// ---------------- data ----------------

// The index that hbmmarch::pattern takes for element e of block `block`.
constexpr uint64_t pattern_index(int path, uint64_t block, uint32_t elems,
                                 uint32_t e) {
    return path == kDma ? e : block * elems + e;
}

// What the reading step `step` of a path expects of an element whose
// pattern is p; what a writing step leaves behind.
constexpr hbmmarch::Element expected_of(int path, hbmmarch::Element p, int step) {
    return is_march(path) ? hbmmarch::expected_of(p, step) : p;
}
constexpr hbmmarch::Element poison() {
    constexpr uint32_t w = 0x01010101u * (uint32_t)hbmpattern::kPoisonByte;
    return {{w, w, w, w}};
}
constexpr hbmmarch::Element to_write_of(int path, hbmmarch::Element p, int step) {
    return is_march(path)               ? hbmmarch::to_write_of(p, step)
           : path == kDma && step == 0 ? poison()
                                        : p;
}

// Word w of an element without indexing at run time (that would cost a
// kernel scratch memory).
constexpr uint32_t word_of(hbmmarch::Element e, uint32_t w) {
    return w == 0 ? e.w[0] : w == 1 ? e.w[1] : w == 2 ? e.w[2] : e.w[3];
}
// The 16-bit value at byte offset `byte` (even, 0..14) of an element.
constexpr uint32_t half_of(hbmmarch::Element e, uint32_t byte) {
    return word_of(e, byte / 4) >> (8 * (byte % 4)) & 0xFFFFu;
}

// ---------------- the first bad access of a block ----------------

// One 64-bit key, smaller for a lower element, so that an atomic minimum
// keeps the whole description of the lowest bad element.  The expected
// word is not stored: the host works it out from the pattern.
// element: 18 bits (4 MiB), path 3, pattern 2, step 2, word 2, half 1 (tr16:
// which 16 bits of the word the value came from), got 32.
constexpr uint64_t pack_first(uint32_t element, uint32_t path, uint32_t pattern,
                              uint32_t step, uint32_t word, uint32_t half,
                              uint32_t got) {
    return (uint64_t)element << 42 | (uint64_t)path << 39 |
           (uint64_t)pattern << 37 | (uint64_t)step << 35 |
           (uint64_t)word << 33 | (uint64_t)half << 32 | got;
}
struct First {
    uint32_t element, path, pattern, step, word, half, got;
};
constexpr First unpack_first(uint64_t key) {
    return {(uint32_t)(key >> 42) & 0x3FFFFu, (uint32_t)(key >> 39) & 7u,
            (uint32_t)(key >> 37) & 3u,       (uint32_t)(key >> 35) & 3u,
            (uint32_t)(key >> 33) & 3u,       (uint32_t)(key >> 32) & 1u,
            (uint32_t)key};
}
constexpr uint32_t kMaxLdsBytes = 1u << 22;  // what 18 bits of element hold

static_assert(thread_of_access(1, 0) == 64 && thread_of_access(3, 255) == 191,
              "one wave further in every step");
static_assert(thread_of_item(kB128, 2, 512, 0) == (255 + 128) % 256,
              "item 0 of the descending step is the last access");
static_assert(lane_residue(1, 64) == 0 && lane_residue(2, 0) == 128, "inverse");
static_assert(covered_bytes(kDma, 2064) == 2048 && covered_bytes(kTr16, 2047) == 0 &&
                  covered_bytes(kB32, 16) == 16,
              "covered bytes");
static_assert(dma_instructions(163840, 0) == 40 && dma_instructions(2048, 2) == 0 &&
                  dma_instructions(5 * 1024, 0) == 2,
              "wave w fills the KiB 4k + w");
static_assert(tr16_source(0, 0) == 0 && tr16_source(1, 0) == 2 &&
                  tr16_source(0, 1) == 32 && tr16_source(16, 0) == 128 &&
                  tr16_source(255, 3) == 2046,
              "lane i of a group: column i, element q = row q");
static_assert(unpack_first(pack_first(10239, kTr16, 3, 3, 3, 1, 0xDEADBEEFu)).element == 10239 &&
                  unpack_first(pack_first(10239, kTr16, 3, 2, 1, 1, 0xDEADBEEFu)).got == 0xDEADBEEFu &&
                  unpack_first(pack_first(1, kTr16, 3, 2, 1, 1, 5)).path == kTr16 &&
                  unpack_first(pack_first(1, kTr16, 3, 2, 1, 1, 5)).half == 1 &&
                  unpack_first(pack_first(0x3FFFF, 0, 0, 0, 0, 0, 0)).element == 0x3FFFF,
              "the key round-trips");
static_assert(pack_first(5, 4, 3, 3, 3, 1, ~0u) < pack_first(6, 0, 0, 0, 0, 0, 0),
              "the lower element is the smaller key");

}  // namespace ldsmarch

// Patterns and march step of the HBM scrub: the one definition that the
// march kernels (probe_kernels.h) write and compare, that hbm_scrub and
// hbm_march_reference (health_probe.hip) state their results in and that
// tests/native/hbm_march_check.cpp runs against a faulty-memory model.
// Plain C++17, no HIP: constexpr functions, usable from device and host
// code alike.
//
// Elements are 16 bytes (uint32_t[4]) and are indexed by a global element
// index i that runs across all slabs of one scrub.
//
//   address   {lo32(i), hi32(i), ~lo32(i), mix32(i)}: words 0 and 1 spell
//             all 64 bits of i, so the pattern is injective and an element
//             displaced by ANY distance (a bad address line) is seen
//   solid     all 0x00000000: with its inverse, every bit holds 0 and 1
//   checker   all 0x55555555: neighbouring bits of a word differ
//   random    four words of splitmix64 over (seed, i): no structure that a
//             fault could share
//
// The inverse of a pattern is the bitwise NOT of all 128 bits.  The march
// runs per pattern p:
//
//   step 0  ascending   reads nothing        writes p
//   step 1  ascending   reads, expecting p   writes ~p
//   step 2  descending  reads, expecting ~p  writes p
//   step 3  ascending   reads, expecting p   writes nothing
//
// A step writes the complement of the value it EXPECTED, never of the value
// it read: one bad read is counted once and does not echo through the steps
// that follow.  In a descending step work item j handles element
// n_total - 1 - j.
#pragma once

#include <cstdint>

namespace hbmmarch {

struct Element {
    uint32_t w[4];
};

enum Pattern { kAddress = 0, kSolid = 1, kChecker = 2, kRandom = 3 };
constexpr int kPatterns = 4;
constexpr const char *kPatternNames[kPatterns] = {"address", "solid", "checker",
                                                  "random"};
constexpr int kSteps = 4;

constexpr bool step_reads(int step) { return step >= 1; }
constexpr bool step_writes(int step) { return step <= 2; }
constexpr bool step_descends(int step) { return step == 2; }

// The element that work item j of a step over n_total elements handles.
constexpr uint64_t step_element(int step, uint64_t n_total, uint64_t j) {
    return step_descends(step) ? n_total - 1 - j : j;
}

constexpr uint64_t kGamma = 0x9E3779B97F4A7C15ull;

// the output function of splitmix64
constexpr uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

constexpr uint32_t mix32(uint64_t i) { return (uint32_t)(mix64(i + kGamma) >> 32); }

// Pattern p at element i, before any inversion.
constexpr Element pattern(int p, uint64_t seed, uint64_t i) {
    switch (p) {
    case kAddress: {
        const uint32_t lo = (uint32_t)i;
        return {{lo, (uint32_t)(i >> 32), ~lo, mix32(i)}};
    }
    case kSolid:
        return {{0u, 0u, 0u, 0u}};
    case kChecker:
        return {{0x55555555u, 0x55555555u, 0x55555555u, 0x55555555u}};
    default: {
        // outputs 2i and 2i + 1 of the splitmix64 stream that starts at seed
        const uint64_t s = seed + (2 * i + 1) * kGamma;
        const uint64_t a = mix64(s), b = mix64(s + kGamma);
        return {{(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b,
                 (uint32_t)(b >> 32)}};
    }
    }
}

constexpr Element inverse(Element e) {
    return {{~e.w[0], ~e.w[1], ~e.w[2], ~e.w[3]}};
}

// The same two questions for a caller that holds e = pattern(p, seed, i)
// already (the kernels work the pattern out once per element).
constexpr Element expected_of(Element e, int step) {
    return step == 2 ? inverse(e) : e;
}
constexpr Element to_write_of(Element e, int step) {
    return step == 1 ? inverse(e) : e;
}

// What step `step` must read at element i.  Step 0 reads nothing; it is
// given the value that it writes.
constexpr Element expected(int p, uint64_t seed, int step, uint64_t i) {
    return expected_of(pattern(p, seed, i), step);
}

// What step `step` writes at element i: the complement of expected() in
// steps 1 and 2.  Step 3 writes nothing; it is given the value that stays.
constexpr Element to_write(int p, uint64_t seed, int step, uint64_t i) {
    return to_write_of(pattern(p, seed, i), step);
}

constexpr bool equal(Element a, Element b) {
    return a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2] &&
           a.w[3] == b.w[3];
}

static_assert(equal(pattern(kAddress, 0, 0x123456789ull),
                    Element{{0x23456789u, 0x1u, ~0x23456789u,
                             mix32(0x123456789ull)}}),
              "fields of the address pattern");
static_assert(equal(to_write(kChecker, 0, 1, 7),
                    inverse(expected(kChecker, 0, 1, 7))) &&
                  equal(to_write(kChecker, 0, 2, 7),
                        inverse(expected(kChecker, 0, 2, 7))),
              "steps 1 and 2 write the complement of what they expect");
// the first output of the reference splitmix64 seeded with 0
static_assert(mix64(kGamma) == 0xE220A8397B1DCDAFull, "splitmix64");

}  // namespace hbmmarch

// gfx950 device code of the deep health probe: the single definition of
// every kernel that health_probe.hip ships and that the mfma_bench /
// hbm_bench sweeps measure.  Device code only (no host policy).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>

#include "hbm_march.h"
#include "hbm_pattern.h"
#include "lds_march.h"
#include "sweep_table.h"
#include "sweep_table_ext.h"

namespace {  // one translation unit per binary; keep the kernels internal

// ---------------- wavefront probe ----------------

__global__ void wave_probe_kernel(unsigned long long *out) {
    unsigned long long active = __ballot(1);
    if (threadIdx.x == 0) {
        out[0] = active;
        out[1] = warpSize;
    }
}

// ---------------- MFMA probe ----------------

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;

__device__ inline __bf16 small_int_bf16(int v) {
    return (__bf16)(float)v;  // small ints are exact in bf16
}

// One wave computes D = A*B with v_mfma_f32_16x16x32_bf16 three times:
//  pass 0: A == 1, B == 0.5     -> every D element must equal 16.0
//  pass 1: A[lane][r] = pattern, B == 1 -> sum(D) == 16 * sum(A) (exact)
//  pass 2: asymmetric A AND B   -> element-wise check against a host
//          matmul through the documented lane maps (tests/test_gpu.py)
__global__ void mfma_probe_kernel(float *d_out /* [3][256] */) {
#if defined(__gfx950__)
    int lane = threadIdx.x;
    if (lane >= 64) return;

    for (int pass = 0; pass < 3; ++pass) {
        bf16x8 a, b;
        for (int r = 0; r < 8; ++r) {
            if (pass == 0) {
                a[r] = small_int_bf16(1);
                b[r] = (__bf16)0.5f;
            } else if (pass == 1) {
                a[r] = small_int_bf16(((lane * 8 + r) % 7) - 3);
                b[r] = small_int_bf16(1);
            } else {
                a[r] = small_int_bf16(((lane * 8 + r) % 7) - 3);
                b[r] = small_int_bf16(((lane * 5 + r * 3) % 11) - 5);
            }
        }
        f32x4 c = {0.f, 0.f, 0.f, 0.f};
        f32x4 d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
        for (int r = 0; r < 4; ++r)
            d_out[pass * 256 + lane * 4 + r] = d[r];
    }
#else
    if (threadIdx.x == 0) d_out[0] = -1.0f;
#endif
}

// ---------------- MFMA peak throughput ----------------

// Back-to-back v_mfma_f32_32x32x16_bf16 on NACC independent accumulators.
// The probe ships <2>: in the recorded mfma_bench sweep
// (profiles/r01_bench_mi355x.md) 2 accumulators at 512 threads x 2
// blocks/CU was fastest (2043 TF/s) — partner waves on each SIMD provide
// the remaining issue cover (guide: §Two waves per SIMD).
// ZERO feeds zero operands (the sweep's DVFS demonstration).
// store != 0 (mfma_peak_check, the tests) writes the accumulators instead of
// discarding them: wave w of block b puts acc[k][r] of its lane l at
// out[(((b * waves + w) * NACC + k) * 16 + r) * 64 + l], waves = blockDim.x /
// 64, so out holds blocks * waves * NACC * 16 * 64 floats.  The operands are
// small integers: after iters rounds every acc[k] is exactly iters * (A @ B).
template <int NACC, bool ZERO = false>
__global__ void __launch_bounds__(512, 2)
mfma_peak_kernel(float *out, int iters, int store) {
#if defined(__gfx950__)
    int lane = threadIdx.x & 63;
    bf16x8 a, b;
    for (int r = 0; r < 8; ++r) {
        a[r] = ZERO ? (__bf16)0.0f : (__bf16)(float)(((lane + r) % 5) - 2);
        b[r] = ZERO ? (__bf16)0.0f : (__bf16)(float)(((lane * 3 + r) % 7) - 3);
    }
    f32x16 acc[NACC];
    for (int k = 0; k < NACC; ++k) acc[k] = f32x16{};
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int k = 0; k < NACC; ++k)
            acc[k] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[k], 0, 0, 0);
    }
    if (store) {
        const size_t wave = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
        float *o = out + wave * NACC * 16 * 64 + lane;
        for (int k = 0; k < NACC; ++k)
            for (int r = 0; r < 16; ++r) o[(k * 16 + r) * 64] = acc[k][r];
        return;
    }
    float s = 0;
    for (int k = 0; k < NACC; ++k)
        for (int r = 0; r < 16; ++r) s += acc[k][r];
    if (s == -1.0f) out[blockIdx.x] = s;  // never true: defeats DCE only
#else
    (void)out;
    (void)iters;
    (void)store;
#endif
}

// ---------------- LDS probe ----------------

// Every thread of a block reads every word once, so one wrong word in one
// block adds exactly blockDim.x to err_count.  corrupt_block / corrupt_word
// (-1 = off) make thread 0 of that block xor corrupt_mask into that word
// after the fill: a bad LDS cell simulated on healthy hardware (lds_check).
__global__ void lds_probe_kernel(uint32_t *err_count, int lds_words,
                                 int corrupt_block, int corrupt_word,
                                 uint32_t corrupt_mask) {
    extern __shared__ uint32_t lds[];
    int tid = threadIdx.x;
    int nthreads = blockDim.x;
    for (int i = tid; i < lds_words; i += nthreads)
        lds[i] = (uint32_t)i * 2654435761u + blockIdx.x;
    __syncthreads();
    if (tid == 0 && (int)blockIdx.x == corrupt_block && corrupt_word >= 0 &&
        corrupt_word < lds_words)
        lds[corrupt_word] ^= corrupt_mask;
    __syncthreads();
    // read back with a stride so each thread checks other threads' writes
    uint32_t errors = 0;
    for (int i = tid * 17 % lds_words, n = 0; n < lds_words; ++n, i = (i + 1) % lds_words)
        if (lds[i] != (uint32_t)i * 2654435761u + blockIdx.x) ++errors;
    if (errors) atomicAdd(err_count, errors);
}

// ---------------- HBM streaming copy ----------------

// Exact-fit one-shot nontemporal stream: thread t moves exactly 4 float4s
// at grid-stride offsets, no loop bookkeeping; threads whose fourth element
// would pass n fall to the grid-stride tail.  nt hints keep the one-shot
// stream out of L1/L2, 4 independent loads per thread hide HBM latency —
// fastest variant of the hbm_bench sweep, 6.22 TB/s on MI355X (99% of the
// 6.29 TB/s float4-copy ceiling; profiles/r01_bench_mi355x.md).
// PRECONDITION: 4 * gridDim.x * blockDim.x >= n.  A thread on the 4-wide path
// never loops, so a smaller grid leaves elements from 4 * stride on uncopied;
// hbm_copy_blocks() below is the grid of the probe and of hbm_bench;
// hbm_copy_check refuses any other grid that is too small.
__global__ void hbm_copy_kernel(const float4 *__restrict__ src4,
                                float4 *__restrict__ dst4, size_t n) {
    const f32x4 *__restrict__ src = reinterpret_cast<const f32x4 *>(src4);
    f32x4 *__restrict__ dst = reinterpret_cast<f32x4 *>(dst4);
    size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i + 3 * stride < n) {
        f32x4 a = __builtin_nontemporal_load(&src[i]);
        f32x4 b = __builtin_nontemporal_load(&src[i + stride]);
        f32x4 c = __builtin_nontemporal_load(&src[i + 2 * stride]);
        f32x4 d = __builtin_nontemporal_load(&src[i + 3 * stride]);
        __builtin_nontemporal_store(a, &dst[i]);
        __builtin_nontemporal_store(b, &dst[i + stride]);
        __builtin_nontemporal_store(c, &dst[i + 2 * stride]);
        __builtin_nontemporal_store(d, &dst[i + 3 * stride]);
    } else {
        for (; i < n; i += stride)
            __builtin_nontemporal_store(__builtin_nontemporal_load(&src[i]),
                                        &dst[i]);
    }
}

// The grid of hbm_copy_kernel for n elements: one thread per 4 float4s,
// rounded UP so that the kernel's precondition holds for every n, and never
// fewer than 1024 blocks (>>256 workgroups for all 8 XCDs).
constexpr size_t hbm_copy_blocks(size_t n, int threads = 256) {
    const size_t per_block = (size_t)threads * 4;
    const size_t want = (n + per_block - 1) / per_block;
    return want < 1024 ? 1024 : want;
}

// buf[i] = hbmpattern::value(i): exact in fp32 and different for every
// i < 2^48 (hbm_pattern.h), so a copy can be checked bit for bit and a
// displaced element cannot pass for the right one.
__global__ void fill_pattern_kernel(float4 *buf, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const hbmpattern::Value v = hbmpattern::value(i);
        buf[i] = make_float4(v.x, v.y, v.z, v.w);
    }
}

// Compares all four components of all n elements of buf with the pattern,
// bit for bit.  The host sets *mismatches = 0 and *first_bad = ~0 before the
// launch; afterwards they hold the number of differing elements and the
// lowest differing index.
__global__ void verify_pattern_kernel(const float4 *__restrict__ buf, size_t n,
                                      unsigned long long *mismatches,
                                      unsigned long long *first_bad) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    unsigned long long bad = 0, first = ~0ull;
    for (; i < n; i += stride) {
        const float4 v = buf[i];
        if (!hbmpattern::matches(i, v.x, v.y, v.z, v.w)) {
            if (!bad) first = i;  // i only grows
            ++bad;
        }
    }
    if (bad) {
        atomicAdd(mismatches, bad);
        atomicMin(first_bad, first);
    }
}

// ---------------- HBM scrub: in-place march over one slab ----------------

// What the march kernels of one scrub report into; the host zeroes it and
// sets first_bad = ~0 before the first launch.
struct MarchReport {
    unsigned long long mismatches;  // elements that read back wrong
    unsigned long long first_bad;   // lowest such global index
    uint32_t bad_bits[4];           // OR of got ^ expected, per word
    uint32_t n_records;             // slots claimed, may pass max_records
    uint32_t reserved;
};

// One wrong element, written into a claimed slot with ordinary stores.
struct MarchRecord {
    uint32_t pattern, step;
    unsigned long long index;  // global element index
    uint32_t word;             // lowest differing word
    uint32_t got, expected;    // that word
    uint32_t reserved;
};

// Elements per entry of the per-range counters: 2 MiB of 16-byte elements.
constexpr int kMarchRangeShift = 17;

// One launch: which step of which pattern, over which slab.
struct MarchParams {
    int pattern, step;              // hbmmarch::Pattern, 0..3
    unsigned long long seed;
    unsigned long long base;        // global index of the slab's element 0
    size_t n;                       // elements of this slab
    uint32_t max_records;
};

using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;

enum MarchMode { kMarchWrite = 0, kMarchRW = 1, kMarchRead = 2 };

// The cold path: element `index` read back as got, not as want.
__device__ __noinline__ void march_report(u32x4 got, u32x4 want,
                                          unsigned long long index,
                                          uint32_t pattern, uint32_t step,
                                          uint32_t max_records, MarchReport *rep,
                                          MarchRecord *records,
                                          uint32_t *range_bad) {
    // no array indexed at run time: that would cost the kernel scratch memory
    const uint32_t d0 = got.x ^ want.x, d1 = got.y ^ want.y,
                   d2 = got.z ^ want.z, d3 = got.w ^ want.w;
    atomicAdd(&rep->mismatches, 1ull);
    atomicMin(&rep->first_bad, index);
    if (d0) atomicOr(&rep->bad_bits[0], d0);
    if (d1) atomicOr(&rep->bad_bits[1], d1);
    if (d2) atomicOr(&rep->bad_bits[2], d2);
    if (d3) atomicOr(&rep->bad_bits[3], d3);
    const int word = d0 ? 0 : d1 ? 1 : d2 ? 2 : 3;
    const uint32_t got_word = d0 ? got.x : d1 ? got.y : d2 ? got.z : got.w;
    atomicAdd(&range_bad[index >> kMarchRangeShift], 1u);
    // the plain read keeps a wholly bad slab from wrapping the counter
    if (*(volatile uint32_t *)&rep->n_records < max_records) {
        const uint32_t slot = atomicAdd(&rep->n_records, 1u);
        if (slot < max_records) {
            MarchRecord r;
            r.pattern = pattern;
            r.step = step;
            r.index = index;
            r.word = (uint32_t)word;
            r.got = got_word;
            r.expected = got_word ^ (d0 ? d0 : d1 ? d1 : d2 ? d2 : d3);
            r.reserved = 0;
            records[slot] = r;
        }
    }
}

// One march step (hbm_march.h) over one slab, in place, in the shape of
// hbm_copy_kernel: 16 B per lane, work item j of the slab's n handles
// element j (n - 1 - j in the descending step), thread t takes the work
// items t + k * stride, k = 0..3, with its four nontemporal loads in flight
// before the first compare and store; threads whose fourth item would pass
// n fall to the grid-stride tail.  kMarchWrite (step 0) only stores,
// kMarchRead (step 3) only loads and compares, kMarchRW (steps 1, 2) loads,
// compares with hbmmarch::expected_of and stores hbmmarch::to_write_of to
// the same address.  NT = false gives plain stores and loads (hbm_bench).
// PRECONDITION, as for hbm_copy_kernel: 4 * gridDim.x * blockDim.x >= n.
template <int MODE, bool NT = true>
__global__ void march_kernel(u32x4 *__restrict__ slab, MarchParams a,
                             MarchReport *rep, MarchRecord *records,
                             uint32_t *range_bad) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool down = hbmmarch::step_descends(a.step);
    auto element = [&](size_t j) { return down ? a.n - 1 - j : j; };
    auto load = [&](size_t e) {
        return NT ? __builtin_nontemporal_load(&slab[e]) : slab[e];
    };
    // the pattern once per element; check and store derive from it
    auto finish = [&](size_t e, u32x4 got) {
        const hbmmarch::Element p =
            hbmmarch::pattern(a.pattern, a.seed, a.base + e);
        if (MODE != kMarchWrite) {
            const hbmmarch::Element v = hbmmarch::expected_of(p, a.step);
            const u32x4 want = {v.w[0], v.w[1], v.w[2], v.w[3]};
            if ((got.x ^ want.x) | (got.y ^ want.y) | (got.z ^ want.z) |
                (got.w ^ want.w))
                march_report(got, want, a.base + e, (uint32_t)a.pattern,
                             (uint32_t)a.step, a.max_records, rep, records,
                             range_bad);
        }
        if (MODE != kMarchRead) {
            const hbmmarch::Element v = hbmmarch::to_write_of(p, a.step);
            const u32x4 x = {v.w[0], v.w[1], v.w[2], v.w[3]};
            if (NT)
                __builtin_nontemporal_store(x, &slab[e]);
            else
                slab[e] = x;
        }
    };
    const u32x4 none = {0, 0, 0, 0};
    if (t + 3 * stride < a.n) {
        const size_t e0 = element(t), e1 = element(t + stride),
                     e2 = element(t + 2 * stride), e3 = element(t + 3 * stride);
        u32x4 g0 = none, g1 = none, g2 = none, g3 = none;
        if (MODE != kMarchWrite) {
            g0 = load(e0);
            g1 = load(e1);
            g2 = load(e2);
            g3 = load(e3);
        }
        finish(e0, g0);
        finish(e1, g1);
        finish(e2, g2);
        finish(e3, g3);
    } else {
        for (size_t j = t; j < a.n; j += stride) {
            const size_t e = element(j);
            finish(e, MODE != kMarchWrite ? load(e) : none);
        }
    }
}

constexpr int march_mode_of_step(int step) {
    return step == 0 ? kMarchWrite : step == 3 ? kMarchRead : kMarchRW;
}

// ---------------- CU sweep: known-answer MFMA on every SIMD ----------------

// One record per wave, written by that wave with plain stores; the host
// zeroes the array before the launch.
struct SweepRecord {
    uint32_t hw_id;       // HW_REG_HW_ID, whole register
    uint32_t xcc_id;      // HW_REG_XCC_ID
    uint32_t fail_pipes;  // bit p: pipe p gave a wrong result
    uint32_t bad_lanes_lo, bad_lanes_hi;  // OR of the mismatch ballots
    // first failure, valid when fail_pipes != 0
    uint32_t first_pipe, first_t, first_lane, first_reg;
    uint32_t first_got, first_expected;
    uint32_t reserved;
};

// where the inject hook flips its one bit
constexpr int kSweepInjectLane = 5;
constexpr int kSweepInjectReg = 1;
constexpr uint32_t kSweepInjectBit = 1u << 3;

using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x8 = __attribute__((ext_vector_type(8))) int;

// D = A * B + zero for pipe P (cusweep::kPipeDesc) from this lane's packed
// fragments, as result register bits.  zero is 0 that the compiler cannot
// see through, so the product is computed again in every round.  Vector
// elements go through __float_as_uint: __builtin_bit_cast of o[r] read
// element 0 for every r (hipcc 7.x), which the first hardware run showed.
template <int P>
__device__ inline void sweep_mfma(const unsigned char *a, const unsigned char *b,
                                  uint32_t zero, uint32_t *d) {
#if defined(__gfx950__)
    constexpr int R = cusweep::kPipeDesc[P].regs;
    const float fz = __uint_as_float(zero);
    if constexpr (P == 1) {
        f32x16 c;
        for (int r = 0; r < 16; ++r) c[r] = fz;
        f32x16 o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            *reinterpret_cast<const bf16x8 *>(a),
            *reinterpret_cast<const bf16x8 *>(b), c, 0, 0, 0);
        for (int r = 0; r < R; ++r) d[r] = __float_as_uint(o[r]);
    } else if constexpr (P == 4) {
        const int iz = (int)zero;
        i32x4 c = {iz, iz, iz, iz};
        i32x4 o = __builtin_amdgcn_mfma_i32_16x16x64_i8(
            *reinterpret_cast<const i32x4 *>(a),
            *reinterpret_cast<const i32x4 *>(b), c, 0, 0, 0);
        for (int r = 0; r < R; ++r) d[r] = (uint32_t)o[r];
    } else {
        f32x4 c = {fz, fz, fz, fz};
        f32x4 o;
        if constexpr (P == 0) {
            o = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                *reinterpret_cast<const bf16x8 *>(a),
                *reinterpret_cast<const bf16x8 *>(b), c, 0, 0, 0);
        } else if constexpr (P == 2) {
            o = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                *reinterpret_cast<const f16x8 *>(a),
                *reinterpret_cast<const f16x8 *>(b), c, 0, 0, 0);
        } else if constexpr (P == 3) {
            o = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
                *reinterpret_cast<const long *>(a),
                *reinterpret_cast<const long *>(b), c, 0, 0, 0);
        } else {
            static_assert(P == 5, "six pipes");
            // fp8 (e4m3) formats on both sides; E8M0 scale 127 = 1.0 in all
            // four bytes of the scale register, so the byte select is moot
            const int one = 0x7F7F7F7F;
            o = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                *reinterpret_cast<const i32x8 *>(a),
                *reinterpret_cast<const i32x8 *>(b), c, 0, 0, 0, one, 0, one);
        }
        for (int r = 0; r < R; ++r) d[r] = __float_as_uint(o[r]);
    }
#else
    (void)a;
    (void)b;
    for (int r = 0; r < cusweep::kPipeDesc[P].regs; ++r) d[r] = zero;
#endif
}

using f64x4 = __attribute__((ext_vector_type(4))) double;
using i32x16 = __attribute__((ext_vector_type(16))) int;

// The 8 operand registers of an f8f6f4 fragment.  The tables pack a lane's
// fp4 / fp6 fragment into 16 / 24 bytes, so the address is only 4-byte
// aligned and the words past the fragment are the next lane's (a pad that
// the instruction does not read for these formats).
__device__ inline i32x8 load_frag8(const unsigned char *p) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(p);
    i32x8 v;
    for (int i = 0; i < 8; ++i) v[i] = (int)w[i];
    return v;
}

// Set mx (cusweepx::kMxDesc): block-scaled v_mfma_scale_f32_*_f8f6f4 with
// the lane's scale words sa / sb and the byte selects SA / SB, which the
// instruction takes as immediates (op_sel, op_sel_hi).
template <int P, int SA, int SB>
__device__ inline void mx_mfma(const unsigned char *a, const unsigned char *b,
                               uint32_t sa, uint32_t sb, uint32_t zero,
                               uint32_t *d) {
#if defined(__gfx950__)
    constexpr int CA = cusweepx::kFmt[cusweepx::kMxDesc[P].a].code;
    constexpr int CB = cusweepx::kFmt[cusweepx::kMxDesc[P].b].code;
    const float fz = __uint_as_float(zero);
    const i32x8 va = load_frag8(a), vb = load_frag8(b);
    if constexpr (cusweepx::kMxDesc[P].M == 16) {
        f32x4 c = {fz, fz, fz, fz};
        f32x4 o = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            va, vb, c, CA, CB, SA, (int)sa, SB, (int)sb);
        for (int r = 0; r < 4; ++r) d[r] = __float_as_uint(o[r]);
    } else {
        f32x16 c;
        for (int r = 0; r < 16; ++r) c[r] = fz;
        f32x16 o = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
            va, vb, c, CA, CB, SA, (int)sa, SB, (int)sb);
        for (int r = 0; r < 16; ++r) d[r] = __float_as_uint(o[r]);
    }
#else
    (void)a;
    (void)b;
    (void)sa;
    (void)sb;
    for (int r = 0; r < cusweepx::regs(cusweepx::kMx, P); ++r) d[r] = zero;
#endif
}

// Set wide (cusweepx::kWideDesc): bf8, the 32x32 shapes of f16 / fp8 / i8,
// f64 and f32-input.  An f64 result is two result registers, low word first.
template <int P>
__device__ inline void wide_mfma(const unsigned char *a, const unsigned char *b,
                                 uint32_t zero, uint32_t *d) {
#if defined(__gfx950__)
    const float fz = __uint_as_float(zero);
    if constexpr (P == 0) {
        f32x4 c = {fz, fz, fz, fz};
        f32x4 o = __builtin_amdgcn_mfma_f32_16x16x32_bf8_bf8(
            *reinterpret_cast<const long *>(a),
            *reinterpret_cast<const long *>(b), c, 0, 0, 0);
        for (int r = 0; r < 4; ++r) d[r] = __float_as_uint(o[r]);
    } else if constexpr (P == 1 || P == 2) {
        f32x16 c;
        for (int r = 0; r < 16; ++r) c[r] = fz;
        f32x16 o;
        if constexpr (P == 1)
            o = __builtin_amdgcn_mfma_f32_32x32x16_f16(
                *reinterpret_cast<const f16x8 *>(a),
                *reinterpret_cast<const f16x8 *>(b), c, 0, 0, 0);
        else
            o = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(
                *reinterpret_cast<const long *>(a),
                *reinterpret_cast<const long *>(b), c, 0, 0, 0);
        for (int r = 0; r < 16; ++r) d[r] = __float_as_uint(o[r]);
    } else if constexpr (P == 3) {
        const int iz = (int)zero;
        i32x16 c;
        for (int r = 0; r < 16; ++r) c[r] = iz;
        i32x16 o = __builtin_amdgcn_mfma_i32_32x32x32_i8(
            *reinterpret_cast<const i32x4 *>(a),
            *reinterpret_cast<const i32x4 *>(b), c, 0, 0, 0);
        for (int r = 0; r < 16; ++r) d[r] = (uint32_t)o[r];
    } else if constexpr (P == 4) {
        const double dz = __longlong_as_double((long long)zero);
        f64x4 c = {dz, dz, dz, dz};
        f64x4 o = __builtin_amdgcn_mfma_f64_16x16x4f64(
            *reinterpret_cast<const double *>(a),
            *reinterpret_cast<const double *>(b), c, 0, 0, 0);
        for (int r = 0; r < 4; ++r) {
            const unsigned long long bits =
                (unsigned long long)__double_as_longlong(o[r]);
            d[2 * r] = (uint32_t)bits;
            d[2 * r + 1] = (uint32_t)(bits >> 32);
        }
    } else {
        static_assert(P == 5, "six pipes");
        f32x4 c = {fz, fz, fz, fz};
        f32x4 o = __builtin_amdgcn_mfma_f32_16x16x4f32(
            *reinterpret_cast<const float *>(a),
            *reinterpret_cast<const float *>(b), c, 0, 0, 0);
        for (int r = 0; r < 4; ++r) d[r] = __float_as_uint(o[r]);
    }
#else
    (void)a;
    (void)b;
    for (int r = 0; r < cusweepx::regs(cusweepx::kWide, P); ++r) d[r] = zero;
#endif
}

// pipe P of set SET (cusweepx::Set): the base set's sweep_mfma or one of the
// two above
template <int SET, int P, int SA, int SB>
__device__ inline void set_mfma(const unsigned char *a, const unsigned char *b,
                                uint32_t sa, uint32_t sb, uint32_t zero,
                                uint32_t *d) {
    if constexpr (SET == cusweepx::kBase)
        sweep_mfma<P>(a, b, zero, d);
    else if constexpr (SET == cusweepx::kMx)
        mx_mfma<P, SA, SB>(a, b, sa, sb, zero, d);
    else
        wide_mfma<P>(a, b, zero, d);
}

// wave-uniform running state of one wave's sweep
struct SweepWaveState {
    uint32_t fail_pipes = 0;
    unsigned long long bad_lanes = 0;
    bool have_first = false;
};

// Compares this lane's R result registers d of test t of unit `unit` (a pipe
// of the CU sweep, an op of the VALU sweep) with want, bit for bit, after the
// inject hook has flipped its one bit of register inject_reg of one lane;
// folds the outcome into the wave's state and, for the wave's first failure,
// lets the lowest bad lane report its registers.
template <int R>
__device__ inline void sweep_check(int unit, int t, int lane, uint32_t *d,
                                   const uint32_t *want, bool inject,
                                   int inject_reg, SweepWaveState &st,
                                   SweepRecord *rec) {
    if (inject && lane == kSweepInjectLane) d[inject_reg] ^= kSweepInjectBit;
    int bad_reg = -1;  // the lowest mismatching register of this lane
    uint32_t got = 0, expected = 0;
#pragma unroll
    for (int r = R - 1; r >= 0; --r)
        if (d[r] != want[r]) {
            bad_reg = r;
            got = d[r];
            expected = want[r];
        }
    unsigned long long ballot = __ballot(bad_reg >= 0);
    if (ballot) {
        st.fail_pipes |= 1u << unit;
        st.bad_lanes |= ballot;
        if (!st.have_first) {
            st.have_first = true;
            // the lowest bad lane reports its own registers
            if (lane == __ffsll((long long)ballot) - 1) {
                rec->first_pipe = unit;
                rec->first_t = t;
                rec->first_lane = lane;
                rec->first_reg = bad_reg;
                rec->first_got = got;
                rec->first_expected = expected;
            }
        }
    }
}

// test t of pipe P of set SET; SA / SB are that test's byte selects (mx)
template <int SET, int P, int SA, int SB>
__device__ inline void sweep_test(const unsigned char *table, int t, int lane,
                                  uint32_t zero, bool inject,
                                  SweepWaveState &st, SweepRecord *rec) {
    constexpr int FA = cusweepx::frag_bytes(SET, P, 0),
                  FB = cusweepx::frag_bytes(SET, P, 1),
                  R = cusweepx::regs(SET, P);
    const unsigned char *a = table + cusweepx::test_offset(SET, P, t);
    const unsigned char *b = a + cusweep::kLanes * FA;
    const uint32_t *want = reinterpret_cast<const uint32_t *>(b + cusweep::kLanes * FB);
    uint32_t sa = 0, sb = 0;
    if constexpr (cusweepx::scaled(SET)) {
        sa = want[lane];
        sb = want[cusweep::kLanes + lane];
        want += 2 * cusweep::kLanes;
    }
    want += lane * R;
    uint32_t d[R];
    set_mfma<SET, P, SA, SB>(a + lane * FA, b + lane * FB, sa, sb, zero, d);
    sweep_check<R>(P, t, lane, d, want, inject, kSweepInjectReg, st, rec);
}

// the tests of an mx pipe, unrolled: each has its own byte selects
template <int P, int... T>
__device__ inline void sweep_mx_tests(std::integer_sequence<int, T...>,
                                      const unsigned char *table, int lane,
                                      uint32_t zero, bool inject,
                                      SweepWaveState &st, SweepRecord *rec) {
    (sweep_test<cusweepx::kMx, P, cusweepx::sel_a(T), cusweepx::sel_b(T)>(
         table, T, lane, zero, inject, st, rec),
     ...);
}

template <int SET, int P>
__device__ inline void sweep_pipe(const unsigned char *table, int lane,
                                  uint32_t zero, bool inject,
                                  SweepWaveState &st, SweepRecord *rec) {
    if constexpr (SET == cusweepx::kMx) {
        sweep_mx_tests<P>(std::make_integer_sequence<int, cusweepx::kTests>{},
                          table, lane, zero, inject, st, rec);
    } else {
        for (int t = 0; t < cusweepx::n_tests(SET); ++t)
            sweep_test<SET, P, 0, 0>(table, t, lane, zero, inject, st, rec);
    }
}

template <int SET, int... P>
__device__ inline void sweep_pipes(std::integer_sequence<int, P...>,
                                   const unsigned char *table, int lane,
                                   uint32_t zero, bool mine, int inject_pipe,
                                   SweepWaveState &st, SweepRecord *rec) {
    (sweep_pipe<SET, P>(table, lane, zero, mine && inject_pipe == P, st, rec), ...);
}

// One 4-wave block per CU, for pipe set SET (cusweepx::Set: the base set of
// sweep_table.h, or mx / wide of sweep_table_ext.h).  The block copies the
// set's packed operand and expected-result table into LDS; the launch asks
// for cusweepx::lds_bytes(SET) of dynamic LDS, more than half of the CU's
// 160 KiB, so no two sweep blocks share a CU.  Each wave then reads where it
// runs from the hardware id registers, runs reps rounds of every pipe's
// known-answer products on its SIMD and compares every result register bit
// for bit.  Nothing here depends on where a block lands and no block waits
// for another; the host works out the coverage from the records.
// inject_block / inject_wave / inject_pipe (-1 = off) make that one wave
// flip one bit of one result register of that pipe before comparing: a bad
// pipe simulated on healthy hardware.
template <int SET>
__global__ void __launch_bounds__(256)
cu_sweep_kernel(const uint4 *__restrict__ table, SweepRecord *records, int reps,
                int inject_block, int inject_wave, int inject_pipe) {
    extern __shared__ uint4 sweep_lds[];
    for (int i = threadIdx.x; i < cusweepx::table_bytes(SET) / 16; i += blockDim.x)
        sweep_lds[i] = table[i];
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    SweepRecord *rec = &records[blockIdx.x * 4 + wave];
    const uint32_t hw_id = __builtin_amdgcn_s_getreg(4 | 31 << 11);
    const uint32_t xcc_id = __builtin_amdgcn_s_getreg(20 | 3 << 11);
    const bool mine = (int)blockIdx.x == inject_block && wave == inject_wave;
    const unsigned char *tbl = reinterpret_cast<const unsigned char *>(sweep_lds);

    SweepWaveState st;
    for (int rep = 0; rep < reps; ++rep) {
        uint32_t zero = 0;
        asm volatile("" : "+v"(zero));
        sweep_pipes<SET>(std::make_integer_sequence<int, cusweepx::n_pipes(SET)>{},
                         tbl, lane, zero, mine, inject_pipe, st, rec);
    }
    if (lane == 0) {
        rec->hw_id = hw_id;
        rec->xcc_id = xcc_id;
        rec->fail_pipes = st.fail_pipes;
        rec->bad_lanes_lo = (uint32_t)st.bad_lanes;
        rec->bad_lanes_hi = (uint32_t)(st.bad_lanes >> 32);
    }
}

// One wave, one product of pipe P of set SET from caller-supplied packed
// fragments and scale words (mfma_raw): out[lane * regs + r].  a and b are
// readable for 32 bytes from every lane's fragment.
template <int SET, int P, int SA, int SB>
__global__ void __launch_bounds__(64)
mfma_raw_kernel(const unsigned char *__restrict__ a,
                const unsigned char *__restrict__ b,
                const uint32_t *__restrict__ scale_a,
                const uint32_t *__restrict__ scale_b, uint32_t *out) {
    constexpr int R = cusweepx::regs(SET, P);
    const int lane = threadIdx.x;
    uint32_t zero = 0;
    asm volatile("" : "+v"(zero));
    uint32_t d[R];
    set_mfma<SET, P, SA, SB>(a + lane * cusweepx::frag_bytes(SET, P, 0),
                             b + lane * cusweepx::frag_bytes(SET, P, 1),
                             scale_a[lane], scale_b[lane], zero, d);
    for (int r = 0; r < R; ++r) out[lane * R + r] = d[r];
}

// ---------------- LDS sweep: march over one CU's whole LDS ----------------

// A few of a block's bad accesses, each in a claimed slot.
struct LdsSlot {
    uint32_t meta;  // path | pattern << 4 | step << 8 | word << 12
    uint32_t element;
    uint32_t got, expected;  // the lowest differing word
};
constexpr int kLdsSlots = 4;

// One record per block; the host zeroes the array and sets first = ~0
// before the launch.
struct LdsBlockRecord {
    uint32_t hw_id[4], xcc_id[4];  // per wave: HW_REG_HW_ID, HW_REG_XCC_ID
    uint32_t mismatches;           // accesses that read back wrong
    uint32_t n_slots;              // slots claimed, may pass kLdsSlots
    uint32_t bad_bits[4];          // OR of got ^ expected, per word
    unsigned long long first;      // ldsmarch::pack_first of the lowest element
    LdsSlot slots[kLdsSlots];
};

enum LdsCorruption { kLdsNone = 0, kLdsFlip = 1, kLdsAlias = 2 };

struct LdsSweepParams {
    uint32_t lds_bytes;  // a multiple of 16
    int reps;
    uint32_t patterns[ldsmarch::kPaths];  // bit p: pattern p runs; 0: path off
    unsigned long long seed;
    const u32x4 *image;  // the dma path's source, covered_bytes(kDma) of it
    // one corruption, in rep 0 (c_block = -1: none)
    int c_block, c_path, c_pattern, c_step, c_kind;
    uint32_t c_element, c_word, c_bit;
    int c_distance;
};

using u32x2 = __attribute__((ext_vector_type(2))) uint32_t;
using i16x4 = __attribute__((ext_vector_type(4))) short;

// The cold path: one access read back wrong.  got and want hold the
// access's words at their place in the 16-byte element, zero elsewhere;
// more is ORed into the bad bits of the lowest differing word (tr16: the
// other 16-bit values of the same read, from the same `half` of that word).
__device__ __noinline__ void lds_report(LdsBlockRecord *rec, uint32_t path,
                                        uint32_t pattern, uint32_t step,
                                        uint32_t element, u32x4 got, u32x4 want,
                                        uint32_t more, uint32_t half = 0) {
    // no array indexed at run time: that would cost the kernel scratch memory
    const uint32_t d0 = got.x ^ want.x, d1 = got.y ^ want.y,
                   d2 = got.z ^ want.z, d3 = got.w ^ want.w;
    const uint32_t word = d0 ? 0 : d1 ? 1 : d2 ? 2 : 3;
    atomicAdd(&rec->mismatches, 1u);
    if (d0 | (word == 0 ? more : 0)) atomicOr(&rec->bad_bits[0], d0 | (word == 0 ? more : 0));
    if (d1 | (word == 1 ? more : 0)) atomicOr(&rec->bad_bits[1], d1 | (word == 1 ? more : 0));
    if (d2 | (word == 2 ? more : 0)) atomicOr(&rec->bad_bits[2], d2 | (word == 2 ? more : 0));
    if (d3 | (word == 3 ? more : 0)) atomicOr(&rec->bad_bits[3], d3 | (word == 3 ? more : 0));
    const uint32_t got_word = d0 ? got.x : d1 ? got.y : d2 ? got.z : got.w;
    const uint32_t want_word = d0 ? want.x : d1 ? want.y : d2 ? want.z : want.w;
    atomicMin(&rec->first, (unsigned long long)ldsmarch::pack_first(
                               element, path, pattern, step, word, half, got_word));
    // the plain read keeps a wholly bad block from wrapping the counter
    if (*(volatile uint32_t *)&rec->n_slots < (uint32_t)kLdsSlots) {
        const uint32_t slot = atomicAdd(&rec->n_slots, 1u);
        if (slot < (uint32_t)kLdsSlots) {
            LdsSlot s;
            s.meta = path | pattern << 4 | step << 8 | word << 12;
            s.element = element;
            s.got = got_word;
            s.expected = want_word;
            rec->slots[slot] = s;
        }
    }
}

// Thread 0 of the chosen block damages its own block's LDS once, after
// step `step` of that path and pattern in rep 0; the caller's barrier has
// passed and a second one follows, on a block-uniform condition.
__device__ inline void lds_corrupt(u32x4 *lds, const LdsSweepParams &a, int rep,
                                   int path, int pattern, int step) {
    if (rep == 0 && (int)blockIdx.x == a.c_block && path == a.c_path &&
        pattern == a.c_pattern && step == a.c_step) {
        const uint32_t elems = a.lds_bytes / 16;
        const long long other = (long long)a.c_element + a.c_distance;
        if (threadIdx.x == 0 && a.c_element < elems) {
            if (a.c_kind == kLdsFlip && a.c_word < 4)
                reinterpret_cast<uint32_t *>(lds)[a.c_element * 4 + a.c_word] ^=
                    1u << (a.c_bit & 31);
            else if (a.c_kind == kLdsAlias && other >= 0 && other < (long long)elems)
                lds[a.c_element] = lds[other];
        }
        __syncthreads();
    }
}

// The four march steps of one pattern at one access width (ldsmarch::kB128,
// kB64, kB32).  In step s thread t handles the accesses
// lane_residue(s, t) + 256 k, from the top in the descending step; a step
// writes the complement of what it EXPECTED.
template <int PATH>
__device__ inline void lds_march(u32x4 *lds, const LdsSweepParams &a, int rep,
                                 int pattern, LdsBlockRecord *rec) {
    constexpr uint32_t W = ldsmarch::access_bytes(PATH);
    const uint32_t n = a.lds_bytes / W, elems = a.lds_bytes / 16;
    const unsigned long long base = (unsigned long long)blockIdx.x * elems;
    for (int step = 0; step < hbmmarch::kSteps; ++step) {
        const uint32_t r = ldsmarch::lane_residue(step, threadIdx.x);
        const uint32_t count = n > r ? (n - r + ldsmarch::kThreads - 1) / ldsmarch::kThreads : 0;
        const bool reads = hbmmarch::step_reads(step), writes = hbmmarch::step_writes(step);
        for (uint32_t k = 0; k < count; ++k) {
            const uint32_t acc =
                r + ldsmarch::kThreads * (hbmmarch::step_descends(step) ? count - 1 - k : k);
            const uint32_t e = acc * W / 16;
            const hbmmarch::Element p = hbmmarch::pattern(pattern, a.seed, base + e);
            const hbmmarch::Element v = hbmmarch::expected_of(p, step);
            const hbmmarch::Element x = hbmmarch::to_write_of(p, step);
            if constexpr (PATH == ldsmarch::kB128) {
                if (reads) {
                    const u32x4 got = lds[acc];
                    const u32x4 want = {v.w[0], v.w[1], v.w[2], v.w[3]};
                    if ((got.x ^ want.x) | (got.y ^ want.y) | (got.z ^ want.z) |
                        (got.w ^ want.w))
                        lds_report(rec, PATH, pattern, step, e, got, want, 0);
                }
                if (writes) lds[acc] = u32x4{x.w[0], x.w[1], x.w[2], x.w[3]};
            } else if constexpr (PATH == ldsmarch::kB64) {
                u32x2 *l2 = reinterpret_cast<u32x2 *>(lds);
                const bool hi = acc & 1;
                if (reads) {
                    const u32x2 got = l2[acc];
                    const u32x2 want = {hi ? v.w[2] : v.w[0], hi ? v.w[3] : v.w[1]};
                    if ((got.x ^ want.x) | (got.y ^ want.y)) {
                        const u32x4 g = hi ? u32x4{0, 0, got.x, got.y} : u32x4{got.x, got.y, 0, 0};
                        const u32x4 w = hi ? u32x4{0, 0, want.x, want.y} : u32x4{want.x, want.y, 0, 0};
                        lds_report(rec, PATH, pattern, step, e, g, w, 0);
                    }
                }
                if (writes) l2[acc] = u32x2{hi ? x.w[2] : x.w[0], hi ? x.w[3] : x.w[1]};
            } else {
                static_assert(PATH == ldsmarch::kB32, "three widths");
                uint32_t *l1 = reinterpret_cast<uint32_t *>(lds);
                const uint32_t word = acc & 3;
                if (reads) {
                    const uint32_t got = l1[acc], want = ldsmarch::word_of(v, word);
                    if (got != want) {
                        const u32x4 g = {word == 0 ? got : 0, word == 1 ? got : 0,
                                         word == 2 ? got : 0, word == 3 ? got : 0};
                        const u32x4 w = {word == 0 ? want : 0, word == 1 ? want : 0,
                                         word == 2 ? want : 0, word == 3 ? want : 0};
                        lds_report(rec, PATH, pattern, step, e, g, w, 0);
                    }
                }
                if (writes) l1[acc] = ldsmarch::word_of(x, word);
            }
        }
        __syncthreads();
        lds_corrupt(lds, a, rep, PATH, pattern, step);
    }
}

// Every element of the block's LDS := `poison` or pattern p, 16-byte stores,
// thread t the elements t + 256 k (step 0 of dma and of tr16).
__device__ inline void lds_fill(u32x4 *lds, const LdsSweepParams &a, int path,
                                int pattern) {
    const uint32_t elems = a.lds_bytes / 16;
    for (uint32_t e = threadIdx.x; e < elems; e += ldsmarch::kThreads) {
        const hbmmarch::Element x = ldsmarch::to_write_of(
            path, hbmmarch::pattern(pattern, a.seed,
                                    ldsmarch::pattern_index(path, blockIdx.x, elems, e)),
            0);
        lds[e] = u32x4{x.w[0], x.w[1], x.w[2], x.w[3]};
    }
    __syncthreads();
}

// dma: poison, fill every whole KiB from the global image with LDS-DMA
// (wave w's instruction k: KiB 4k + w, a wave-uniform LDS base to which the
// hardware adds lane * 16), read-verify with 16-byte loads by the waves two
// further on.  A byte the fill did not reach still holds the poison and is
// a counted mismatch.
__device__ inline void lds_dma(u32x4 *lds, const LdsSweepParams &a, int rep,
                               LdsBlockRecord *rec) {
#if defined(__gfx950__)
    constexpr int P = hbmmarch::kRandom;
    lds_fill(lds, a, ldsmarch::kDma, P);
    lds_corrupt(lds, a, rep, ldsmarch::kDma, P, 0);

    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t instructions = ldsmarch::dma_instructions(a.lds_bytes, wave);
    for (uint32_t k = 0; k < instructions; ++k) {
        const uint32_t kib = __builtin_amdgcn_readfirstlane(ldsmarch::dma_kib(wave, k));
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void *)(a.image + 64 * kib + lane),
            (__attribute__((address_space(3))) void *)(reinterpret_cast<char *>(lds) +
                                                       ldsmarch::kDmaBytes * kib),
            16, 0, 0);
    }
    __syncthreads();  // waits for vmcnt(0) first: the fill has landed
    lds_corrupt(lds, a, rep, ldsmarch::kDma, P, 1);

    const uint32_t n = ldsmarch::accesses(ldsmarch::kDma, a.lds_bytes);
    for (uint32_t e = ldsmarch::lane_residue(2, threadIdx.x); e < n; e += ldsmarch::kThreads) {
        const hbmmarch::Element v = hbmmarch::pattern(P, a.seed, e);
        const u32x4 got = lds[e];
        const u32x4 want = {v.w[0], v.w[1], v.w[2], v.w[3]};
        if ((got.x ^ want.x) | (got.y ^ want.y) | (got.z ^ want.z) | (got.w ^ want.w))
            lds_report(rec, ldsmarch::kDma, P, 2, e, got, want, 0);
    }
    __syncthreads();
#else
    (void)lds;
    (void)a;
    (void)rep;
    (void)rec;
#endif
}

// tr16: write the address pattern, then ds_read_b64_tr_b16 over every whole
// 2048 bytes: thread t of round k gives the address 2048 k + 8 t, and its
// four 16-bit results must come from ldsmarch::tr16_source(t, 0..3).  The
// trip count is uniform and every address in bounds, so EXEC is all ones at
// the read; the only lane-dependent branch is the report after it.
__device__ inline void lds_tr16(u32x4 *lds, const LdsSweepParams &a, int rep,
                                LdsBlockRecord *rec) {
#if defined(__gfx950__)
    constexpr int P = hbmmarch::kAddress;
    lds_fill(lds, a, ldsmarch::kTr16, P);
    lds_corrupt(lds, a, rep, ldsmarch::kTr16, P, 0);

    const uint32_t elems = a.lds_bytes / 16, t = threadIdx.x;
    const unsigned long long base = (unsigned long long)blockIdx.x * elems;
    const uint32_t rounds = ldsmarch::tr16_rounds(a.lds_bytes);
    // the same for q = 0..3: 32 q is a multiple of 16
    const uint32_t byte = ldsmarch::tr16_source(t, 0) % 16, shift = 8 * (byte % 4);
    for (uint32_t k = 0; k < rounds; ++k) {
        const i16x4 got = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) i16x4 *)(reinterpret_cast<char *>(lds) +
                                                        ldsmarch::tr16_address(t, k)));
        const uint32_t first_e = (ldsmarch::kTr16Bytes * k + ldsmarch::tr16_source(t, 0)) / 16;
        // element q's source: two elements on per q (32 bytes)
        const uint32_t g0 = (uint16_t)got.x, g1 = (uint16_t)got.y,
                       g2 = (uint16_t)got.z, g3 = (uint16_t)got.w;
        const uint32_t w0 = ldsmarch::half_of(hbmmarch::pattern(P, a.seed, base + first_e), byte),
                       w1 = ldsmarch::half_of(hbmmarch::pattern(P, a.seed, base + first_e + 2), byte),
                       w2 = ldsmarch::half_of(hbmmarch::pattern(P, a.seed, base + first_e + 4), byte),
                       w3 = ldsmarch::half_of(hbmmarch::pattern(P, a.seed, base + first_e + 6), byte);
        const uint32_t d0 = g0 ^ w0, d1 = g1 ^ w1, d2 = g2 ^ w2, d3 = g3 ^ w3;
        if (d0 | d1 | d2 | d3) {
            const uint32_t q = d0 ? 0 : d1 ? 1 : d2 ? 2 : 3;
            const uint32_t g = (d0 ? g0 : d1 ? g1 : d2 ? g2 : g3) << shift;
            const uint32_t w = (d0 ? w0 : d1 ? w1 : d2 ? w2 : w3) << shift;
            const uint32_t word = byte / 4;
            const u32x4 gv = {word == 0 ? g : 0, word == 1 ? g : 0,
                              word == 2 ? g : 0, word == 3 ? g : 0};
            const u32x4 wv = {word == 0 ? w : 0, word == 1 ? w : 0,
                              word == 2 ? w : 0, word == 3 ? w : 0};
            lds_report(rec, ldsmarch::kTr16, P, 1, first_e + 2 * q, gv, wv,
                       (d0 | d1 | d2 | d3) << shift, byte % 4 / 2);
        }
    }
    __syncthreads();
#else
    (void)lds;
    (void)a;
    (void)rep;
    (void)rec;
#endif
}

template <int PATH>
__device__ inline void lds_march_patterns(u32x4 *lds, const LdsSweepParams &a,
                                          int rep, LdsBlockRecord *rec) {
    for (int p = 0; p < hbmmarch::kPatterns; ++p)
        if (a.patterns[PATH] >> p & 1) lds_march<PATH>(lds, a, rep, p, rec);
}

// One 4-wave block with a.lds_bytes of dynamic LDS: at the card's
// sharedMemPerBlock that is a CU's whole LDS, so no two such blocks share a
// CU.  Each wave records where it runs; the block then runs a.reps rounds
// of the selected paths and patterns (lds_march.h) over its LDS and reports
// into its own record.  Nothing depends on where a block lands and no block
// waits for another; the host works out the coverage from the records.
// Every LDS address is below a.lds_bytes for every multiple of 16.
__global__ void __launch_bounds__(256)
lds_sweep_kernel(LdsSweepParams a, LdsBlockRecord *records) {
    extern __shared__ u32x4 lds_sweep_mem[];
    u32x4 *lds = lds_sweep_mem;
    LdsBlockRecord *rec = &records[blockIdx.x];
    if ((threadIdx.x & 63) == 0) {
        rec->hw_id[threadIdx.x >> 6] = __builtin_amdgcn_s_getreg(4 | 31 << 11);
        rec->xcc_id[threadIdx.x >> 6] = __builtin_amdgcn_s_getreg(20 | 3 << 11);
    }
    for (int rep = 0; rep < a.reps; ++rep) {
        lds_march_patterns<ldsmarch::kB128>(lds, a, rep, rec);
        lds_march_patterns<ldsmarch::kB64>(lds, a, rep, rec);
        lds_march_patterns<ldsmarch::kB32>(lds, a, rep, rec);
        if (a.patterns[ldsmarch::kDma]) lds_dma(lds, a, rep, rec);
        if (a.patterns[ldsmarch::kTr16]) lds_tr16(lds, a, rep, rec);
    }
}

}  // namespace

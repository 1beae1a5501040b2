// gfx950 device code of the deep health probe: the single definition of
// every kernel that health_probe.hip ships and that the mfma_bench /
// hbm_bench sweeps measure.  Device code only (no host policy).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

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
template <int NACC, bool ZERO = false>
__global__ void __launch_bounds__(512, 2)
mfma_peak_kernel(float *out, int iters) {
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
    float s = 0;
    for (int k = 0; k < NACC; ++k)
        for (int r = 0; r < 16; ++r) s += acc[k][r];
    if (s == -1.0f) out[blockIdx.x] = s;  // never true: defeats DCE only
#else
    (void)out;
    (void)iters;
#endif
}

// ---------------- LDS probe ----------------

__global__ void lds_probe_kernel(uint32_t *err_count, int lds_words) {
    extern __shared__ uint32_t lds[];
    int tid = threadIdx.x;
    int nthreads = blockDim.x;
    for (int i = tid; i < lds_words; i += nthreads)
        lds[i] = (uint32_t)i * 2654435761u + blockIdx.x;
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

// buf[i] = (v, v+0.25, v+0.5, v+0.75) with v = float(i & 0xFFFF): exact in
// fp32, so the host can check a copy bit for bit.
__global__ void fill_pattern_kernel(float4 *buf, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        float v = (float)(i & 0xFFFF);
        buf[i] = make_float4(v, v + 0.25f, v + 0.5f, v + 0.75f);
    }
}

}  // namespace

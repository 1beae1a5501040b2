// HBM streaming-copy variant bench (standalone binary, gfx950).
//
// Finds the fastest copy formulation for the health probe's bandwidth
// check: plain float4 grid-stride vs unrolled vs nontemporal hints.
// Guide: MI355X_MICROARCH.md §HBM (6.29 TB/s measured float4 copy ceiling).
//
// The winner, the nontemporal one-shot, is the probe's hbm_copy_kernel and is
// measured from probe_kernels.h; the variants it beat stay here.
//
// Build: python -m k8s_device_plugin_amd.native.build --sweeps  (make sweeps)
// Run:   ./hbm_bench [bytes]

#include <cstdio>
#include <cstdlib>
#include <exception>

#include "hip_util.h"
#include "probe_kernels.h"

__global__ void copy_plain(const float4 *__restrict__ src,
                           float4 *__restrict__ dst, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) dst[i] = src[i];
}

__global__ void copy_unroll4(const float4 *__restrict__ src,
                             float4 *__restrict__ dst, size_t n) {
    size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    // 4 independent loads in flight before the stores
    for (; i + 3 * stride < n; i += 4 * stride) {
        float4 a = src[i];
        float4 b = src[i + stride];
        float4 c = src[i + 2 * stride];
        float4 d = src[i + 3 * stride];
        dst[i] = a;
        dst[i + stride] = b;
        dst[i + 2 * stride] = c;
        dst[i + 3 * stride] = d;
    }
    for (; i < n; i += stride) dst[i] = src[i];
}

__global__ void copy_nt(const float4 *__restrict__ src4,
                        float4 *__restrict__ dst4, size_t n) {
    const f32x4 *__restrict__ src = reinterpret_cast<const f32x4 *>(src4);
    f32x4 *__restrict__ dst = reinterpret_cast<f32x4 *>(dst4);
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride)
        __builtin_nontemporal_store(__builtin_nontemporal_load(&src[i]), &dst[i]);
}

__global__ void copy_nt_unroll4(const float4 *__restrict__ src4,
                                float4 *__restrict__ dst4, size_t n) {
    const f32x4 *__restrict__ src = reinterpret_cast<const f32x4 *>(src4);
    f32x4 *__restrict__ dst = reinterpret_cast<f32x4 *>(dst4);
    size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < n; i += 4 * stride) {
        f32x4 a = __builtin_nontemporal_load(&src[i]);
        f32x4 b = __builtin_nontemporal_load(&src[i + stride]);
        f32x4 c = __builtin_nontemporal_load(&src[i + 2 * stride]);
        f32x4 d = __builtin_nontemporal_load(&src[i + 3 * stride]);
        __builtin_nontemporal_store(a, &dst[i]);
        __builtin_nontemporal_store(b, &dst[i + stride]);
        __builtin_nontemporal_store(c, &dst[i + 2 * stride]);
        __builtin_nontemporal_store(d, &dst[i + 3 * stride]);
    }
    for (; i < n; i += stride)
        __builtin_nontemporal_store(__builtin_nontemporal_load(&src[i]), &dst[i]);
}

template <typename K>
double bench(K kernel, const float4 *src, float4 *dst, size_t n, int blocks,
             int threads, int iters) {
    auto launch = [&] {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, 0, src, dst, n);
    };
    float ms = timed_ms(launch, [&] {
        for (int i = 0; i < iters; ++i) launch();
    });
    return (2.0 * n * sizeof(float4) * iters) / (ms * 1e6);  // GB/s
}

static void sweep(size_t bytes) {
    size_t n = bytes / sizeof(float4);
    if (n == 0) throw std::invalid_argument("bytes must be at least 16 (one float4)");
    DeviceBuffer<float4> src_buf(n), dst_buf(n);
    float4 *src = src_buf.get(), *dst = dst_buf.get();
    hipLaunchKernelGGL(fill_pattern_kernel, dim3(8192), dim3(256), 0, 0, src, n);
    HIP_CHECK(hipDeviceSynchronize());

    const int iters = 10;
    struct { const char *name; double gbps; } best{"", 0};
    for (int blocks : {8192, 16384, 32768, 65536, 131072}) {
        double p = bench(copy_plain, src, dst, n, blocks, 256, iters);
        double u = bench(copy_unroll4, src, dst, n, blocks, 256, iters);
        double t = bench(copy_nt, src, dst, n, blocks, 256, iters);
        double tu = bench(copy_nt_unroll4, src, dst, n, blocks, 256, iters);
        printf("blocks=%5d plain=%7.0f unroll4=%7.0f nt=%7.0f nt_unroll4=%7.0f GB/s\n",
               blocks, p, u, t, tu);
        if (p > best.gbps) best = {"plain", p};
        if (u > best.gbps) best = {"unroll4", u};
        if (t > best.gbps) best = {"nt", t};
        if (tu > best.gbps) best = {"nt_unroll4", tu};
    }
    {
        // the probe's kernel on the probe's grid, rounded up: at an n that is
        // no multiple of 1024 the last threads take the tail path, and the
        // GB/s counts only elements that were copied.  dst is poisoned first
        // and then compared with the pattern, all of it.
        int blocks = (int)hbm_copy_blocks(n, 256);
        HIP_CHECK(hipMemset(dst, hbmpattern::kPoisonByte, n * sizeof(float4)));
        double o = bench(hbm_copy_kernel, src, dst, n, blocks, 256, iters);
        printf("oneshot blocks=%d nt_oneshot=%7.0f GB/s\n", blocks, o);
        if (o > best.gbps) best = {"nt_oneshot", o};

        DeviceBuffer<unsigned long long> verdict(2);
        unsigned long long h[2] = {0, ~0ull};
        HIP_CHECK(hipMemcpy(verdict.get(), h, sizeof(h), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(verify_pattern_kernel, dim3(blocks), dim3(256), 0, 0,
                           dst, n, verdict.get(), verdict.get() + 1);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(h, verdict.get(), sizeof(h), hipMemcpyDeviceToHost));
        printf("oneshot copied %zu elements, %llu differ from the pattern\n", n, h[0]);
        if (h[0])
            throw std::runtime_error("oneshot copy is wrong, first at element " +
                                     std::to_string(h[1]));
    }
    printf("BEST %s %.0f GB/s\n", best.name, best.gbps);
}

int main(int argc, char **argv) {
    try {
        sweep(argc > 1 ? strtoull(argv[1], nullptr, 0) : (size_t)4 << 30);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}

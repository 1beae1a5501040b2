// HBM streaming-copy variant bench (standalone binary, gfx950).
//
// Finds the fastest copy formulation for the health probe's bandwidth
// check: plain float4 grid-stride vs unrolled vs nontemporal hints.
// Guide: MI355X_MICROARCH.md §HBM (6.29 TB/s measured float4 copy ceiling).
//
// The winner, the nontemporal one-shot, is the probe's hbm_copy_kernel and is
// measured from probe_kernels.h; the variants it beat stay here.
//
// After the copy rows come the HBM scrub's march kernels (march_kernel,
// probe_kernels.h) at the same n in the same run: write, read-verify-write
// and read-verify, per pattern, with nt and plain accesses and three block
// sizes, each as min / median / max over single launches next to the same
// figures for the copy, and last the copy, march_rw into a second buffer
// and march_rw in place alternated launch by launch
// (profiles/hbm_scrub_mi355x.md).
//
// Build: python -m k8s_device_plugin_amd.native.build --sweeps  (make sweeps)
// Run:   ./hbm_bench [bytes]

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <vector>

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

// min / median / max of the GB/s of single launches
struct Spread {
    double lo, mid, hi;
};

template <typename Launch>
Spread spread_gbps(Launch &&launch, double bytes_per_launch, int repeats) {
    std::vector<double> gbps;
    launch();  // warm
    for (int r = 0; r < repeats; ++r) {
        float ms = timed_ms([] {}, launch);
        gbps.push_back(bytes_per_launch / (ms * 1e6));
    }
    std::sort(gbps.begin(), gbps.end());
    return {gbps.front(), gbps[gbps.size() / 2], gbps.back()};
}

// The scrub's march kernels, in place on buf, next to the copy: march_rw
// moves what a copy moves (n read, n written).  The steps run in an order
// that keeps every expectation true (0; 1, 2, 1, 2, ...; 3), so no launch
// takes the cold path; the report is checked at the end.
template <bool NT>
static void march_rows(u32x4 *buf, size_t n, int pattern, int threads,
                       int repeats) {
    DeviceBuffer<MarchReport> rep(1);
    DeviceBuffer<MarchRecord> rec(64);
    DeviceBuffer<uint32_t> ranges((n >> kMarchRangeShift) + 1);
    MarchReport h{};
    h.first_bad = ~0ull;
    HIP_CHECK(hipMemcpy(rep.get(), &h, sizeof(h), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemset(ranges.get(), 0,
                        ((n >> kMarchRangeShift) + 1) * sizeof(uint32_t)));
    const dim3 grid((unsigned)hbm_copy_blocks(n, threads)), block(threads);
    MarchParams a{};
    a.pattern = pattern;
    a.seed = 0x5EED;
    a.base = 0;
    a.n = n;
    a.max_records = 64;
    const double bytes = (double)n * 16;

    a.step = 0;
    Spread w = spread_gbps([&] {
        hipLaunchKernelGGL((march_kernel<kMarchWrite, NT>), grid, block, 0, 0,
                           buf, a, rep.get(), rec.get(), ranges.get());
    }, bytes, repeats);
    // the warm launch plus an even count of repeats ends on step 2's state
    int flip = 0;
    Spread rw = spread_gbps([&] {
        a.step = 1 + (flip++ & 1);
        hipLaunchKernelGGL((march_kernel<kMarchRW, NT>), grid, block, 0, 0, buf,
                           a, rep.get(), rec.get(), ranges.get());
    }, 2 * bytes, repeats | 1);
    a.step = 3;
    Spread rd = spread_gbps([&] {
        hipLaunchKernelGGL((march_kernel<kMarchRead, NT>), grid, block, 0, 0,
                           buf, a, rep.get(), rec.get(), ranges.get());
    }, bytes, repeats);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpy(&h, rep.get(), sizeof(h), hipMemcpyDeviceToHost));
    printf("march pattern=%-7s %s threads=%4d  march_write=%5.0f/%5.0f/%5.0f  "
           "march_rw=%5.0f/%5.0f/%5.0f  march_read=%5.0f/%5.0f/%5.0f GB/s "
           "(min/median/max of %d)\n",
           hbmmarch::kPatternNames[pattern], NT ? "nt   " : "plain", threads,
           w.lo, w.mid, w.hi, rw.lo, rw.mid, rw.hi, rd.lo, rd.mid, rd.hi,
           repeats);
    if (h.mismatches)
        throw std::runtime_error("march found " + std::to_string(h.mismatches) +
                                 " mismatches, first at element " +
                                 std::to_string(h.first_bad));
}

// march_rw's loads, compares and stores with the stores going to a SECOND
// buffer: what march_rw would do if it were not in place.  Separates the
// cost of reading and writing the same DRAM page from the cost of the
// compare.  from holds step 1's expectation (the pattern); to gets ~p.
__global__ void march_rw_two_buffers(const u32x4 *__restrict__ from,
                                     u32x4 *__restrict__ to, MarchParams a,
                                     unsigned long long *bad) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    auto finish = [&](size_t e, u32x4 got) {
        const hbmmarch::Element p = hbmmarch::pattern(a.pattern, a.seed, a.base + e);
        const hbmmarch::Element want = hbmmarch::expected_of(p, a.step);
        const hbmmarch::Element v = hbmmarch::to_write_of(p, a.step);
        if ((got.x ^ want.w[0]) | (got.y ^ want.w[1]) | (got.z ^ want.w[2]) |
            (got.w ^ want.w[3]))
            atomicAdd(bad, 1ull);
        const u32x4 x = {v.w[0], v.w[1], v.w[2], v.w[3]};
        __builtin_nontemporal_store(x, &to[e]);
    };
    if (t + 3 * stride < a.n) {
        const u32x4 g0 = __builtin_nontemporal_load(&from[t]),
                    g1 = __builtin_nontemporal_load(&from[t + stride]),
                    g2 = __builtin_nontemporal_load(&from[t + 2 * stride]),
                    g3 = __builtin_nontemporal_load(&from[t + 3 * stride]);
        finish(t, g0);
        finish(t + stride, g1);
        finish(t + 2 * stride, g2);
        finish(t + 3 * stride, g3);
    } else {
        for (size_t e = t; e < a.n; e += stride)
            finish(e, __builtin_nontemporal_load(&from[e]));
    }
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

        // the same copy launch by launch: its min-to-max spread is the
        // margin that the march rows below are judged against
        const int repeats = 10;
        Spread c = spread_gbps([&] {
            hipLaunchKernelGGL(hbm_copy_kernel, dim3(blocks), dim3(256), 0, 0,
                               src, dst, n);
        }, 2.0 * n * sizeof(float4), repeats);
        printf("oneshot single launches nt_oneshot=%5.0f/%5.0f/%5.0f GB/s "
               "(min/median/max of %d)\n", c.lo, c.mid, c.hi, repeats);

        // the scrub's kernels, same n, in place on dst: the shipped form
        // (nt, 256 threads) per pattern, then store flavour and block size
        u32x4 *buf = reinterpret_cast<u32x4 *>(dst);
        for (int p = 0; p < hbmmarch::kPatterns; ++p)
            march_rows<true>(buf, n, p, 256, repeats);
        for (int threads : {512, 1024})
            march_rows<true>(buf, n, hbmmarch::kAddress, threads, repeats);
        for (int threads : {256, 512, 1024})
            march_rows<false>(buf, n, hbmmarch::kAddress, threads, repeats);

        // the last row left the address pattern in dst: march_rw's work out
        // of place, dst -> src (the copy is checked, src is free)
        DeviceBuffer<unsigned long long> bad(1);
        HIP_CHECK(hipMemset(bad.get(), 0, sizeof(unsigned long long)));
        MarchParams a{};
        a.pattern = hbmmarch::kAddress;
        a.step = 1;
        a.seed = 0x5EED;
        a.n = n;
        Spread two = spread_gbps([&] {
            hipLaunchKernelGGL(march_rw_two_buffers, dim3(blocks), dim3(256), 0,
                               0, buf, reinterpret_cast<u32x4 *>(src_buf.get()),
                               a, bad.get());
        }, 2.0 * n * sizeof(float4), repeats);
        unsigned long long h_bad = 0;
        HIP_CHECK(hipMemcpy(&h_bad, bad.get(), sizeof(h_bad), hipMemcpyDeviceToHost));
        printf("march pattern=address nt    threads= 256  "
               "march_rw_two_buffers=%5.0f/%5.0f/%5.0f GB/s "
               "(min/median/max of %d), %llu mismatches\n",
               two.lo, two.mid, two.hi, repeats, h_bad);
        if (h_bad) throw std::runtime_error("march_rw_two_buffers read a wrong element");

        // The rows above ran one after the other, and the card's rate drifts
        // over a run.  So the three two-way kernels once more, ALTERNATED
        // launch by launch: copy dst -> src, march_rw's work dst -> src, and
        // march_rw in place on dst (last, because it moves dst on to the next
        // step's expectation).  dst holds the address pattern here.
        DeviceBuffer<MarchReport> rep(1);
        DeviceBuffer<MarchRecord> rec(64);
        DeviceBuffer<uint32_t> ranges((n >> kMarchRangeShift) + 1);
        MarchReport h_rep{};
        h_rep.first_bad = ~0ull;
        HIP_CHECK(hipMemcpy(rep.get(), &h_rep, sizeof(h_rep), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(ranges.get(), 0,
                            ((n >> kMarchRangeShift) + 1) * sizeof(uint32_t)));
        a.max_records = 64;
        const int rounds = 20;  // even: dst ends on the pattern again
        const double two_way = 2.0 * n * sizeof(float4);
        std::vector<double> g_copy, g_two, g_rw;
        u32x4 *other = reinterpret_cast<u32x4 *>(src_buf.get());
        for (int r = 0; r < rounds; ++r) {
            a.step = 1 + (r & 1);
            g_copy.push_back(two_way / (1e6 * timed_ms([] {}, [&] {
                hipLaunchKernelGGL(hbm_copy_kernel, dim3(blocks), dim3(256), 0,
                                   0, dst, src, n);
            })));
            g_two.push_back(two_way / (1e6 * timed_ms([] {}, [&] {
                hipLaunchKernelGGL(march_rw_two_buffers, dim3(blocks), dim3(256),
                                   0, 0, buf, other, a, bad.get());
            })));
            g_rw.push_back(two_way / (1e6 * timed_ms([] {}, [&] {
                hipLaunchKernelGGL((march_kernel<kMarchRW, true>), dim3(blocks),
                                   dim3(256), 0, 0, buf, a, rep.get(), rec.get(),
                                   ranges.get());
            })));
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(&h_rep, rep.get(), sizeof(h_rep), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(&h_bad, bad.get(), sizeof(h_bad), hipMemcpyDeviceToHost));
        auto show = [&](const char *name, std::vector<double> &g) {
            std::sort(g.begin(), g.end());
            printf("alternated %-22s %5.0f/%5.0f/%5.0f GB/s (min/median/max of %d)\n",
                   name, g.front(), g[g.size() / 2], g.back(), rounds);
        };
        show("nt_oneshot copy", g_copy);
        show("march_rw_two_buffers", g_two);
        show("march_rw in place", g_rw);
        if (h_rep.mismatches || h_bad)
            throw std::runtime_error("the alternated march read a wrong element");
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

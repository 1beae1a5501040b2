// bf16 MFMA peak-throughput variant sweep (standalone binary, gfx950).
//
// Finds the fastest formulation for the health probe's matrix-pipe check.
// v_mfma_f32_32x32x16_bf16 issues back-to-back at 32 cyc/SIMD (guide:
// MI355X_MICROARCH.md §Per-instruction constants); the sweep varies
// accumulator count (dependency cover) and wave geometry over the kernel
// the probe ships (probe_kernels.h, same launch bounds).
//
// Build: python -m k8s_device_plugin_amd.native.build --sweeps  (make sweeps)

#include <cstdio>
#include <exception>

#include "hip_util.h"
#include "probe_kernels.h"

template <int NACC, bool ZERO = false>
double bench(int blocks, int threads, int iters, float *d) {
    auto launch = [&](int n) {
        hipLaunchKernelGGL((mfma_peak_kernel<NACC, ZERO>), dim3(blocks),
                           dim3(threads), 0, 0, d, n, 0);
    };
    float ms = timed_ms([&] { launch(64); }, [&] { launch(iters); });
    double waves = (double)blocks * threads / 64;
    double flops = waves * iters * NACC * 2.0 * 32 * 32 * 16;
    return flops / (ms * 1e9);  // TF/s
}

static void sweep() {
    hipDeviceProp_t props;
    HIP_CHECK(hipGetDeviceProperties(&props, 0));
    int cu = props.multiProcessorCount;
    DeviceBuffer<float> buf(65536);
    float *d = buf.get();
    const int iters = 8192;
    struct { char name[64]; double tf; } best{{0}, 0};
    struct Shape { int blocks, threads; const char *desc; };
    Shape shapes[] = {
        {cu, 512, "512x1/CU"},
        {cu * 2, 512, "512x2/CU"},
        {cu * 2, 256, "256x2/CU"},
        {cu * 4, 256, "256x4/CU"},
    };
    for (auto &sh : shapes) {
        double t2 = bench<2>(sh.blocks, sh.threads, iters, d);
        double t4 = bench<4>(sh.blocks, sh.threads, iters, d);
        double t8 = bench<8>(sh.blocks, sh.threads, iters, d);
        printf("%-10s acc2=%6.0f acc4=%6.0f acc8=%6.0f TF/s\n", sh.desc, t2, t4, t8);
        if (t2 > best.tf) { best.tf = t2; snprintf(best.name, 64, "%s acc2", sh.desc); }
        if (t4 > best.tf) { best.tf = t4; snprintf(best.name, 64, "%s acc4", sh.desc); }
        if (t8 > best.tf) { best.tf = t8; snprintf(best.name, 64, "%s acc8", sh.desc); }
    }
    printf("BEST %s %.0f TF/s\n", best.name, best.tf);
    // DVFS demonstration: zero operands draw less power -> higher clock
    double zr = bench<2, true>(cu * 2, 512, iters, d);
    printf("DVFS check: 512x2/CU acc2 zero-operands = %.0f TF/s\n", zr);
}

int main() {
    try {
        sweep();
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}

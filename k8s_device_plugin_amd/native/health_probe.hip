// gfx950 deep health probe (HIP/CDNA4).
//
// MI355X-native upgrade over the reference's liveness check, which only
// opens the device node (reference: internal/pkg/amdgpu/amdgpu.go:390-399).
// This probe actually executes CDNA4 code on the GPU and verifies:
//   1. wavefront size is 64 and all lanes participate (ballot);
//   2. the bf16 MFMA matrix pipe computes correct sums
//      (v_mfma_f32_16x16x32_bf16 invariant checks, exact in bf16/f32);
//   3. LDS write/read round-trips a full 128 KiB per CU;
//   4. HBM sustains a float4 streaming copy at a reportable GB/s
//      (grid sized >>256 workgroups to cover all 8 XCDs).
//
// Used by the plugin's optional deep health check, __graft_entry__.smoke(),
// and the gpu-marked tests.  The kernels live in probe_kernels.h (shared
// with the mfma_bench / hbm_bench sweeps), the HIP host scaffolding in
// hip_util.h; this file is host policy and the pybind module.  Build:
// hipcc --offload-arch=gfx950, see native/build.py.

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "hip_util.h"
#include "probe_kernels.h"

namespace py = pybind11;

namespace {

struct WaveResult {
    int wavefront_size;
    bool ok;
};

WaveResult check_wave() {
    DeviceBuffer<unsigned long long> d(2);
    hipLaunchKernelGGL(wave_probe_kernel, dim3(1), dim3(64), 0, 0, d.get());
    HIP_CHECK(hipGetLastError());
    unsigned long long h[2];
    HIP_CHECK(hipMemcpy(h, d.get(), sizeof(h), hipMemcpyDeviceToHost));
    return {(int)h[1], h[0] == ~0ull && h[1] == 64};
}

// One wave of mfma_probe_kernel; returns its [3][256] per-lane fragments.
std::vector<float> run_mfma_probe() {
    std::vector<float> h(3 * 256);
    DeviceBuffer<float> d(h.size());
    HIP_CHECK(hipMemset(d.get(), 0, h.size() * sizeof(float)));
    hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, 0, d.get());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpy(h.data(), d.get(), h.size() * sizeof(float),
                        hipMemcpyDeviceToHost));
    return h;
}

struct MfmaResult {
    bool const_ok, sum_ok;
};

MfmaResult check_mfma() {
    std::vector<float> h = run_mfma_probe();
    bool pass0 = true;
    for (int i = 0; i < 256; ++i)
        if (h[i] != 16.0f) pass0 = false;
    double sum_a = 0;
    for (int lane = 0; lane < 64; ++lane)
        for (int r = 0; r < 8; ++r)
            sum_a += ((lane * 8 + r) % 7) - 3;
    double sum_d = 0;
    for (int i = 0; i < 256; ++i) sum_d += h[256 + i];
    return {pass0, sum_d == 16.0 * sum_a};
}

// Matrix pipes at speed on all CUs; returns TF/s.  <2> won the recorded
// sweep (profiles/r01_bench_mi355x.md), whose 8-accumulator build had no
// launch bounds, was capped at 128 VGPRs and spilled (152 TF/s).  Under
// the kernel's launch bounds the compiler reports no spill for any width:
// 40 / 72 / 136 VGPRs, 0 scratch, occupancy 8 / 7 / 3 waves per SIMD for
// 2 / 4 / 8 accumulators; run the sweep again before changing the choice.
double measure_mfma_tflops(int cu_count) {
    DeviceBuffer<float> d(4096);
    const int iters = 8192, blocks = cu_count * 2;
    auto launch = [&](int n) {
        hipLaunchKernelGGL(mfma_peak_kernel<2>, dim3(blocks), dim3(512), 0, 0,
                           d.get(), n);
    };
    float ms = timed_ms([&] { launch(64); }, [&] { launch(iters); });
    // FLOPs: blocks * 8 waves * iters * 2 MFMA * 2*32*32*16
    double flops = (double)blocks * 8 * iters * 2 * 2 * 32 * 32 * 16;
    return flops / (ms * 1e9);
}

struct LdsResult {
    bool ok;
    int bytes_tested;
};

// 128 KiB dynamic LDS per workgroup (160 KiB/CU on gfx950), one per CU
LdsResult check_lds(int cu_count) {
    const int lds_bytes = 128 * 1024;
    DeviceBuffer<uint32_t> d_err(1);
    HIP_CHECK(hipMemset(d_err.get(), 0, sizeof(uint32_t)));
    hipLaunchKernelGGL(lds_probe_kernel, dim3(cu_count), dim3(256), lds_bytes,
                       0, d_err.get(), lds_bytes / 4);
    HIP_CHECK(hipGetLastError());
    uint32_t h_err = 1;
    HIP_CHECK(hipMemcpy(&h_err, d_err.get(), sizeof(h_err),
                        hipMemcpyDeviceToHost));
    return {h_err == 0, lds_bytes};
}

struct HbmResult {
    double gbps;
    uint64_t bytes_tested;
    bool copy_ok;
};

// Streaming copy bandwidth (read+write) of n >= 1 float4s, then a spot
// check of the copy against the fill pattern.
HbmResult check_hbm(size_t n) {
    DeviceBuffer<float4> src(n), dst(n);
    // exact-fit grid: one thread per 4 float4s (no loop), which was the
    // fastest measured formulation; still >>256 workgroups for all 8 XCDs
    const int threads = 256, iters = 5;
    long want = (long)((n + threads * 4 - 1) / (threads * 4));
    const int blocks = (int)(want < 1024 ? 1024 : want);
    auto copy = [&] {
        hipLaunchKernelGGL(hbm_copy_kernel, dim3(blocks), dim3(threads), 0, 0,
                           src.get(), dst.get(), n);
    };
    float ms = timed_ms(
        [&] {
            hipLaunchKernelGGL(fill_pattern_kernel, dim3(blocks), dim3(threads),
                               0, 0, src.get(), n);
            copy();
        },
        [&] {
            for (int i = 0; i < iters; ++i) copy();
        });
    double gbps = (2.0 * n * sizeof(float4) * iters) / (ms * 1e6);

    // min(16, n) elements at the head, the middle and the end of dst
    const size_t m = std::min<size_t>(16, n);
    bool copy_ok = true;
    for (size_t first : {(size_t)0, std::min(n / 2, n - m), n - m}) {
        float4 sample[16];
        HIP_CHECK(hipMemcpy(sample, dst.get() + first, m * sizeof(float4),
                            hipMemcpyDeviceToHost));
        for (size_t k = 0; k < m; ++k) {
            float v = (float)((first + k) & 0xFFFF);
            const float4 &s = sample[k];
            if (s.x != v || s.y != v + 0.25f || s.z != v + 0.5f ||
                s.w != v + 0.75f)
                copy_ok = false;
        }
    }
    return {gbps, (uint64_t)(n * sizeof(float4)), copy_ok};
}

py::dict run_probe(int device, size_t hbm_bytes) {
    if (hbm_bytes < sizeof(float4))
        throw std::invalid_argument("hbm_bytes must be at least 16 (one float4)");
    HIP_CHECK(hipSetDevice(device));
    hipDeviceProp_t props;
    HIP_CHECK(hipGetDeviceProperties(&props, device));

    WaveResult wave = check_wave();
    MfmaResult mfma = check_mfma();
    double mfma_tflops = measure_mfma_tflops(props.multiProcessorCount);
    LdsResult lds = check_lds(props.multiProcessorCount);
    HbmResult hbm = check_hbm(hbm_bytes / sizeof(float4));

    py::dict result;
    result["device_name"] = std::string(props.name);
    result["gcn_arch"] = std::string(props.gcnArchName);
    result["cu_count"] = props.multiProcessorCount;
    result["vram_bytes"] = (uint64_t)props.totalGlobalMem;
    result["wavefront_size"] = wave.wavefront_size;
    result["wave_ok"] = wave.ok;
    result["mfma_ok"] = mfma.const_ok && mfma.sum_ok;
    result["mfma_const_ok"] = mfma.const_ok;
    result["mfma_sum_ok"] = mfma.sum_ok;
    result["mfma_tflops"] = mfma_tflops;
    result["lds_ok"] = lds.ok;
    result["lds_bytes_tested"] = lds.bytes_tested;
    result["hbm_gbps"] = hbm.gbps;
    result["hbm_bytes_tested"] = hbm.bytes_tested;
    result["hbm_copy_ok"] = hbm.copy_ok;
    result["healthy"] = wave.ok && mfma.const_ok && mfma.sum_ok && lds.ok &&
                        hbm.copy_ok;
    return result;
}

// Raw MFMA fragment outputs for element-wise verification against a host
// (PyTorch) reference (tests/test_gpu.py reconstructs the lane->element
// mapping).
py::dict mfma_probe_raw(int device) {
    HIP_CHECK(hipSetDevice(device));
    std::vector<float> h = run_mfma_probe();
    py::list pass[3];
    for (int p = 0; p < 3; ++p)
        for (int i = 0; i < 256; ++i) pass[p].append(h[p * 256 + i]);
    py::dict out;
    out["pass0"] = pass[0];  // expect all 16.0
    out["pass1"] = pass[1];  // D = A_pattern @ ones, per-lane fragments
    out["pass2"] = pass[2];  // D = A_pattern @ B_pattern (asymmetric both)
    return out;
}

int device_count() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return 0;
    return n;
}

// Measured GPU->GPU copy bandwidth: on an 8*MI355X hive this runs over one
// xGMI point-to-point link (~153 GB/s class); PCIe-bridged pairs land far
// lower — the hardware truth behind the allocator's hive packing
// (docs/resource-allocation.md).
py::dict p2p_bandwidth(int src, int dst, size_t bytes) {
    py::dict out;
    out["src"] = src;
    out["dst"] = dst;

    int can = 0;
    HIP_CHECK(hipDeviceCanAccessPeer(&can, dst, src));
    out["peer_access"] = (bool)can;

    HIP_CHECK(hipSetDevice(src));
    DeviceBuffer<char> src_buf(bytes);
    HIP_CHECK(hipMemset(src_buf.get(), 0x5A, bytes));
    HIP_CHECK(hipSetDevice(dst));
    if (can) {
        hipError_t e = hipDeviceEnablePeerAccess(src, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
            throw std::runtime_error(hipGetErrorString(e));
    }
    {
        DeviceBuffer<char> dst_buf(bytes);
        const int iters = 10;
        auto copy = [&] {
            HIP_CHECK(hipMemcpyPeerAsync(dst_buf.get(), dst, src_buf.get(), src,
                                         bytes, 0));
        };
        float ms = timed_ms(copy, [&] {
            for (int i = 0; i < iters; ++i) copy();
        });
        out["gbps"] = ((double)bytes * iters) / (ms * 1e6);
    }
    HIP_CHECK(hipSetDevice(src));  // src_buf is released on its own device
    return out;
}

} // namespace

// PCI bus id per HIP ordinal ("domain:bus:device.function", lowercase) —
// lets the plugin map its kfd-derived device ids onto ordinals exactly
// instead of assuming enumeration order (ROCR_VISIBLE_DEVICES can
// reorder it).
std::vector<std::string> pci_bus_ids() {
    int n = 0;
    HIP_CHECK(hipGetDeviceCount(&n));
    std::vector<std::string> out;
    out.reserve(n);
    for (int i = 0; i < n; ++i) {
        char buf[32] = {0};
        if (hipDeviceGetPCIBusId(buf, sizeof(buf), i) == hipSuccess)
            out.emplace_back(buf);
        else
            out.emplace_back("");
    }
    return out;
}

PYBIND11_MODULE(_healthprobe, m) {
    m.doc() = "gfx950 deep GPU health probe (MFMA/LDS/HBM)";
    m.def("run_probe", &run_probe, py::arg("device") = 0,
          py::arg("hbm_bytes") = (size_t)1 << 30);
    m.def("device_count", &device_count);
    m.def("pci_bus_ids", &pci_bus_ids);
    m.def("p2p_bandwidth", &p2p_bandwidth, py::arg("src") = 0,
          py::arg("dst") = 1, py::arg("bytes") = (size_t)1 << 30);
    m.def("mfma_probe_raw", &mfma_probe_raw, py::arg("device") = 0);
}

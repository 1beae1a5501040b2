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
//      (grid sized >>256 workgroups to cover all 8 XCDs), and every element
//      of the copy equals a pattern that does not repeat (hbm_pattern.h);
//   5. on request (cu_sweep), exact known-answer products of the bf16, f16,
//      fp8, i8 and MX-fp8 matrix pipes on every SIMD of every CU, with the
//      place each wave ran read from the hardware id registers; with
//      pipe_set "mx" / "wide" the same over block-scaled fp4 / fp6 with
//      live scales and over bf8, the 32x32 shapes, f64 and f32-input
//      (sweep_table_ext.h);
//   6. on request (hbm_scrub), in-place march passes over all free VRAM:
//      fused read-verify-write at streaming rate, four data patterns and
//      their complements (hbm_march.h);
//   7. on request (lds_sweep), the same march over all 160 KiB of LDS of
//      every CU, through the 128-, 64- and 32-bit loads and stores, the
//      LDS-DMA and the transposed read (lds_march.h), with the place each
//      block ran read from the hardware id registers;
//   8. on request (valu_sweep), known-answer vector, conversion, cross-lane,
//      scalar and transcendental instructions on every SIMD of every CU, in
//      the CU sweep's shape and with its host code (valu_kernels.h,
//      valu_table.h).
//
// Used by the plugin's optional deep health check, __graft_entry__.smoke(),
// and the gpu-marked tests.  The kernels live in probe_kernels.h (shared
// with the mfma_bench / hbm_bench sweeps), the HIP host scaffolding in
// hip_util.h; this file is host policy and the pybind module.  Build:
// hipcc --offload-arch=gfx950, see native/build.py.

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <initializer_list>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "hip_util.h"
#include "probe_kernels.h"
#include "valu_kernels.h"

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
// 42 / 74 / 138 VGPRs, 0 scratch, occupancy 8 / 6 / 3 waves per SIMD for
// 2 / 4 / 8 accumulators (the store argument costs 2 VGPRs, and <4> a
// seventh wave); run the sweep again before changing the choice.
// mfma_peak_check runs this same instantiation with store = 1 and the tests
// compare its accumulators with iters * (A @ B): the iters * 2 MFMAs per
// wave that the formula below counts are the ones that ran.
double measure_mfma_tflops(int cu_count) {
    DeviceBuffer<float> d(4096);
    const int iters = 8192, blocks = cu_count * 2;
    auto launch = [&](int n) {
        hipLaunchKernelGGL(mfma_peak_kernel<2>, dim3(blocks), dim3(512), 0, 0,
                           d.get(), n, 0);
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

// lds_probe_kernel on blocks workgroups of lds_bytes dynamic LDS each;
// returns the raw error count.  corrupt_block = -1: nothing corrupted.
uint32_t run_lds_probe(int blocks, int threads, int lds_bytes,
                       int corrupt_block, int corrupt_word,
                       uint32_t corrupt_mask) {
    DeviceBuffer<uint32_t> d_err(1);
    HIP_CHECK(hipMemset(d_err.get(), 0, sizeof(uint32_t)));
    hipLaunchKernelGGL(lds_probe_kernel, dim3(blocks), dim3(threads), lds_bytes,
                       0, d_err.get(), lds_bytes / 4, corrupt_block,
                       corrupt_word, corrupt_mask);
    HIP_CHECK(hipGetLastError());
    uint32_t h_err = 1;
    HIP_CHECK(hipMemcpy(&h_err, d_err.get(), sizeof(h_err),
                        hipMemcpyDeviceToHost));
    return h_err;
}

// 128 KiB dynamic LDS per workgroup (160 KiB/CU on gfx950), one per CU
LdsResult check_lds(int cu_count) {
    const int lds_bytes = 128 * 1024;
    return {run_lds_probe(cu_count, 256, lds_bytes, -1, -1, 0) == 0, lds_bytes};
}

struct PatternResult {
    unsigned long long mismatches;
    long long first_bad;  // lowest differing index, -1 when there is none
};

// verify_pattern_kernel over all n elements of buf.
PatternResult verify_pattern(const float4 *buf, size_t n) {
    DeviceBuffer<unsigned long long> d(2);
    unsigned long long h[2] = {0, ~0ull};
    HIP_CHECK(hipMemcpy(d.get(), h, sizeof(h), hipMemcpyHostToDevice));
    // the fill's grid: four elements per thread, grid-stride
    hipLaunchKernelGGL(verify_pattern_kernel, dim3((unsigned)hbm_copy_blocks(n)),
                       dim3(256), 0, 0, buf, n, d.get(), d.get() + 1);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpy(h, d.get(), sizeof(h), hipMemcpyDeviceToHost));
    return {h[0], h[0] ? (long long)h[1] : -1};
}

struct HbmResult {
    double gbps;
    uint64_t bytes_tested;
    bool copy_ok;
    PatternResult verdict;
};

// Streaming copy bandwidth (read+write) of n >= 1 float4s, then a check of
// the WHOLE copy against the fill pattern.  dst is poisoned first, so an
// element that no thread wrote cannot pass on what the allocation held.
HbmResult check_hbm(size_t n) {
    DeviceBuffer<float4> src(n), dst(n);
    HIP_CHECK(hipMemset(dst.get(), hbmpattern::kPoisonByte, n * sizeof(float4)));
    // exact-fit grid: one thread per 4 float4s (no loop), which was the
    // fastest measured formulation; still >>256 workgroups for all 8 XCDs
    const int threads = 256, iters = 5;
    const int blocks = (int)hbm_copy_blocks(n, threads);
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

    const PatternResult verdict = verify_pattern(dst.get(), n);
    return {gbps, (uint64_t)(n * sizeof(float4)), verdict.mismatches == 0,
            verdict};
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
    result["hbm_mismatches"] = hbm.verdict.mismatches;
    result["hbm_first_bad"] = hbm.verdict.first_bad;
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

// ---------------- the default checks, one at a time, for the tests ----------------
//
// Each entry validates its arguments before any HIP call (ValueError), so
// the rejections are testable without a GPU.

void require_whole_waves(int threads) {
    if (threads < 64 || threads > 1024 || threads % 64)
        throw std::invalid_argument(
            "threads must be a multiple of 64 in 64..1024");
}

constexpr long long kCopyCheckMaxN = 1ll << 32;      // 64 GiB per buffer
constexpr long long kCopyCheckMaxGuard = 1ll << 20;  // float4s per band
constexpr long long kCopyCheckMaxData = 1ll << 21;   // n for return_data

// Damage to one 16-byte element of device memory from the host, with
// hipMemcpy inside the allocation and no kernel: bit `bit` of its 32-bit
// word `word` flipped or, with alias_of, the whole element := *alias_of.
void damage_from_host(void *element, long long word, long long bit,
                      const void *alias_of) {
    if (alias_of) {
        HIP_CHECK(hipMemcpy(element, alias_of, 16, hipMemcpyDeviceToDevice));
        return;
    }
    uint32_t *at = static_cast<uint32_t *>(element) + word;
    uint32_t w = 0;
    HIP_CHECK(hipMemcpy(&w, at, sizeof(w), hipMemcpyDeviceToHost));
    w ^= 1u << bit;
    HIP_CHECK(hipMemcpy(at, &w, sizeof(w), hipMemcpyHostToDevice));
}

// Whether both guard bands of a guard + data + guard allocation still hold
// the poison.
bool guards_hold_poison(const void *alloc, size_t guard_bytes, size_t data_bytes) {
    bool ok = true;
    std::vector<unsigned char> band(guard_bytes);
    const char *low = static_cast<const char *>(alloc);
    for (const char *from : {low, low + guard_bytes + data_bytes}) {
        if (band.empty()) break;
        HIP_CHECK(hipMemcpy(band.data(), from, band.size(),
                            hipMemcpyDeviceToHost));
        for (unsigned char b : band)
            if (b != hbmpattern::kPoisonByte) ok = false;
    }
    return ok;
}

// ONE hbm_copy_kernel launch of n float4s into the middle of a poisoned
// guard + n + guard allocation (guard counts float4s), then the device
// verifier over the n elements and a host check that both guard bands still
// hold the poison.  blocks = 0 takes the production grid, hbm_copy_blocks.
// corrupt damages dst between the copy and the verifier (damage_from_host):
//   ("flip", index, component, bit)   flips one bit of one float
//   ("alias", index, distance)        element index := element index + distance
py::dict hbm_copy_check(int device, long long n, long long blocks, int threads,
                        long long guard, py::object corrupt, bool return_data) {
    if (n < 1 || n > kCopyCheckMaxN)
        throw std::invalid_argument("n must be in 1..2^32");
    require_whole_waves(threads);
    if (blocks < 0 || blocks > INT32_MAX)
        throw std::invalid_argument("blocks must be in 0..2^31-1 (0 = default)");
    if (blocks == 0) blocks = (long long)hbm_copy_blocks((size_t)n, threads);
    if (blocks > INT32_MAX)
        throw std::invalid_argument("n needs more than 2^31-1 blocks");
    if (4 * blocks * threads < n)
        throw std::invalid_argument(
            "hbm_copy_kernel needs 4 * blocks * threads >= n");
    if (guard < 0 || guard > kCopyCheckMaxGuard)
        throw std::invalid_argument("guard must be in 0..2^20 float4s");
    if (return_data && n > kCopyCheckMaxData)
        throw std::invalid_argument("return_data needs n <= 2^21");
    enum { kNone, kFlip, kAlias } kind = kNone;
    long long c_index = 0, c_component = 0, c_bit = 0, c_distance = 0;
    if (!corrupt.is_none()) {
        py::sequence seq = corrupt.cast<py::sequence>();
        const std::string what =
            py::len(seq) ? seq[0].cast<std::string>() : std::string();
        if (what == "flip" && py::len(seq) == 4) {
            kind = kFlip;
            c_index = seq[1].cast<long long>();
            c_component = seq[2].cast<long long>();
            c_bit = seq[3].cast<long long>();
            if (c_component < 0 || c_component > 3 || c_bit < 0 || c_bit > 31)
                throw std::invalid_argument(
                    "flip: component in 0..3, bit in 0..31");
        } else if (what == "alias" && py::len(seq) == 3) {
            kind = kAlias;
            c_index = seq[1].cast<long long>();
            c_distance = seq[2].cast<long long>();
            if (c_index < 0 || c_index >= n || c_distance == 0 ||
                c_distance <= -n || c_distance >= n ||
                c_index + c_distance < 0 || c_index + c_distance >= n)
                throw std::invalid_argument(
                    "alias: index + distance must be another element of 0..n-1");
        } else {
            throw std::invalid_argument(
                "corrupt must be ('flip', index, component, bit) or "
                "('alias', index, distance)");
        }
        if (c_index < 0 || c_index >= n)
            throw std::invalid_argument("corrupt: index must be in 0..n-1");
    }

    HIP_CHECK(hipSetDevice(device));
    const size_t total = (size_t)(guard + n + guard);
    DeviceBuffer<float4> src((size_t)n), dst(total);
    float4 *out = dst.get() + guard;
    HIP_CHECK(hipMemset(dst.get(), hbmpattern::kPoisonByte,
                        total * sizeof(float4)));
    hipLaunchKernelGGL(fill_pattern_kernel, dim3((unsigned)hbm_copy_blocks(n)),
                       dim3(256), 0, 0, src.get(), (size_t)n);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(hbm_copy_kernel, dim3((unsigned)blocks), dim3(threads), 0,
                       0, src.get(), out, (size_t)n);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());

    if (kind == kFlip)
        damage_from_host(out + c_index, c_component, c_bit, nullptr);
    else if (kind == kAlias)
        damage_from_host(out + c_index, 0, 0, out + c_index + c_distance);

    const PatternResult verdict = verify_pattern(out, (size_t)n);
    const bool guard_ok = guards_hold_poison(
        dst.get(), (size_t)guard * sizeof(float4), (size_t)n * sizeof(float4));

    const unsigned long long grid = (unsigned long long)blocks * threads;
    const unsigned long long un = (unsigned long long)n;
    // the kernel's condition i + 3 * stride < n, i = 0..stride-1
    const unsigned long long wide =
        un > 3 * grid ? std::min(un - 3 * grid, grid) : 0;

    py::dict res;
    res["mismatches"] = verdict.mismatches;
    res["first_bad"] = verdict.first_bad;
    res["guard_ok"] = guard_ok;
    res["blocks"] = blocks;
    res["threads"] = threads;
    res["stride"] = grid;
    res["wide_threads"] = wide;
    res["tail_threads"] = grid - wide;
    res["guard"] = guard;
    res["poison_byte"] = hbmpattern::kPoisonByte;
    if (return_data) {
        std::vector<char> all(total * sizeof(float4));
        HIP_CHECK(hipMemcpy(all.data(), dst.get(), all.size(),
                            hipMemcpyDeviceToHost));
        res["data"] = py::bytes(all.data(), all.size());  // guards included
    }
    return res;
}

// lds_probe_kernel at one shape; returns the raw error count.
// corrupt = (block, word, mask) xors mask into that word of that block.
long long lds_check(int device, long long lds_bytes, int blocks, int threads,
                    py::object corrupt) {
    if (lds_bytes <= 0 || lds_bytes % 4 || lds_bytes > (1ll << 30))
        throw std::invalid_argument("lds_bytes must be a positive multiple of 4");
    if (blocks < 1 || blocks > 65536)
        throw std::invalid_argument("blocks must be in 1..65536");
    require_whole_waves(threads);
    long long c_block = -1, c_word = -1, c_mask = 0;
    if (!corrupt.is_none()) {
        py::sequence seq = corrupt.cast<py::sequence>();
        if (py::len(seq) != 3)
            throw std::invalid_argument("corrupt must be (block, word, mask)");
        c_block = seq[0].cast<long long>();
        c_word = seq[1].cast<long long>();
        c_mask = seq[2].cast<long long>();
        if (c_block < 0 || c_block >= blocks || c_word < 0 ||
            c_word >= lds_bytes / 4 || c_mask < 1 || c_mask > 0xFFFFFFFFll)
            throw std::invalid_argument(
                "corrupt: block in 0..blocks-1, word in 0..lds_bytes/4-1, "
                "mask in 1..2^32-1");
    }

    HIP_CHECK(hipSetDevice(device));
    hipDeviceProp_t props;
    HIP_CHECK(hipGetDeviceProperties(&props, device));
    if ((size_t)lds_bytes > props.sharedMemPerBlock)
        throw std::invalid_argument(
            "lds_bytes is above this GPU's sharedMemPerBlock of " +
            std::to_string(props.sharedMemPerBlock));
    return run_lds_probe(blocks, threads, (int)lds_bytes, (int)c_block,
                         (int)c_word, (uint32_t)c_mask);
}

size_t shared_mem_per_block(int device) {
    hipDeviceProp_t props;
    HIP_CHECK(hipGetDeviceProperties(&props, device));
    return props.sharedMemPerBlock;
}

// The kernel that measure_mfma_tflops times, mfma_peak_kernel<2> at 512
// threads, with store = 1: returns its accumulators as float32 bytes,
// [blocks][8 waves][2 acc][16 regs][64 lanes].
py::bytes mfma_peak_check(int device, int iters, int blocks) {
    if (iters < 1 || iters > (1 << 20))
        throw std::invalid_argument("iters must be in 1..2^20");
    if (blocks < 1 || blocks > 4096)
        throw std::invalid_argument("blocks must be in 1..4096");
    HIP_CHECK(hipSetDevice(device));
    std::vector<float> h((size_t)blocks * 8 * 2 * 16 * 64);
    DeviceBuffer<float> d(h.size());
    // NaN wherever no wave stores
    HIP_CHECK(hipMemset(d.get(), 0xFF, h.size() * sizeof(float)));
    hipLaunchKernelGGL(mfma_peak_kernel<2>, dim3(blocks), dim3(512), 0, 0,
                       d.get(), iters, 1);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpy(h.data(), d.get(), h.size() * sizeof(float),
                        hipMemcpyDeviceToHost));
    return py::bytes((const char *)h.data(), h.size() * sizeof(float));
}

// ---------------- CU sweep ----------------

// Rounds a sweep launch runs when the caller passes reps = 0.  Measured on
// MI355X (profiles/cu_sweep_mi355x.md): already reps = 1 (22 us) reached all
// 1024 SIMDs in one launch, 35 of 35 times; 8 keeps each block alive 2.4x
// as long (53 us) and runs every product 8 times, for 1 % of the probe's
// 5.5 ms.
constexpr int kSweepDefaultReps = 8;
// The same for the extra sets, chosen the same way from
// profiles/cu_sweep_ext_mi355x.md: reps = 1 (mx 24 us, wide 25 us) reached
// all 1024 SIMDs in one launch 24 of 24 times each, so coverage asks for no
// more; 8 keeps a block alive 2.2x (mx, 52 us) and 2.5x (wide, 64 us) as
// long and runs every product 8 times, each under 1 % of the plain probe's
// 6.5 ms measured in the same session.  16 would double that again (85 and
// 110 us) for nothing the coverage needs.
constexpr int kSweepMxDefaultReps = 8;
constexpr int kSweepWideDefaultReps = 8;
constexpr int kSweepMaxLaunches = 4;

constexpr int sweep_default_reps(int set) {
    return set == cusweepx::kMx     ? kSweepMxDefaultReps
           : set == cusweepx::kWide ? kSweepWideDefaultReps
                                    : kSweepDefaultReps;
}

struct SimdId {
    int xcc, se, sh, cu, simd;
    bool operator<(const SimdId &o) const {
        return std::tie(xcc, se, sh, cu, simd) <
               std::tie(o.xcc, o.se, o.sh, o.cu, o.simd);
    }
};

// HW_ID of GCN/CDNA: SIMD_ID 5:4, CU_ID 11:8, SH_ID 12, SE_ID 14:13 (two
// bits from gfx942 on, 4 SEs per XCC); XCC_ID 3:0 of its own register.
SimdId decode_hw_id(uint32_t hw_id, uint32_t xcc_id) {
    return {(int)(xcc_id & 15), (int)(hw_id >> 13 & 3), (int)(hw_id >> 12 & 1),
            (int)(hw_id >> 8 & 15), (int)(hw_id >> 4 & 3)};
}

// where a result names a CU
py::dict place_dict(int xcc, int se, int sh, int cu) {
    py::dict d;
    d["xcc"] = xcc;
    d["se"] = se;
    d["sh"] = sh;
    d["cu"] = cu;
    return d;
}

py::tuple decode_hw_id_py(uint32_t hw_id, uint32_t xcc_id) {
    SimdId id = decode_hw_id(hw_id, xcc_id);
    return py::make_tuple(id.xcc, id.se, id.sh, id.cu, id.simd);
}

// "base", "mx" or "wide" -> cusweepx::Set
int sweep_set_of(const std::string &name) {
    for (int s = 0; s < cusweepx::kSets; ++s)
        if (name == cusweepx::kSetName[s]) return s;
    throw std::invalid_argument("pipe_set must be base, mx or wide, not " + name);
}

// A runtime index i in 0..N-1 as a compile-time constant: the value of
// fn(std::integral_constant<int, i>{}), there to choose a kernel instantiation.
template <int N, typename Fn, int I = 0>
auto with_index(int i, Fn &&fn) {
    if constexpr (I + 1 < N)
        if (i != I) return with_index<N, Fn, I + 1>(i, std::forward<Fn>(fn));
    return fn(std::integral_constant<int, I>{});
}

// What one kind of sweep (CU sweep, VALU sweep) hands to the shared runner:
// its kernel for one set, the set's table and LDS request, and how its
// units (pipes, ops) are called.
using SweepKernel = void (*)(const uint4 *, SweepRecord *, int, int, int, int);

struct SweepSpec {
    SweepKernel kernel;
    const std::vector<uint8_t> *table;
    int lds_bytes;
    int n_units;
    const char *(*unit_name)(int set, int unit);
    int set;
    const char *unit_key;   // "pipe" / "op"
    const char *units_key;  // "pipes" / "ops"
};

py::list sweep_unit_names(const SweepSpec &spec, uint32_t mask) {
    py::list names;
    for (int p = 0; p < spec.n_units; ++p)
        if (mask >> p & 1) names.append(spec.unit_name(spec.set, p));
    return names;
}

py::dict sweep_first_failure(const SweepSpec &spec, const SweepRecord &r) {
    py::dict first;
    first[spec.unit_key] = r.first_pipe < (uint32_t)spec.n_units
                               ? spec.unit_name(spec.set, (int)r.first_pipe) : "?";
    first["t"] = r.first_t;
    first["lane"] = r.first_lane;
    first["reg"] = r.first_reg;
    first["got"] = r.first_got;            // result register bits
    first["expected"] = r.first_expected;
    return first;
}

// inject = (block, wave, unit) or None -> inj[3], -1 = off
void parse_sweep_inject(py::object inject, int n_units, const char *unit_key,
                        int inj[3]) {
    inj[0] = inj[1] = inj[2] = -1;
    if (inject.is_none()) return;
    const std::string unit = unit_key;
    py::sequence seq = inject.cast<py::sequence>();
    if (py::len(seq) != 3)
        throw std::invalid_argument("inject must be (block, wave, " + unit + ")");
    for (int i = 0; i < 3; ++i) inj[i] = seq[i].cast<int>();
    if (inj[0] < 0 || inj[1] < 0 || inj[1] >= 4 || inj[2] < 0 || inj[2] >= n_units)
        throw std::invalid_argument(
            "inject: block >= 0, wave in 0..3, " + unit + " in 0.." +
            std::to_string(n_units - 1));
}

int checked_sweep_reps(int reps, int default_reps) {
    if (reps < 0) throw std::invalid_argument("reps must be >= 0");
    if (reps == 0) reps = default_reps;
    if (reps > (1 << 16)) throw std::invalid_argument("reps must be <= 65536");
    return reps;
}

// The host side of a known-answer sweep (cu_sweep_kernel, valu_sweep_kernel).
// One launch of cu_count blocks; where the records show a SIMD that no wave
// ran on, launch again with doubled reps (longer-lived blocks overlap more
// surely), at most kSweepMaxLaunches in all, accumulating coverage and
// failures.  inj = (block, wave, unit) simulates one bad unit, -1 = off.
py::dict run_sweep(int device, int reps, const int inj[3], const SweepSpec &spec) {
    HIP_CHECK(hipSetDevice(device));
    hipDeviceProp_t props;
    HIP_CHECK(hipGetDeviceProperties(&props, device));
    const int cu_count = props.multiProcessorCount;
    if (inj[0] >= cu_count)
        throw std::invalid_argument("inject: block must be below cu_count");
    const int lds_bytes = spec.lds_bytes;
    if ((size_t)lds_bytes > props.sharedMemPerBlock)
        throw std::runtime_error("the sweep tables do not fit this GPU's LDS");

    const std::vector<uint8_t> &table = *spec.table;
    DeviceBuffer<uint4> d_table(table.size() / sizeof(uint4));
    HIP_CHECK(hipMemcpy(d_table.get(), table.data(), table.size(),
                        hipMemcpyHostToDevice));
    const size_t n_rec = (size_t)cu_count * 4;
    DeviceBuffer<SweepRecord> d_rec(n_rec);
    std::vector<SweepRecord> h_rec(n_rec);

    std::map<std::tuple<int, int, int, int>, unsigned> simds_of_cu;
    struct Bad {
        uint32_t pipes = 0;
        unsigned long long lanes = 0;
        SweepRecord first;
    };
    std::map<SimdId, Bad> bad;
    py::list records;
    double sweep_ms = 0;
    int launches = 0, simds_covered = 0;
    bool complete = false;
    EventPair ev;
    while (launches < kSweepMaxLaunches && !complete) {
        if (launches) reps = std::min(reps * 2, 1 << 16);
        ++launches;
        HIP_CHECK(hipMemset(d_rec.get(), 0, n_rec * sizeof(SweepRecord)));
        sweep_ms += ev.time([&] {
            hipLaunchKernelGGL(spec.kernel, dim3(cu_count), dim3(256), lds_bytes,
                               0, d_table.get(), d_rec.get(), reps, inj[0],
                               inj[1], inj[2]);
        });
        HIP_CHECK(hipMemcpy(h_rec.data(), d_rec.get(),
                            n_rec * sizeof(SweepRecord), hipMemcpyDeviceToHost));

        for (const SweepRecord &r : h_rec) {
            const unsigned long long lanes =
                (unsigned long long)r.bad_lanes_hi << 32 | r.bad_lanes_lo;
            records.append(py::make_tuple(
                r.hw_id, r.xcc_id, r.fail_pipes, lanes, r.first_pipe, r.first_t,
                r.first_lane, r.first_reg, r.first_got, r.first_expected));
            const SimdId id = decode_hw_id(r.hw_id, r.xcc_id);
            simds_of_cu[{id.xcc, id.se, id.sh, id.cu}] |= 1u << id.simd;
            if (r.fail_pipes) {
                auto it = bad.find(id);
                if (it == bad.end()) it = bad.emplace(id, Bad{0, 0, r}).first;
                it->second.pipes |= r.fail_pipes;
                it->second.lanes |= lanes;
            }
        }
        simds_covered = 0;
        for (const auto &kv : simds_of_cu)
            simds_covered += __builtin_popcount(kv.second);
        complete = (int)simds_of_cu.size() == cu_count &&
                   simds_covered == 4 * cu_count;
    }

    py::list bad_list, uncovered;
    for (const auto &kv : bad) {
        py::dict b = place_dict(kv.first.xcc, kv.first.se, kv.first.sh, kv.first.cu);
        b["simd"] = kv.first.simd;
        b[spec.units_key] = sweep_unit_names(spec, kv.second.pipes);
        b["bad_lanes"] = kv.second.lanes;
        b["first"] = sweep_first_failure(spec, kv.second.first);
        bad_list.append(b);
    }
    for (const auto &kv : simds_of_cu)
        if (kv.second != 0xF) {
            py::dict u = std::apply(place_dict, kv.first);
            py::list seen;
            for (int s = 0; s < 4; ++s)
                if (kv.second >> s & 1) seen.append(s);
            u["simds"] = seen;
            uncovered.append(u);
        }

    py::dict out;
    out["cu_count"] = cu_count;
    out["cus_covered"] = (int)simds_of_cu.size();
    out["simds_covered"] = simds_covered;
    out["coverage_complete"] = complete;
    out["launches"] = launches;
    out["reps"] = reps;  // of the last launch
    out["waves_checked"] = (uint64_t)n_rec * launches;
    out[spec.units_key] = sweep_unit_names(spec, ~0u);
    out["bad"] = bad_list;
    out["uncovered"] = uncovered;
    out["records"] = records;
    out["sweep_ms"] = sweep_ms;
    out["ok"] = bad.empty();
    return out;
}

// Known-answer MFMA products on every SIMD of every CU (cu_sweep_kernel,
// run_sweep).  inject = (block, wave, pipe) simulates one bad pipe.  pipe_set
// chooses the pipes: "base" (sweep_table.h), "mx" or "wide"
// (sweep_table_ext.h); pipe indices and names are the set's own.
py::dict cu_sweep(int device, int reps, py::object inject,
                  const std::string &pipe_set) {
    const int set = sweep_set_of(pipe_set);
    int inj[3];
    parse_sweep_inject(inject, cusweepx::n_pipes(set), "pipe", inj);
    reps = checked_sweep_reps(reps, sweep_default_reps(set));

    // built on a set's first use (under the GIL)
    static std::vector<uint8_t> tables[cusweepx::kSets];
    if (tables[set].empty()) tables[set] = cusweepx::build_table(set);
    const SweepSpec spec = {
        with_index<cusweepx::kSets>(set, [](auto s) -> SweepKernel {
            return cu_sweep_kernel<decltype(s)::value>;
        }),
        &tables[set], cusweepx::lds_bytes(set), cusweepx::n_pipes(set),
        [](int s, int p) { return cusweepx::pipe_name(s, p); }, set, "pipe", "pipes"};
    py::dict out = run_sweep(device, reps, inj, spec);
    out["pipe_set"] = pipe_set;
    return out;
}

// The tables of an extra set (mx or wide) for the tests: per test the
// packed fragments, for mx the 64 scale words of each side and the op_sel
// pair, and the expected result register bits; `table` is the whole blob
// and `offset` each test's place in it (the pad a lane's 32-byte operand
// load reads past an fp4 / fp6 fragment is what follows there).
py::dict cu_sweep_reference_ext(int set) {
    py::list pipes;
    for (int p = 0; p < cusweepx::n_pipes(set); ++p) {
        const cusweepx::PipeDesc &d = cusweepx::desc(set, p);
        const int regs = cusweepx::ext_regs(set, p);
        py::list tests;
        for (int t = 0; t < cusweepx::kTests; ++t) {
            const cusweepx::TestVector v = cusweepx::make_test(set, p, t);
            py::list expected_bits;  // [64 lanes][regs]
            for (int l = 0; l < cusweepx::kLanes; ++l) {
                py::list bits;
                for (int r = 0; r < regs; ++r)
                    bits.append(v.expected[(size_t)l * regs + r]);
                expected_bits.append(bits);
            }
            py::dict test;
            test["a_frag"] = py::bytes((const char *)v.a_frag.data(), v.a_frag.size());
            test["b_frag"] = py::bytes((const char *)v.b_frag.data(), v.b_frag.size());
            if (cusweepx::scaled(set)) {
                test["scale_a"] = v.scale_a;
                test["scale_b"] = v.scale_b;
                test["sel"] = py::make_tuple(cusweepx::sel_a(t), cusweepx::sel_b(t));
            }
            test["expected_bits"] = expected_bits;
            test["offset"] = cusweepx::test_offset(set, p, t);
            test["abs_sum_max"] = v.abs_sum_max;
            test["unit_shift"] = v.unit_shift;
            tests.append(test);
        }
        py::dict pipe;
        pipe["name"] = d.name;
        pipe["M"] = d.M;
        pipe["N"] = d.N;
        pipe["K"] = d.K;
        pipe["regs"] = regs;
        pipe["result"] = d.result == cusweepx::RF32   ? "f32"
                         : d.result == cusweepx::RI32 ? "i32" : "f64";
        pipe["a_format"] = cusweepx::kFmt[d.a].name;
        pipe["b_format"] = cusweepx::kFmt[d.b].name;
        pipe["frag_bytes_a"] = cusweepx::ext_frag_bytes(set, p, 0);
        pipe["frag_bytes_b"] = cusweepx::ext_frag_bytes(set, p, 1);
        pipe["tests"] = tests;
        pipes.append(pipe);
    }
    const std::vector<uint8_t> table = cusweepx::build_table(set);
    py::dict out;
    out["pipe_set"] = cusweepx::kSetName[set];
    out["pipes"] = pipes;
    out["tests_per_pipe"] = cusweepx::kTests;
    out["table_bytes"] = cusweepx::table_bytes(set);
    out["lds_bytes"] = cusweepx::lds_bytes(set);
    out["table"] = py::bytes((const char *)table.data(), table.size());
    out["default_reps"] = sweep_default_reps(set);
    return out;
}

// The sweep's tables for the tests: no HIP call, works without a GPU.
py::dict cu_sweep_reference(const std::string &pipe_set) {
    const int set = sweep_set_of(pipe_set);
    if (set != cusweepx::kBase) return cu_sweep_reference_ext(set);
    auto matrix = [](const std::vector<int> &m, int rows, int cols) {
        py::list out;
        for (int i = 0; i < rows; ++i) {
            py::list row;
            for (int j = 0; j < cols; ++j) row.append(m[(size_t)i * cols + j]);
            out.append(row);
        }
        return out;
    };
    py::list pipes;
    for (int p = 0; p < cusweep::kPipes; ++p) {
        const cusweep::PipeDesc &d = cusweep::kPipeDesc[p];
        py::list tests;
        for (int t = 0; t < cusweep::kTests; ++t) {
            const cusweep::TestVector v = cusweep::make_test(p, t);
            py::list expected, expected_bits;  // [64 lanes][regs]
            for (int l = 0; l < cusweep::kLanes; ++l) {
                py::list vals, bits;
                for (int r = 0; r < d.regs; ++r) {
                    const uint32_t b = v.expected[(size_t)l * d.regs + r];
                    bits.append(b);
                    if (d.int_result) {
                        vals.append((int32_t)b);
                    } else {
                        float f;
                        std::memcpy(&f, &b, 4);
                        vals.append(f);
                    }
                }
                expected.append(vals);
                expected_bits.append(bits);
            }
            py::dict test;
            test["A"] = matrix(v.A, d.M, d.K);
            test["B"] = matrix(v.B, d.K, d.N);
            test["expected"] = expected;
            test["expected_bits"] = expected_bits;
            test["a_frag"] = py::bytes((const char *)v.a_frag.data(), v.a_frag.size());
            test["b_frag"] = py::bytes((const char *)v.b_frag.data(), v.b_frag.size());
            tests.append(test);
        }
        py::dict pipe;
        pipe["name"] = d.name;
        pipe["M"] = d.M;
        pipe["N"] = d.N;
        pipe["K"] = d.K;
        pipe["regs"] = d.regs;
        pipe["int_result"] = d.int_result;
        pipe["tests"] = tests;
        pipes.append(pipe);
    }
    py::dict out;
    out["pipes"] = pipes;
    out["tests_per_pipe"] = cusweep::kTests;
    out["table_bytes"] = cusweep::kTableBytes;
    out["default_reps"] = kSweepDefaultReps;
    return out;
}

// ---- mfma_raw: one wave, one product, caller-supplied fragments ----

using RawKernel = void (*)(const unsigned char *, const unsigned char *,
                           const uint32_t *, const uint32_t *, uint32_t *);

// One product of one pipe of any set on one wave, from packed per-lane
// fragments (and, for an mx pipe, the 64 scale words of each side and the
// byte selects) laid out as in the tables: the raw result registers,
// [64 lanes][regs] uint32.  For the tests and for establishing operand maps
// with one-hot data.  Names and lengths are checked before any HIP call.
py::bytes mfma_raw(int device, const std::string &pipe, py::bytes a_frag,
                   py::bytes b_frag, py::object scale_a, py::object scale_b,
                   std::pair<int, int> sel) {
    int set = -1, p = -1;
    for (int s = 0; s < cusweepx::kSets; ++s)
        for (int q = 0; q < cusweepx::n_pipes(s); ++q)
            if (pipe == cusweepx::pipe_name(s, q)) {
                set = s;
                p = q;
            }
    if (set < 0) throw std::invalid_argument("mfma_raw: unknown pipe " + pipe);
    const std::string a = a_frag, b = b_frag;
    const size_t fa = (size_t)cusweepx::kLanes * cusweepx::frag_bytes(set, p, 0);
    const size_t fb = (size_t)cusweepx::kLanes * cusweepx::frag_bytes(set, p, 1);
    if (a.size() != fa || b.size() != fb)
        throw std::invalid_argument(
            "mfma_raw: " + pipe + " takes " + std::to_string(fa) + " bytes of A and " +
            std::to_string(fb) + " of B");
    if (sel.first < 0 || sel.first > 3 || sel.second < 0 || sel.second > 3)
        throw std::invalid_argument("mfma_raw: sel is a pair of byte selects 0..3");
    std::vector<uint32_t> scales(2 * cusweepx::kLanes, 0x7F7F7F7Fu);
    const bool mx = cusweepx::scaled(set);
    if (!mx && (!scale_a.is_none() || !scale_b.is_none() || sel.first || sel.second))
        throw std::invalid_argument("mfma_raw: " + pipe + " takes no scales");
    for (int side = 0; side < 2; ++side) {
        const py::object &given = side ? scale_b : scale_a;
        if (given.is_none()) continue;
        const std::string raw = given.cast<py::bytes>();
        if (raw.size() != 4 * (size_t)cusweepx::kLanes)
            throw std::invalid_argument("mfma_raw: a side's scales are 64 words, 256 bytes");
        std::memcpy(&scales[(size_t)side * cusweepx::kLanes], raw.data(), raw.size());
    }
    const int code = sel.first * 4 + sel.second;
    // an mx pipe's byte selects are template arguments
    RawKernel kernel = with_index<cusweepx::kSets>(set, [&](auto s) {
        constexpr int S = decltype(s)::value;
        return with_index<cusweepx::n_pipes(S)>(p, [&](auto q) -> RawKernel {
            constexpr int Q = decltype(q)::value;
            if constexpr (S == cusweepx::kMx)
                return with_index<16>(code, [](auto c) -> RawKernel {
                    constexpr int C = decltype(c)::value;
                    return mfma_raw_kernel<S, Q, C / 4, C % 4>;
                });
            else
                return mfma_raw_kernel<S, Q, 0, 0>;
        });
    });

    HIP_CHECK(hipSetDevice(device));
    // every lane's operand load may read 32 bytes from its fragment's start
    constexpr size_t kPad = 32;
    DeviceBuffer<unsigned char> d_a(fa + kPad), d_b(fb + kPad);
    HIP_CHECK(hipMemset(d_a.get(), 0xA5, fa + kPad));
    HIP_CHECK(hipMemset(d_b.get(), 0xA5, fb + kPad));
    HIP_CHECK(hipMemcpy(d_a.get(), a.data(), fa, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_b.get(), b.data(), fb, hipMemcpyHostToDevice));
    DeviceBuffer<uint32_t> d_s(scales.size());
    HIP_CHECK(hipMemcpy(d_s.get(), scales.data(), scales.size() * 4,
                        hipMemcpyHostToDevice));
    const size_t n_out = (size_t)cusweepx::kLanes * cusweepx::regs(set, p);
    DeviceBuffer<uint32_t> d_out(n_out);
    HIP_CHECK(hipMemset(d_out.get(), 0xFF, n_out * 4));
    hipLaunchKernelGGL(kernel, dim3(1), dim3(64), 0, 0, d_a.get(), d_b.get(),
                       d_s.get(), d_s.get() + cusweepx::kLanes, d_out.get());
    HIP_CHECK(hipGetLastError());
    std::vector<uint32_t> h(n_out);
    HIP_CHECK(hipMemcpy(h.data(), d_out.get(), n_out * 4, hipMemcpyDeviceToHost));
    return py::bytes((const char *)h.data(), n_out * 4);
}

// ---------------- VALU sweep ----------------

// Rounds a VALU sweep launch runs when the caller passes reps = 0, per set
// (valusweep::Set), chosen from profiles/valu_sweep_mi355x.md as the CU
// sweep's were: reps = 1 already reached all 1024 SIMDs in one launch every
// time, so coverage asks for no more; 8 runs every op 8 times on every SIMD
// and keeps the six sets together under a tenth of the plain probe.
constexpr int kValuDefaultReps[valusweep::kSets] = {8, 8, 8, 8, 8, 8};

int valu_set_of(const std::string &name) {
    for (int s = 0; s < valusweep::kSets; ++s)
        if (name == valusweep::kSetName[s]) return s;
    throw std::invalid_argument(
        "op_set must be fma, int, cvt, xlane, salu or trans, not " + name);
}

const std::vector<uint8_t> &valu_table(int set) {
    // built on a set's first use (under the GIL)
    static std::vector<uint8_t> tables[valusweep::kSets];
    if (tables[set].empty()) tables[set] = valusweep::build_table(set);
    return tables[set];
}

// Known-answer vector, conversion, cross-lane, scalar and transcendental
// ops on every SIMD of every CU (valu_sweep_kernel, run_sweep): the dict of
// cu_sweep with `ops` and `op_set` in the place of `pipes` and `pipe_set`.
// inject = (block, wave, op) simulates one bad op.
py::dict valu_sweep(int device, int reps, py::object inject,
                    const std::string &op_set) {
    const int set = valu_set_of(op_set);
    int inj[3];
    parse_sweep_inject(inject, valusweep::n_ops(set), "op", inj);
    reps = checked_sweep_reps(reps, kValuDefaultReps[set]);
    const SweepSpec spec = {
        with_index<valusweep::kSets>(set, [](auto s) -> SweepKernel {
            return valu_sweep_kernel<decltype(s)::value>;
        }),
        &valu_table(set), valusweep::lds_bytes(set), valusweep::n_ops(set),
        [](int s, int op) { return valusweep::desc(s, op).name; }, set, "op", "ops"};
    py::dict out = run_sweep(device, reps, inj, spec);
    out["op_set"] = op_set;
    return out;
}

// The VALU sweep's tables for the tests: the packed table, and per op its
// descriptor and each test's place.  No HIP call, works without a GPU.
py::dict valu_sweep_reference(const std::string &op_set) {
    const int set = valu_set_of(op_set);
    py::list ops;
    for (int op = 0; op < valusweep::n_ops(set); ++op) {
        const valusweep::OpDesc &d = valusweep::desc(set, op);
        py::dict o;
        o["name"] = d.name;
        o["mnemonic"] = d.mnemonic;
        o["widths"] = py::make_tuple(d.w[0], d.w[1], d.w[2], d.w[3]);
        o["in_words"] = valusweep::in_words(set, op);
        o["regs"] = (int)d.regs;
        o["vary"] = py::make_tuple(d.vary[0], d.vary[1], d.vary[2], d.vary[3]);
        o["out_vary"] = py::make_tuple(d.out_vary[0], d.out_vary[1], d.out_vary[2],
                                       d.out_vary[3]);
        py::list offsets;
        for (int t = 0; t < valusweep::n_tests(set); ++t)
            offsets.append(valusweep::test_offset(set, op, t));
        o["offsets"] = offsets;
        ops.append(o);
    }
    const std::vector<uint8_t> &table = valu_table(set);
    py::dict out;
    out["op_set"] = op_set;
    out["ops"] = ops;
    out["tests_per_op"] = valusweep::n_tests(set);
    out["lanes"] = valusweep::lanes(set);
    out["table_bytes"] = valusweep::table_bytes(set);
    out["lds_bytes"] = valusweep::lds_bytes(set);
    out["table"] = py::bytes((const char *)table.data(), table.size());
    out["default_reps"] = kValuDefaultReps[set];
    out["inject"] = py::make_tuple(kSweepInjectLane, kSweepInjectReg, kSweepInjectBit);
    return out;
}

using ValuRawKernel = void (*)(const uint32_t *, uint32_t *);

// One wave of one op of any set on caller-supplied operand words: a, b, c
// and old are 64 lanes x the descriptor's width of uint32 each, None where
// the op takes none (the scalar ops and the lane selects read lane 0); the
// raw result registers, out[lane * regs + r] uint32.  The study and test
// tool, the counterpart of mfma_raw.  Names and lengths are checked before
// any HIP call.
py::bytes valu_raw(int device, const std::string &op_name, py::object a,
                   py::object b, py::object c, py::object old) {
    int set = -1, op = -1;
    for (int s = 0; s < valusweep::kSets; ++s)
        for (int q = 0; q < valusweep::n_ops(s); ++q)
            if (op_name == valusweep::desc(s, q).name) {
                set = s;
                op = q;
            }
    if (set < 0) throw std::invalid_argument("valu_raw: unknown op " + op_name);
    const valusweep::OpDesc &d = valusweep::desc(set, op);
    const int NI = valusweep::in_words(set, op);
    std::vector<uint32_t> in((size_t)valusweep::kLanes * NI);
    const py::object *given[4] = {&a, &b, &c, &old};
    const char *const label[4] = {"a", "b", "c", "old"};
    for (int which = 0; which < 4; ++which) {
        const int w = d.w[which], at = valusweep::in_offset(set, op, which);
        if (given[which]->is_none()) {
            if (w)
                throw std::invalid_argument("valu_raw: " + op_name + " takes " + label[which]);
            continue;
        }
        if (!w)
            throw std::invalid_argument("valu_raw: " + op_name + " takes no " + label[which]);
        if (!py::isinstance<py::bytes>(*given[which]))
            throw std::invalid_argument(std::string("valu_raw: ") + label[which] +
                                        " must be bytes");
        const std::string raw = given[which]->cast<py::bytes>();
        if (raw.size() != (size_t)valusweep::kLanes * w * 4)
            throw std::invalid_argument(
                "valu_raw: " + std::string(label[which]) + " of " + op_name + " is 64 lanes x " +
                std::to_string(w) + " words, " + std::to_string(valusweep::kLanes * w * 4) +
                " bytes");
        for (int l = 0; l < valusweep::kLanes; ++l)
            std::memcpy(&in[(size_t)l * NI + at], raw.data() + (size_t)l * w * 4, (size_t)w * 4);
    }
    ValuRawKernel kernel = with_index<valusweep::kSets>(set, [&](auto s) {
        constexpr int S = decltype(s)::value;
        return with_index<valusweep::n_ops(S)>(op, [](auto o) -> ValuRawKernel {
            return valu_raw_kernel<S, decltype(o)::value>;
        });
    });

    HIP_CHECK(hipSetDevice(device));
    DeviceBuffer<uint32_t> d_in(in.size());
    HIP_CHECK(hipMemcpy(d_in.get(), in.data(), in.size() * 4, hipMemcpyHostToDevice));
    const size_t n_out = (size_t)valusweep::kLanes * d.regs;
    DeviceBuffer<uint32_t> d_out(n_out);
    HIP_CHECK(hipMemset(d_out.get(), 0xFF, n_out * 4));
    hipLaunchKernelGGL(kernel, dim3(1), dim3(64), 0, 0, d_in.get(), d_out.get());
    HIP_CHECK(hipGetLastError());
    std::vector<uint32_t> h(n_out);
    HIP_CHECK(hipMemcpy(h.data(), d_out.get(), n_out * 4, hipMemcpyDeviceToHost));
    return py::bytes((const char *)h.data(), n_out * 4);
}

// ---------------- HBM scrub ----------------

constexpr long long kScrubDefaultSlabBytes = 4ll << 30;
constexpr long long kScrubMaxSlabBytes = 64ll << 30;
constexpr long long kScrubMaxSlabs = 65536;
constexpr long long kScrubMaxData = 1ll << 21;  // elements for return_data
constexpr long long kScrubMaxRecords = 4096;
// twice the Infinity Cache: from here on a line is read back from HBM
constexpr unsigned long long kScrubBeyondCacheBytes = 512ull << 20;
constexpr long long kMarchReferenceMaxCount = 1ll << 24;

int march_pattern_by_name(const std::string &name) {
    for (int p = 0; p < hbmmarch::kPatterns; ++p)
        if (name == hbmmarch::kPatternNames[p]) return p;
    throw std::invalid_argument("unknown pattern '" + name +
                                "' (address, solid, checker, random)");
}

// A sequence of names of `what`s -> their indices by lookup (which throws on
// an unknown name), in the order given: at least one, none twice.
template <typename Lookup>
std::vector<int> names_to_indices(const py::object &names, const std::string &what,
                                  Lookup lookup) {
    std::vector<int> out;
    try {
        for (py::handle h : names.cast<py::sequence>()) {
            const int i = lookup(h.cast<std::string>());
            if (std::find(out.begin(), out.end(), i) != out.end())
                throw std::invalid_argument("a " + what + " is given twice");
            out.push_back(i);
        }
    } catch (const py::cast_error &) {
        throw std::invalid_argument(what + "s must be a sequence of names");
    } catch (const py::type_error &) {
        throw std::invalid_argument(what + "s must be a sequence of names");
    }
    if (out.empty()) throw std::invalid_argument(what + "s must name at least one");
    return out;
}

const char *march_mode_name(int mode) {
    return mode == kMarchWrite ? "march_write"
           : mode == kMarchRW  ? "march_rw"
                               : "march_read";
}

// guard + n + guard elements of device memory, freed on scope exit
struct ScrubSlab {
    char *alloc = nullptr;
    size_t n = 0;                  // elements under test
    unsigned long long base = 0;   // global index of the first
};

struct ScrubSlabs {
    std::vector<ScrubSlab> slabs;
    ~ScrubSlabs() {
        for (ScrubSlab &s : slabs) (void)hipFree(s.alloc);
    }
};

struct ScrubCorruption {
    enum Kind { kFlip, kAlias } kind;
    int pattern;
    long long after_step, element, word, bit, distance;
};

const char *const kScrubCorruptForm =
    "corrupt must be (pattern, after_step, 'flip', element, word, bit) or "
    "(pattern, after_step, 'alias', element, distance), or a list of such";

ScrubCorruption parse_scrub_corruption(const py::sequence &seq,
                                       const std::vector<int> &pats,
                                       long long n) {
    if (py::len(seq) < 5) throw std::invalid_argument(kScrubCorruptForm);
    ScrubCorruption c{};
    c.pattern = march_pattern_by_name(seq[0].cast<std::string>());
    if (std::find(pats.begin(), pats.end(), c.pattern) == pats.end())
        throw std::invalid_argument("corrupt: that pattern is not run");
    c.after_step = seq[1].cast<long long>();
    if (c.after_step < 0 || c.after_step > 2)
        throw std::invalid_argument("corrupt: after_step must be in 0..2");
    const std::string what = seq[2].cast<std::string>();
    c.element = seq[3].cast<long long>();
    if (c.element < 0 || c.element >= n)
        throw std::invalid_argument("corrupt: element must be in 0..n-1");
    if (what == "flip" && py::len(seq) == 6) {
        c.kind = ScrubCorruption::kFlip;
        c.word = seq[4].cast<long long>();
        c.bit = seq[5].cast<long long>();
        if (c.word < 0 || c.word > 3 || c.bit < 0 || c.bit > 31)
            throw std::invalid_argument("flip: word in 0..3, bit in 0..31");
    } else if (what == "alias" && py::len(seq) == 5) {
        c.kind = ScrubCorruption::kAlias;
        c.distance = seq[4].cast<long long>();
        if (c.distance == 0 || c.distance <= -n || c.distance >= n ||
            c.element + c.distance < 0 || c.element + c.distance >= n)
            throw std::invalid_argument(
                "alias: element + distance must be another element");
    } else {
        throw std::invalid_argument(kScrubCorruptForm);
    }
    return c;
}

void launch_march(u32x4 *data, const MarchParams &a, MarchReport *rep,
                  MarchRecord *records, uint32_t *range_bad) {
    const dim3 grid((unsigned)hbm_copy_blocks(a.n)), block(256);
    switch (march_mode_of_step(a.step)) {
    case kMarchWrite:
        hipLaunchKernelGGL((march_kernel<kMarchWrite>), grid, block, 0, 0, data,
                           a, rep, records, range_bad);
        break;
    case kMarchRW:
        hipLaunchKernelGGL((march_kernel<kMarchRW>), grid, block, 0, 0, data, a,
                           rep, records, range_bad);
        break;
    default:
        hipLaunchKernelGGL((march_kernel<kMarchRead>), grid, block, 0, 0, data,
                           a, rep, records, range_bad);
    }
    HIP_CHECK(hipGetLastError());
}

// In-place march test (hbm_march.h) of `bytes` of device memory, allocated
// in slabs of at most slab_bytes, each between two poisoned guard bands of
// `guard` elements.  Each step runs over ALL slabs before the next starts,
// so between the write of a line and its read-back the whole region has
// moved through the caches.  A slab that cannot be allocated ends the
// allocation; what was obtained is tested.
// corrupt = (pattern, after_step, "flip", element, word, bit) or
//           (pattern, after_step, "alias", element, distance),
//           or a list of such,
// damages memory from the host, with hipMemcpy and no kernel, between step
// after_step of that pattern and the step that follows; element is global.
py::dict hbm_scrub(int device, long long bytes, long long slab_bytes,
                   long long guard, py::object patterns,
                   unsigned long long seed, py::object corrupt,
                   long long max_records, bool return_data) {
    if (bytes < 16 || bytes % 16)
        throw std::invalid_argument("bytes must be a positive multiple of 16");
    if (slab_bytes < 16 || slab_bytes % 16 || slab_bytes > kScrubMaxSlabBytes)
        throw std::invalid_argument(
            "slab_bytes must be a multiple of 16 in 16..64 GiB");
    if ((bytes + slab_bytes - 1) / slab_bytes > kScrubMaxSlabs)
        throw std::invalid_argument("bytes / slab_bytes must be at most 65536");
    if (guard < 0 || guard > kCopyCheckMaxGuard)
        throw std::invalid_argument("guard must be in 0..2^20 float4s");
    if (max_records < 1 || max_records > kScrubMaxRecords)
        throw std::invalid_argument("max_records must be in 1..4096");
    const long long n_req = bytes / 16, slab_elems = slab_bytes / 16;
    if (return_data && n_req > kScrubMaxData)
        throw std::invalid_argument("return_data needs bytes <= 16 * 2^21");

    std::vector<int> pats;
    if (patterns.is_none())
        for (int p = 0; p < hbmmarch::kPatterns; ++p) pats.push_back(p);
    else
        pats = names_to_indices(patterns, "pattern", march_pattern_by_name);

    // one corruption, or a list of them
    std::vector<ScrubCorruption> damage;
    if (!corrupt.is_none()) try {
        py::sequence seq = corrupt.cast<py::sequence>();
        if (py::len(seq) && py::isinstance<py::str>(seq[0])) {
            damage.push_back(parse_scrub_corruption(seq, pats, n_req));
        } else {
            if (!py::len(seq)) throw std::invalid_argument(kScrubCorruptForm);
            for (py::handle one : seq)
                damage.push_back(parse_scrub_corruption(
                    one.cast<py::sequence>(), pats, n_req));
        }
    } catch (const py::cast_error &) {
        throw std::invalid_argument(kScrubCorruptForm);
    } catch (const py::type_error &) {
        throw std::invalid_argument(kScrubCorruptForm);
    }

    HIP_CHECK(hipSetDevice(device));
    size_t free_before = 0, total_mem = 0;
    HIP_CHECK(hipMemGetInfo(&free_before, &total_mem));

    const auto wall_start = std::chrono::steady_clock::now();
    ScrubSlabs owned;
    std::vector<ScrubSlab> &slabs = owned.slabs;
    const size_t guard_bytes = (size_t)guard * 16;
    unsigned long long n_total = 0;
    while (n_total < (unsigned long long)n_req) {
        ScrubSlab s;
        s.n = (size_t)std::min<unsigned long long>(slab_elems, n_req - n_total);
        s.base = n_total;
        const size_t alloc_bytes = 2 * guard_bytes + s.n * 16;
        if (hipMalloc(reinterpret_cast<void **>(&s.alloc), alloc_bytes) !=
            hipSuccess) {
            (void)hipGetLastError();  // clear it: test what was obtained
            break;
        }
        slabs.push_back(s);
        n_total += s.n;
        HIP_CHECK(hipMemset(s.alloc, hbmpattern::kPoisonByte, alloc_bytes));
    }
    if (slabs.empty())
        throw std::runtime_error("hbm_scrub: no slab could be allocated");
    for (const ScrubCorruption &c : damage)
        if ((unsigned long long)c.element >= n_total ||
            (unsigned long long)(c.element + c.distance) >= n_total)
            throw std::runtime_error(
                "hbm_scrub: corrupt names an element beyond what was allocated");
    auto data_of = [&](const ScrubSlab &s) {
        return reinterpret_cast<u32x4 *>(s.alloc + guard_bytes);
    };
    auto address_of = [&](unsigned long long elem) {
        const ScrubSlab &s = slabs[elem / slab_elems];
        return reinterpret_cast<char *>(data_of(s)) + (elem - s.base) * 16;
    };

    const size_t n_ranges =
        (size_t)((n_total + (1ull << kMarchRangeShift) - 1) >> kMarchRangeShift);
    DeviceBuffer<MarchReport> d_rep(1);
    DeviceBuffer<MarchRecord> d_rec((size_t)max_records);
    DeviceBuffer<uint32_t> d_ranges(n_ranges);
    MarchReport rep{};
    rep.first_bad = ~0ull;
    HIP_CHECK(hipMemcpy(d_rep.get(), &rep, sizeof(rep), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemset(d_rec.get(), 0, (size_t)max_records * sizeof(MarchRecord)));
    HIP_CHECK(hipMemset(d_ranges.get(), 0, n_ranges * sizeof(uint32_t)));
    HIP_CHECK(hipDeviceSynchronize());

    double mode_ms[3] = {0, 0, 0}, mode_bytes[3] = {0, 0, 0};
    EventPair ev;
    for (int p : pats) {
        for (int step = 0; step < hbmmarch::kSteps; ++step) {
            const float ms = ev.time([&] {
                for (size_t k = 0; k < slabs.size(); ++k) {
                    // the descending step also takes the slabs from the top
                    const ScrubSlab &s = slabs[hbmmarch::step_descends(step)
                                                   ? slabs.size() - 1 - k : k];
                    MarchParams a;
                    a.pattern = p;
                    a.step = step;
                    a.seed = seed;
                    a.base = s.base;
                    a.n = s.n;
                    a.max_records = (uint32_t)max_records;
                    launch_march(data_of(s), a, d_rep.get(), d_rec.get(),
                                 d_ranges.get());
                }
            });
            const int mode = march_mode_of_step(step);
            mode_ms[mode] += ms;
            mode_bytes[mode] += (mode == kMarchRW ? 2.0 : 1.0) * 16.0 * n_total;

            for (const ScrubCorruption &c : damage) {
                if (c.pattern != p || c.after_step != step) continue;
                damage_from_host(address_of(c.element), c.word, c.bit,
                                 c.kind == ScrubCorruption::kAlias
                                     ? address_of(c.element + c.distance) : nullptr);
                HIP_CHECK(hipDeviceSynchronize());
            }
        }
    }

    HIP_CHECK(hipMemcpy(&rep, d_rep.get(), sizeof(rep), hipMemcpyDeviceToHost));
    const size_t n_rec = std::min<size_t>(rep.n_records, (size_t)max_records);
    std::vector<MarchRecord> h_rec(n_rec);
    if (n_rec)
        HIP_CHECK(hipMemcpy(h_rec.data(), d_rec.get(),
                            n_rec * sizeof(MarchRecord), hipMemcpyDeviceToHost));
    std::vector<uint32_t> h_ranges(n_ranges);
    HIP_CHECK(hipMemcpy(h_ranges.data(), d_ranges.get(),
                        n_ranges * sizeof(uint32_t), hipMemcpyDeviceToHost));

    bool guard_ok = true;
    for (const ScrubSlab &s : slabs)
        guard_ok &= guards_hold_poison(s.alloc, guard_bytes, s.n * 16);
    const double wall_ms =
        std::chrono::duration<double, std::milli>(
            std::chrono::steady_clock::now() - wall_start).count();

    auto record_dict = [](const MarchRecord &r) {
        py::dict d;
        d["pattern"] = r.pattern < (uint32_t)hbmmarch::kPatterns
                           ? hbmmarch::kPatternNames[r.pattern] : "?";
        d["step"] = r.step;
        d["index"] = r.index;
        d["word"] = r.word;
        d["got"] = r.got;
        d["expected"] = r.expected;
        return d;
    };
    py::list records;
    for (const MarchRecord &r : h_rec) records.append(record_dict(r));

    // 2 MiB-aligned ranges of the scrub's byte offsets with a bad element,
    // neighbours merged
    py::list bad_ranges;
    for (size_t lo = 0; lo < n_ranges; ++lo) {
        if (!h_ranges[lo]) continue;
        size_t hi = lo;
        unsigned long long count = 0;
        while (hi < n_ranges && h_ranges[hi]) count += h_ranges[hi++];
        const unsigned long long first_elem = (unsigned long long)lo
                                              << kMarchRangeShift;
        const unsigned long long end_elem = std::min<unsigned long long>(
            (unsigned long long)hi << kMarchRangeShift, n_total);
        py::dict r;
        r["start"] = first_elem * 16;
        r["end"] = end_elem * 16 - 1;  // inclusive
        r["mismatches"] = count;
        r["slab"] = first_elem / slab_elems;
        r["device_address"] = (unsigned long long)(uintptr_t)address_of(first_elem);
        const MarchRecord *first = nullptr;  // the lowest record in the range
        for (const MarchRecord &rec : h_rec)
            if (rec.index >= first_elem && rec.index < end_elem &&
                (!first || rec.index < first->index))
                first = &rec;
        r["first"] = first ? py::object(record_dict(*first)) : py::none();
        bad_ranges.append(r);
        lo = hi;
    }

    py::dict steps;
    double scrub_ms = 0;
    for (int mode = 0; mode < 3; ++mode) {
        py::dict m;
        m["bytes"] = (unsigned long long)mode_bytes[mode];
        m["ms"] = mode_ms[mode];
        m["gbps"] = mode_ms[mode] > 0 ? mode_bytes[mode] / (mode_ms[mode] * 1e6) : 0.0;
        steps[march_mode_name(mode)] = m;
        scrub_ms += mode_ms[mode];
    }
    py::list pattern_names;
    for (int p : pats) pattern_names.append(hbmmarch::kPatternNames[p]);

    py::dict out;
    out["bytes_requested"] = bytes;
    out["bytes_tested"] = n_total * 16;
    out["slabs"] = slabs.size();
    out["slab_bytes"] = slab_bytes;
    out["guard"] = guard;
    out["patterns"] = pattern_names;
    out["seed"] = seed;
    out["vram_bytes"] = (uint64_t)total_mem;
    out["vram_free_before"] = (uint64_t)free_before;
    out["mismatches"] = rep.mismatches;
    out["first_bad"] = rep.mismatches ? (long long)rep.first_bad : -1;
    out["bad_bits"] = py::make_tuple(rep.bad_bits[0], rep.bad_bits[1],
                                     rep.bad_bits[2], rep.bad_bits[3]);
    out["records"] = records;
    out["bad_ranges"] = bad_ranges;
    out["guard_ok"] = guard_ok;
    out["beyond_cache"] = n_total * 16 >= kScrubBeyondCacheBytes;
    out["scrub_ms"] = scrub_ms;
    out["wall_ms"] = wall_ms;  // allocation, poison and guard check included
    out["steps"] = steps;
    out["poison_byte"] = hbmpattern::kPoisonByte;
    out["ok"] = rep.mismatches == 0 && guard_ok;
    if (return_data) {
        py::list data;  // per slab, guard bands included
        for (const ScrubSlab &s : slabs) {
            std::vector<char> all(2 * guard_bytes + s.n * 16);
            HIP_CHECK(hipMemcpy(all.data(), s.alloc, all.size(),
                                hipMemcpyDeviceToHost));
            data.append(py::bytes(all.data(), all.size()));
        }
        out["data"] = data;
    }
    return out;
}

// hbmmarch::expected for elements start..start+count-1 as bytes: no HIP
// call, works without a GPU.
py::bytes hbm_march_reference(const std::string &pattern,
                              unsigned long long seed, int step,
                              unsigned long long start, long long count) {
    const int p = march_pattern_by_name(pattern);
    if (step < 0 || step >= hbmmarch::kSteps)
        throw std::invalid_argument("step must be in 0..3");
    if (count < 0 || count > kMarchReferenceMaxCount)
        throw std::invalid_argument("count must be in 0..2^24");
    std::vector<hbmmarch::Element> out((size_t)count);
    for (long long k = 0; k < count; ++k)
        out[(size_t)k] = hbmmarch::expected(p, seed, step, start + k);
    return py::bytes((const char *)out.data(), out.size() * sizeof(out[0]));
}

// ---------------- LDS sweep ----------------

constexpr int kLdsSweepMaxLaunches = 4;
constexpr long long kLdsSweepMaxArgBytes = 1ll << 30;

int lds_path_by_name(const std::string &name) {
    for (int p = 0; p < ldsmarch::kPaths; ++p)
        if (name == ldsmarch::kPathNames[p]) return p;
    throw std::invalid_argument("unknown path '" + name +
                                "' (b128, b64, b32, dma, tr16)");
}

const char *const kLdsCorruptForm =
    "corrupt must be (block, path, pattern, after_step, 'flip', element, word, "
    "bit) or (block, path, pattern, after_step, 'alias', element, distance)";

struct LdsCorruptSpec {
    bool given = false;
    long long block = -1, step = 0, element = 0, word = 0, bit = 0, distance = 0;
    int path = 0, pattern = 0, kind = kLdsNone;
};

// The part of the corruption that depends on the sizes, which with
// lds_bytes = 0 or blocks = 0 are known only once the card is.
void check_lds_corruption(const LdsCorruptSpec &c, long long lds_bytes,
                          long long blocks) {
    if (!c.given) return;
    if (blocks && c.block >= blocks)
        throw std::invalid_argument("corrupt: block must be in 0..blocks-1");
    if (!lds_bytes) return;
    const long long n = ldsmarch::covered_bytes(c.path, (uint32_t)lds_bytes) / 16;
    if (c.element >= n)
        throw std::invalid_argument(
            "corrupt: element must be inside the bytes the path covers");
    if (c.kind == kLdsAlias &&
        (c.element + c.distance < 0 || c.element + c.distance >= n))
        throw std::invalid_argument(
            "alias: element + distance must be another element that the path covers");
}

py::dict lds_first_failure(const ldsmarch::First &f, uint32_t expected) {
    py::dict first;
    first["path"] = f.path < (uint32_t)ldsmarch::kPaths
                        ? ldsmarch::kPathNames[f.path] : "?";
    first["pattern"] = hbmmarch::kPatternNames[f.pattern];
    first["step"] = f.step;
    first["element"] = f.element;
    first["word"] = f.word;
    first["got"] = f.got;
    first["expected"] = expected;
    return first;
}

// March test of a CU's LDS through every route into and out of it
// (lds_sweep_kernel, lds_march.h), one block of lds_bytes per CU, with the
// place each block ran read from the hardware id registers.  Where the
// records show a CU that hosted no block, launch again with doubled reps,
// at most kLdsSweepMaxLaunches in all, accumulating coverage and failures
// (with fewer blocks than CUs there is nothing to wait for: one launch).
// lds_bytes = 0: sharedMemPerBlock; blocks = 0: one per CU; reps = 0: the
// default.  patterns names the patterns of the three march paths; dma is
// defined with `random` and tr16 with `address`.
// corrupt = (block, path, pattern, after_step, "flip", element, word, bit)
//        or (block, path, pattern, after_step, "alias", element, distance)
// makes thread 0 of that block damage its own LDS once per launch.
py::dict lds_sweep(int device, long long lds_bytes, long long blocks,
                   long long reps, py::object paths, py::object patterns,
                   unsigned long long seed, py::object corrupt) {
    if (lds_bytes < 0 || lds_bytes % 16 || lds_bytes > kLdsSweepMaxArgBytes)
        throw std::invalid_argument(
            "lds_bytes must be a multiple of 16 in 16..2^30 (0 = the card's "
            "sharedMemPerBlock)");
    if (blocks < 0 || blocks > 65536)
        throw std::invalid_argument("blocks must be in 1..65536 (0 = cu_count)");
    if (reps < 0 || reps > 65536)
        throw std::invalid_argument("reps must be in 0..65536 (0 = default)");
    if (reps == 0) reps = ldsmarch::kDefaultReps;

    bool path_on[ldsmarch::kPaths] = {};
    if (paths.is_none())
        for (bool &on : path_on) on = true;
    else
        for (int p : names_to_indices(paths, "path", lds_path_by_name))
            path_on[p] = true;
    uint32_t march_mask = 0;  // 0: each path's default
    if (!patterns.is_none())
        for (int p : names_to_indices(patterns, "pattern", march_pattern_by_name))
            march_mask |= ldsmarch::pattern_bit(p);
    uint32_t mask_of[ldsmarch::kPaths];
    for (int p = 0; p < ldsmarch::kPaths; ++p)
        mask_of[p] = !path_on[p] ? 0
                     : march_mask && !ldsmarch::pattern_is_fixed(p)
                         ? march_mask
                         : ldsmarch::default_patterns(p);

    LdsCorruptSpec c;
    if (!corrupt.is_none()) try {
        py::sequence seq = corrupt.cast<py::sequence>();
        const size_t len = py::len(seq);
        if (len != 7 && len != 8) throw std::invalid_argument(kLdsCorruptForm);
        c.given = true;
        c.block = seq[0].cast<long long>();
        c.path = lds_path_by_name(seq[1].cast<std::string>());
        c.pattern = march_pattern_by_name(seq[2].cast<std::string>());
        c.step = seq[3].cast<long long>();
        const std::string what = seq[4].cast<std::string>();
        c.element = seq[5].cast<long long>();
        if (c.block < 0)
            throw std::invalid_argument("corrupt: block must be in 0..blocks-1");
        if (!(mask_of[c.path] >> c.pattern & 1))
            throw std::invalid_argument(
                "corrupt: that pattern does not run on that path");
        if (c.step < 0 || c.step > 3 ||
            !ldsmarch::step_is_followed_by_read(c.path, (int)c.step))
            throw std::invalid_argument(
                "corrupt: after_step must be a step of the path that a reading "
                "step follows");
        if (c.element < 0 || c.element >= kLdsSweepMaxArgBytes / 16)
            throw std::invalid_argument(
                "corrupt: element must be inside the bytes the path covers");
        if (what == "flip" && len == 8) {
            c.kind = kLdsFlip;
            c.word = seq[6].cast<long long>();
            c.bit = seq[7].cast<long long>();
            if (c.word < 0 || c.word > 3 || c.bit < 0 || c.bit > 31)
                throw std::invalid_argument("flip: word in 0..3, bit in 0..31");
        } else if (what == "alias" && len == 7) {
            c.kind = kLdsAlias;
            c.distance = seq[6].cast<long long>();
            if (c.distance == 0 || c.distance <= -kLdsSweepMaxArgBytes / 16 ||
                c.distance >= kLdsSweepMaxArgBytes / 16)
                throw std::invalid_argument(
                    "alias: element + distance must be another element that "
                    "the path covers");
        } else {
            throw std::invalid_argument(kLdsCorruptForm);
        }
        check_lds_corruption(c, lds_bytes, blocks);
    } catch (const py::cast_error &) {
        throw std::invalid_argument(kLdsCorruptForm);
    } catch (const py::type_error &) {
        throw std::invalid_argument(kLdsCorruptForm);
    }

    HIP_CHECK(hipSetDevice(device));
    hipDeviceProp_t props;
    HIP_CHECK(hipGetDeviceProperties(&props, device));
    const int cu_count = props.multiProcessorCount;
    const long long lds_bytes_per_cu = (long long)props.maxSharedMemoryPerMultiProcessor;
    if (lds_bytes == 0) lds_bytes = (long long)props.sharedMemPerBlock / 16 * 16;
    if (lds_bytes < 16 || (size_t)lds_bytes > props.sharedMemPerBlock ||
        lds_bytes > (long long)ldsmarch::kMaxLdsBytes)
        throw std::invalid_argument(
            "lds_bytes is above this GPU's sharedMemPerBlock of " +
            std::to_string(props.sharedMemPerBlock));
    if (blocks == 0) blocks = cu_count;
    check_lds_corruption(c, lds_bytes, blocks);

    const uint32_t elems = (uint32_t)(lds_bytes / 16);
    const uint32_t image_elems =
        ldsmarch::covered_bytes(ldsmarch::kDma, (uint32_t)lds_bytes) / 16;
    std::vector<hbmmarch::Element> image(std::max<uint32_t>(image_elems, 1));
    for (uint32_t e = 0; e < image_elems; ++e)
        image[e] = hbmmarch::pattern(hbmmarch::kRandom, seed, e);
    DeviceBuffer<u32x4> d_image(image.size());
    HIP_CHECK(hipMemcpy(d_image.get(), image.data(),
                        image.size() * sizeof(image[0]), hipMemcpyHostToDevice));

    LdsSweepParams a{};
    a.lds_bytes = (uint32_t)lds_bytes;
    for (int p = 0; p < ldsmarch::kPaths; ++p) a.patterns[p] = mask_of[p];
    a.seed = seed;
    a.image = d_image.get();
    a.c_block = c.given ? (int)c.block : -1;
    a.c_path = c.path;
    a.c_pattern = c.pattern;
    a.c_step = (int)c.step;
    a.c_kind = c.kind;
    a.c_element = (uint32_t)c.element;
    a.c_word = (uint32_t)c.word;
    a.c_bit = (uint32_t)c.bit;
    a.c_distance = (int)c.distance;

    const size_t n_rec = (size_t)blocks;
    DeviceBuffer<LdsBlockRecord> d_rec(n_rec);
    std::vector<LdsBlockRecord> h_rec(n_rec);
    LdsBlockRecord blank{};
    blank.first = ~0ull;
    const std::vector<LdsBlockRecord> blanks(n_rec, blank);

    using CuId = std::tuple<int, int, int, int>;  // xcc, se, sh, cu
    struct Bad {
        unsigned long long mismatches = 0;
        uint32_t bits[4] = {0, 0, 0, 0};
        unsigned long long first = ~0ull;
        uint32_t block = 0;
    };
    std::map<CuId, unsigned> blocks_of_cu;
    std::map<CuId, Bad> bad;
    py::list records;
    unsigned long long mismatches = 0;
    double sweep_ms = 0;
    int launches = 0;
    bool covered = false, consistent = true;
    EventPair ev;
    while (launches < kLdsSweepMaxLaunches && !covered) {
        if (launches) reps = std::min<long long>(reps * 2, 1 << 16);
        ++launches;
        a.reps = (int)reps;
        HIP_CHECK(hipMemcpy(d_rec.get(), blanks.data(),
                            n_rec * sizeof(LdsBlockRecord), hipMemcpyHostToDevice));
        sweep_ms += ev.time([&] {
            hipLaunchKernelGGL(lds_sweep_kernel, dim3((unsigned)blocks),
                               dim3(ldsmarch::kThreads), (size_t)lds_bytes, 0, a,
                               d_rec.get());
        });
        HIP_CHECK(hipMemcpy(h_rec.data(), d_rec.get(),
                            n_rec * sizeof(LdsBlockRecord), hipMemcpyDeviceToHost));

        for (size_t b = 0; b < n_rec; ++b) {
            const LdsBlockRecord &r = h_rec[b];
            py::list slots;
            for (uint32_t s = 0; s < std::min<uint32_t>(r.n_slots, kLdsSlots); ++s)
                slots.append(py::make_tuple(r.slots[s].meta, r.slots[s].element,
                                            r.slots[s].got, r.slots[s].expected));
            records.append(py::make_tuple(
                py::make_tuple(r.hw_id[0], r.hw_id[1], r.hw_id[2], r.hw_id[3]),
                py::make_tuple(r.xcc_id[0], r.xcc_id[1], r.xcc_id[2], r.xcc_id[3]),
                r.mismatches,
                py::make_tuple(r.bad_bits[0], r.bad_bits[1], r.bad_bits[2],
                               r.bad_bits[3]),
                r.first, slots));
            const SimdId w0 = decode_hw_id(r.hw_id[0], r.xcc_id[0]);
            const CuId cu{w0.xcc, w0.se, w0.sh, w0.cu};
            for (int w = 1; w < ldsmarch::kWaves; ++w) {
                const SimdId id = decode_hw_id(r.hw_id[w], r.xcc_id[w]);
                if (CuId{id.xcc, id.se, id.sh, id.cu} != cu) consistent = false;
            }
            ++blocks_of_cu[cu];
            mismatches += r.mismatches;
            if (r.mismatches) {
                Bad &x = bad[cu];
                x.mismatches += r.mismatches;
                for (int w = 0; w < 4; ++w) x.bits[w] |= r.bad_bits[w];
                if (r.first < x.first) {
                    x.first = r.first;
                    x.block = (uint32_t)b;
                }
            }
        }
        covered = (int)blocks_of_cu.size() >= cu_count;
        if (blocks < cu_count) break;  // can never reach every CU
    }

    py::list bad_list;
    for (const auto &kv : bad) {
        const ldsmarch::First f = ldsmarch::unpack_first(kv.second.first);
        const hbmmarch::Element p = hbmmarch::pattern(
            (int)f.pattern, seed,
            ldsmarch::pattern_index((int)f.path, kv.second.block, elems, f.element));
        py::dict b = std::apply(place_dict, kv.first);
        b["mismatches"] = kv.second.mismatches;
        b["bad_bits"] = py::make_tuple(kv.second.bits[0], kv.second.bits[1],
                                       kv.second.bits[2], kv.second.bits[3]);
        uint32_t expected = ldsmarch::word_of(
            ldsmarch::expected_of((int)f.path, p, (int)f.step), f.word);
        // tr16 reports one 16-bit value, at its place in the word
        if (f.path == ldsmarch::kTr16)
            expected &= f.half ? 0xFFFF0000u : 0x0000FFFFu;
        b["first"] = lds_first_failure(f, expected);
        bad_list.append(b);
    }
    // a CU that no wave ran on has no id to report: a count
    const int uncovered = std::max(0, cu_count - (int)blocks_of_cu.size());

    py::dict path_bytes, path_patterns;
    for (int p = 0; p < ldsmarch::kPaths; ++p) {
        if (!path_on[p]) continue;
        path_bytes[ldsmarch::kPathNames[p]] =
            ldsmarch::covered_bytes(p, (uint32_t)lds_bytes);
        py::list names;
        for (int q = 0; q < hbmmarch::kPatterns; ++q)
            if (mask_of[p] >> q & 1) names.append(hbmmarch::kPatternNames[q]);
        path_patterns[ldsmarch::kPathNames[p]] = names;
    }

    py::dict out;
    out["cu_count"] = cu_count;
    out["cus_covered"] = (int)blocks_of_cu.size();
    out["coverage_complete"] = covered && consistent &&
                               (int)blocks_of_cu.size() == cu_count &&
                               lds_bytes == lds_bytes_per_cu;
    out["placement_consistent"] = consistent;
    out["uncovered"] = uncovered;
    out["launches"] = launches;
    out["reps"] = reps;  // of the last launch
    out["blocks"] = blocks;
    out["lds_bytes"] = lds_bytes;
    out["lds_bytes_per_cu"] = lds_bytes_per_cu;
    out["paths"] = path_bytes;
    out["patterns"] = path_patterns;
    out["seed"] = seed;
    out["mismatches"] = mismatches;
    out["bad"] = bad_list;
    out["records"] = records;
    out["sweep_ms"] = sweep_ms;
    out["ok"] = mismatches == 0;
    return out;
}

// The sweep's schedule for the tests: no HIP call, works without a GPU.
py::dict lds_sweep_reference(long long lds_bytes) {
    if (lds_bytes < 16 || lds_bytes % 16 ||
        lds_bytes > (long long)ldsmarch::kMaxLdsBytes)
        throw std::invalid_argument("lds_bytes must be a multiple of 16 in 16..2^22");
    py::list paths;
    for (int p = 0; p < ldsmarch::kPaths; ++p) {
        py::dict d;
        d["name"] = ldsmarch::kPathNames[p];
        d["access_bytes"] = ldsmarch::access_bytes(p);
        d["steps"] = ldsmarch::path_steps(p);
        d["bytes"] = ldsmarch::covered_bytes(p, (uint32_t)lds_bytes);
        d["accesses"] = ldsmarch::accesses(p, (uint32_t)lds_bytes);
        py::list names, after;
        for (int q = 0; q < hbmmarch::kPatterns; ++q)
            if (ldsmarch::default_patterns(p) >> q & 1)
                names.append(hbmmarch::kPatternNames[q]);
        for (int s = 0; s < ldsmarch::path_steps(p); ++s)
            if (ldsmarch::step_is_followed_by_read(p, s)) after.append(s);
        d["default_patterns"] = names;
        d["corruptible_after"] = after;
        // [steps][items]: the thread that handles work item j in step s
        py::list threads;
        const uint32_t n = ldsmarch::accesses(p, (uint32_t)lds_bytes);
        for (int s = 0; s < ldsmarch::path_steps(p); ++s) {
            py::list row;
            for (uint32_t j = 0; j < n; ++j)
                row.append(ldsmarch::thread_of_item(p, s, n, j));
            threads.append(row);
        }
        d["thread_of_item"] = threads;
        paths.append(d);
    }
    py::list tr16;  // [256 threads][4]
    for (uint32_t t = 0; t < (uint32_t)ldsmarch::kThreads; ++t) {
        py::list row;
        for (uint32_t q = 0; q < 4; ++q) row.append(ldsmarch::tr16_source(t, q));
        tr16.append(row);
    }
    py::dict out;
    out["paths"] = paths;
    out["default_reps"] = ldsmarch::kDefaultReps;
    out["threads"] = ldsmarch::kThreads;
    out["tr16_source"] = tr16;
    out["tr16_round_bytes"] = ldsmarch::kTr16Bytes;
    out["dma_instruction_bytes"] = ldsmarch::kDmaBytes;
    out["poison_byte"] = hbmpattern::kPoisonByte;
    return out;
}

// (free, total) bytes of device memory, hipMemGetInfo.
py::tuple mem_info(int device) {
    HIP_CHECK(hipSetDevice(device));
    size_t free_bytes = 0, total = 0;
    HIP_CHECK(hipMemGetInfo(&free_bytes, &total));
    return py::make_tuple((uint64_t)free_bytes, (uint64_t)total);
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
    m.def("hbm_copy_check", &hbm_copy_check, py::arg("device") = 0,
          py::arg("n") = 1, py::arg("blocks") = 0, py::arg("threads") = 256,
          py::arg("guard") = 4096, py::arg("corrupt") = py::none(),
          py::arg("return_data") = false);
    m.def("lds_check", &lds_check, py::arg("device") = 0,
          py::arg("lds_bytes") = 128 * 1024, py::arg("blocks") = 1,
          py::arg("threads") = 256, py::arg("corrupt") = py::none());
    m.def("shared_mem_per_block", &shared_mem_per_block, py::arg("device") = 0);
    m.def("mfma_peak_check", &mfma_peak_check, py::arg("device") = 0,
          py::arg("iters") = 8192, py::arg("blocks") = 2);
    m.def("cu_sweep", &cu_sweep, py::arg("device") = 0, py::arg("reps") = 0,
          py::arg("inject") = py::none(), py::arg("pipe_set") = "base");
    m.def("cu_sweep_reference", &cu_sweep_reference,
          py::arg("pipe_set") = "base");
    m.def("mfma_raw", &mfma_raw, py::arg("device"), py::arg("pipe"),
          py::arg("a_frag"), py::arg("b_frag"), py::arg("scale_a") = py::none(),
          py::arg("scale_b") = py::none(),
          py::arg("sel") = std::pair<int, int>(0, 0));
    m.def("valu_sweep", &valu_sweep, py::arg("device") = 0, py::arg("reps") = 0,
          py::arg("inject") = py::none(), py::arg("op_set") = "fma");
    m.def("valu_sweep_reference", &valu_sweep_reference, py::arg("op_set") = "fma");
    m.def("valu_raw", &valu_raw, py::arg("device"), py::arg("op"), py::arg("a"),
          py::arg("b") = py::none(), py::arg("c") = py::none(),
          py::arg("old") = py::none());
    m.def("decode_hw_id", &decode_hw_id_py, py::arg("hw_id"),
          py::arg("xcc_id"));
    m.def("hbm_scrub", &hbm_scrub, py::arg("device") = 0,
          py::arg("bytes") = (long long)1 << 30,
          py::arg("slab_bytes") = kScrubDefaultSlabBytes,
          py::arg("guard") = 4096, py::arg("patterns") = py::none(),
          py::arg("seed") = 0x5EEDull, py::arg("corrupt") = py::none(),
          py::arg("max_records") = 64, py::arg("return_data") = false);
    m.def("hbm_march_reference", &hbm_march_reference, py::arg("pattern"),
          py::arg("seed"), py::arg("step"), py::arg("start"), py::arg("count"));
    m.def("lds_sweep", &lds_sweep, py::arg("device") = 0,
          py::arg("lds_bytes") = 0, py::arg("blocks") = 0, py::arg("reps") = 0,
          py::arg("paths") = py::none(), py::arg("patterns") = py::none(),
          py::arg("seed") = 0x5EEDull, py::arg("corrupt") = py::none());
    m.def("lds_sweep_reference", &lds_sweep_reference, py::arg("lds_bytes"));
    m.def("mem_info", &mem_info, py::arg("device") = 0);
}

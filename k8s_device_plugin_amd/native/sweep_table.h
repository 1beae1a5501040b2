// Known-answer tables of the CU sweep (cu_sweep_kernel in probe_kernels.h,
// cu_sweep / cu_sweep_reference in health_probe.hip).  Plain C++17, no HIP:
// the host builds the tables and the expected results, the kernel only
// reads them, and tests/native/sweep_table_check.cpp rebuilds them under
// the host sanitizers.
//
// Every operand is a small integer in [-2, 2], exact in bf16, f16, fp8
// (e4m3) and i8, and every sum stays below 2^9, so each product is exact in
// f32 / i32 and the device compares results bit for bit.
//
// Operands are defined by SLOT, not by a claimed k order: lane l supplies
// row (A) or column (B) l % M and the slots (l / M) * J + j, j = 0..J-1,
// where J is the number of elements a lane holds.  The hardware pairs
// element j of lane group h in A with the same (h, j) in B, so
// D = sum over slots of A[row][slot] * B[slot][col] whatever k each slot
// is; for bf16 32x32x16 the slot is the documented k = 8 (l >> 5) + j.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

namespace cusweep {

// 8 vectors would need 176 KiB of tables, more than the CU's 160 KiB of
// LDS; 6 need 132 KiB, which still leaves no room for a second sweep block.
constexpr int kTests = 6;
constexpr int kLanes = 64;
constexpr int kPipes = 6;

enum Elem { BF16, F16, FP8, I8 };

struct PipeDesc {
    const char *name;
    int M, N, K;
    Elem elem;
    int regs;         // result registers per lane = M * N / 64
    bool int_result;  // i32 accumulator, else f32
};

constexpr PipeDesc kPipeDesc[kPipes] = {
    {"bf16_16", 16, 16, 32, BF16, 4, false},
    {"bf16_32", 32, 32, 16, BF16, 16, false},
    {"f16_16", 16, 16, 32, F16, 4, false},
    {"fp8_16", 16, 16, 32, FP8, 4, false},
    {"i8_16", 16, 16, 64, I8, 4, true},
    {"mxfp8_16", 16, 16, 128, FP8, 4, false},  // E8M0 scale 127 on A and B
};

constexpr int elem_bytes(Elem e) { return e == BF16 || e == F16 ? 2 : 1; }
// elements of A (or B) that one lane holds
constexpr int lane_elems(int p) {
    return kPipeDesc[p].K / (kLanes / kPipeDesc[p].M);
}
constexpr int frag_bytes(int p) {
    return lane_elems(p) * elem_bytes(kPipeDesc[p].elem);
}

// Packed table, as the kernel stages it into LDS.  Per pipe and test:
// A fragments [64 lanes][frag_bytes], B fragments likewise, then the
// expected result bits [64 lanes][regs] as uint32.
constexpr int test_bytes(int p) {
    return kLanes * (2 * frag_bytes(p) + 4 * kPipeDesc[p].regs);
}
constexpr int pipe_offset(int p) {
    int off = 0;
    for (int q = 0; q < p; ++q) off += kTests * test_bytes(q);
    return off;
}
constexpr int test_offset(int p, int t) {
    return pipe_offset(p) + t * test_bytes(p);
}
constexpr int kTableBytes = pipe_offset(kPipes);
static_assert(kTableBytes % 16 == 0, "the kernel stages 16 bytes a thread");
static_assert(kTableBytes > 80 * 1024 && kTableBytes <= 160 * 1024,
              "one sweep block per CU: more than half of its 160 KiB LDS");

// which: 0 = A (rc is the row), 1 = B (rc is the column).  A multiplicative
// hash with two xor-shifts; a periodic pattern such as (3 i + 5 s) % 5
// repeats rows, and a repeated row would let a swapped lane go unseen.
constexpr int operand_value(int t, int which, int rc, int slot) {
    uint32_t x = (uint32_t)(((t * 2 + which) * 32 + rc) * 128 + slot);
    x *= 2654435761u;
    x ^= x >> 15;
    x *= 2246822519u;
    x ^= x >> 13;
    return (int)(x % 5u) - 2;
}

// encodings of -2, -1, 0, 1, 2
constexpr uint16_t kBf16Bits[5] = {0xC000, 0xBF80, 0x0000, 0x3F80, 0x4000};
constexpr uint16_t kF16Bits[5] = {0xC000, 0xBC00, 0x0000, 0x3C00, 0x4000};
constexpr uint8_t kFp8Bits[5] = {0xC0, 0xB8, 0x00, 0x38, 0x40};  // OCP e4m3
constexpr uint8_t kI8Bits[5] = {0xFE, 0xFF, 0x00, 0x01, 0x02};

// C/D lane map, the same for every dtype: which row of D lane l holds in
// result register reg (its column is l % N).
constexpr int result_row(int p, int lane, int reg) {
    return kPipeDesc[p].M == 16
               ? 4 * (lane >> 4) + reg
               : (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
}

struct TestVector {
    std::vector<int> A;               // M x K, row-major, indexed by slot
    std::vector<int> B;               // K x N, row-major
    std::vector<int> D;               // M x N = A * B
    std::vector<uint8_t> a_frag;      // [64][frag_bytes]
    std::vector<uint8_t> b_frag;      // [64][frag_bytes]
    std::vector<uint32_t> expected;   // [64][regs], result register bits
};

inline void pack_elem(Elem e, int v, uint8_t *dst) {
    const int i = v + 2;
    if (e == BF16 || e == F16) {
        const uint16_t bits = e == BF16 ? kBf16Bits[i] : kF16Bits[i];
        std::memcpy(dst, &bits, 2);  // little endian, as the GPU reads it
    } else {
        *dst = e == FP8 ? kFp8Bits[i] : kI8Bits[i];
    }
}

inline TestVector make_test(int p, int t) {
    const PipeDesc &d = kPipeDesc[p];
    const int J = lane_elems(p), eb = elem_bytes(d.elem), fb = frag_bytes(p);
    TestVector v;
    v.A.resize((size_t)d.M * d.K);
    v.B.resize((size_t)d.K * d.N);
    v.D.assign((size_t)d.M * d.N, 0);
    for (int i = 0; i < d.M; ++i)
        for (int s = 0; s < d.K; ++s)
            v.A[(size_t)i * d.K + s] = operand_value(t, 0, i, s);
    for (int s = 0; s < d.K; ++s)
        for (int j = 0; j < d.N; ++j)
            v.B[(size_t)s * d.N + j] = operand_value(t, 1, j, s);
    for (int i = 0; i < d.M; ++i)
        for (int j = 0; j < d.N; ++j) {
            int sum = 0;
            for (int s = 0; s < d.K; ++s)
                sum += v.A[(size_t)i * d.K + s] * v.B[(size_t)s * d.N + j];
            v.D[(size_t)i * d.N + j] = sum;
        }

    v.a_frag.resize((size_t)kLanes * fb);
    v.b_frag.resize((size_t)kLanes * fb);
    v.expected.resize((size_t)kLanes * d.regs);
    for (int l = 0; l < kLanes; ++l) {
        const int rc = l % d.M, group = l / d.M;
        for (int j = 0; j < J; ++j) {
            const int s = group * J + j;
            pack_elem(d.elem, v.A[(size_t)rc * d.K + s],
                      &v.a_frag[(size_t)l * fb + (size_t)j * eb]);
            pack_elem(d.elem, v.B[(size_t)s * d.N + rc],
                      &v.b_frag[(size_t)l * fb + (size_t)j * eb]);
        }
        for (int r = 0; r < d.regs; ++r) {
            const int val = v.D[(size_t)result_row(p, l, r) * d.N + l % d.N];
            uint32_t bits;
            if (d.int_result) {
                bits = (uint32_t)val;
            } else {
                const float f = (float)val;
                std::memcpy(&bits, &f, 4);
            }
            v.expected[(size_t)l * d.regs + r] = bits;
        }
    }
    return v;
}

// the kTableBytes blob the kernel copies into LDS
inline std::vector<uint8_t> build_table() {
    std::vector<uint8_t> blob((size_t)kTableBytes);
    for (int p = 0; p < kPipes; ++p)
        for (int t = 0; t < kTests; ++t) {
            const TestVector v = make_test(p, t);
            uint8_t *dst = blob.data() + test_offset(p, t);
            std::memcpy(dst, v.a_frag.data(), v.a_frag.size());
            dst += v.a_frag.size();
            std::memcpy(dst, v.b_frag.data(), v.b_frag.size());
            dst += v.b_frag.size();
            std::memcpy(dst, v.expected.data(), v.expected.size() * 4);
        }
    return blob;
}

}  // namespace cusweep

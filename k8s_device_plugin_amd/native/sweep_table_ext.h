// Known-answer tables of the CU sweep's two extra pipe sets (cu_sweep with
// pipe_set "mx" / "wide", mfma_raw and cu_sweep_reference in
// health_probe.hip).  Plain C++17, no HIP: the host builds the tables, the
// kernel only reads them, and tests/native/sweep_table_ext_check.cpp
// rebuilds them under the host sanitizers.  The base set stays in
// sweep_table.h, byte for byte; the accessors at the end of this header
// cover all three sets so that kernel and host are written once.
//
// Set mx:   block-scaled v_mfma_scale_f32_*_f8f6f4 with LIVE E8M0 scales:
//           every lane owns one 32-element MX block of A and one of B, its
//           two scale words hold the block's true scale in the byte that
//           the test's op_sel pair selects and decoys in the other three.
// Set wide: the unscaled paths the base set leaves out (bf8, the 32x32
//           shapes of f16 / fp8 / i8, f64 and f32-input).
//
// The slot rule of sweep_table.h carries over: lane l supplies row (A) or
// column (B) l % M and the slots (l / M) * J + j, and element j of lane
// group h in A meets the same (h, j) in B.  J = 32 for every mx pipe (one
// lane = one MX block; the fp8 side of fp8 x fp4 is the exception, see
// slot_of), J = 1 for f64 and f32-input.
//
// Every operand is k * 2^-shift of its format with an integer k (its
// "units"), so every product, times the block scales, is an integer number
// of one unit u per pipe, and sum |a b| scale / u stays below 2^23 (f32
// result), 2^31 (i32) or 2^52 (f64): every partial sum in any order is
// exact and the device compares bit for bit.
#pragma once

#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "sweep_table.h"

namespace cusweepx {

using cusweep::kLanes;

enum Set { kBase = 0, kMx = 1, kWide = 2, kSets = 3 };
constexpr const char *kSetName[kSets] = {"base", "mx", "wide"};

constexpr int kTests = 6;  // per pipe, in both extra sets

enum Fmt { FP4, FP6, BF6, FP8, BF8, F16, F32, F64, I8 };
enum Result { RF32, RI32, RF64 };

struct FmtDesc {
    const char *name;
    int bits, E, M, bias;  // sign, E exponent bits, M mantissa bits
    int shift;             // the tables use multiples of 2^-shift
    int code;              // cbsz / blgp of the f8f6f4 instruction, or -1
};

constexpr FmtDesc kFmt[] = {
    {"fp4_e2m1", 4, 2, 1, 1, 1, 4},
    {"fp6_e2m3", 6, 2, 3, 1, 3, 2},
    {"bf6_e3m2", 6, 3, 2, 3, 3, 3},
    {"fp8_e4m3", 8, 4, 3, 7, 3, 0},
    {"bf8_e5m2", 8, 5, 2, 15, 2, 1},
    {"f16", 16, 5, 10, 15, 6, -1},
    {"f32", 32, 8, 23, 127, 5, -1},
    {"f64", 64, 11, 52, 1023, 0, -1},
    {"i8", 8, 0, 0, 0, 0, -1},  // two's complement
};

struct PipeDesc {
    const char *name;
    int M, N, K;
    Fmt a, b;
    Result result;
};

constexpr int kMxPipes = 5;
constexpr PipeDesc kMxDesc[kMxPipes] = {
    {"mxfp4_16", 16, 16, 128, FP4, FP4, RF32},
    {"mxfp4_32", 32, 32, 64, FP4, FP4, RF32},
    {"mxfp6_16", 16, 16, 128, FP6, FP6, RF32},
    {"mxbf6_16", 16, 16, 128, BF6, BF6, RF32},
    {"mxfp8xfp4_16", 16, 16, 128, FP8, FP4, RF32},  // activations x weights
};

constexpr int kWidePipes = 6;
constexpr PipeDesc kWideDesc[kWidePipes] = {
    {"bf8_16", 16, 16, 32, BF8, BF8, RF32},
    {"f16_32", 32, 32, 16, F16, F16, RF32},
    {"fp8_32", 32, 32, 16, FP8, FP8, RF32},
    {"i8_32", 32, 32, 32, I8, I8, RI32},
    {"f64_16", 16, 16, 4, F64, F64, RF64},
    {"f32_16", 16, 16, 4, F32, F32, RF32},
};

// ---- the extra sets' own geometry (set is kMx or kWide) ----

constexpr const PipeDesc &desc(int set, int p) {
    return set == kMx ? kMxDesc[p] : kWideDesc[p];
}
constexpr bool scaled(int set) { return set == kMx; }
// elements of A (or B) that one lane holds
constexpr int ext_lane_elems(int set, int p) {
    return desc(set, p).K / (kLanes / desc(set, p).M);
}
constexpr int ext_frag_bytes(int set, int p, int which) {
    return ext_lane_elems(set, p) *
           kFmt[which ? desc(set, p).b : desc(set, p).a].bits / 8;
}
// results per lane, and the 32-bit result registers that hold them
constexpr int ext_results(int set, int p) {
    return desc(set, p).M * desc(set, p).N / kLanes;
}
constexpr int ext_regs(int set, int p) {
    return ext_results(set, p) * (desc(set, p).result == RF64 ? 2 : 1);
}

// The op_sel pair of test t of an mx pipe: the byte of the scale word that
// the instruction reads, for A and for B.  Over the 6 tests each of the four
// selects is used on each side, and never the same one on both sides.
constexpr int sel_a(int t) { return t % 4; }
constexpr int sel_b(int t) { return (t + 1) % 4; }
// which byte of the 32-bit scale word a select value reads
constexpr int byte_of_sel(int sel) { return sel; }

// The slot that element j of lane group `group` holds.  Everywhere but one
// case it is the slot rule's group * J + j.  The case, found with one-hot
// operands on MI355X: the 8 registers of an 8-bit operand of the scaled
// 16x16x128 instruction are two halves, k = 16 group + j for j < 16 and
// k = 64 + 16 group + (j - 16) above, while a 4- or 6-bit operand holds
// k = 32 group + j.  Against an operand of the same width that changes
// nothing (both sides hold the same k in the same place), but fp8 x fp4
// pairs by k.  The block scales follow k as well: the scale word of lane
// group g belongs to the MX block k = 32 g .. 32 g + 31 of that row or
// column, which for fp4 / fp6 is the lane's own 32 elements and for the
// 8-bit side of a mixed pipe is not.  For the mixed pipe the tables
// therefore index slots by k.
constexpr int slot_of(int set, int p, int which, int group, int j) {
    const PipeDesc &d = desc(set, p);
    const bool split = scaled(set) && d.a != d.b &&
                       kFmt[which ? d.b : d.a].bits == 8 && d.M == 16;
    return !split   ? group * ext_lane_elems(set, p) + j
           : j < 16 ? 16 * group + j
                    : 64 + 16 * group + (j - 16);
}

// C/D lane map: the row of D that result `res` of lane l is (its column is
// l % N).  f64 has a map of its own; everything else follows the base sets.
constexpr int ext_result_row(int set, int p, int lane, int res) {
    return desc(set, p).result == RF64 ? (lane >> 4) + 4 * res
           : desc(set, p).M == 16      ? 4 * (lane >> 4) + res
                                  : (res & 3) + 8 * (res >> 2) + 4 * (lane >> 5);
}

// ---- all three sets, for the kernel and the host ----

constexpr int n_pipes(int set) {
    return set == kBase ? cusweep::kPipes : set == kMx ? kMxPipes : kWidePipes;
}
constexpr int n_tests(int set) { return set == kBase ? cusweep::kTests : kTests; }
constexpr const char *pipe_name(int set, int p) {
    return set == kBase ? cusweep::kPipeDesc[p].name : desc(set, p).name;
}
constexpr int frag_bytes(int set, int p, int which) {
    return set == kBase ? cusweep::frag_bytes(p) : ext_frag_bytes(set, p, which);
}
constexpr int regs(int set, int p) {
    return set == kBase ? cusweep::kPipeDesc[p].regs : ext_regs(set, p);
}
// Packed table, as the kernel stages it into LDS.  Per pipe and test: the A
// fragments [64][frag_bytes A], the B fragments [64][frag_bytes B], for mx
// the A scale words [64] and the B scale words [64], then the expected
// result registers [64][regs].  The matrix instruction reads 8 registers of
// an f8f6f4 operand whatever its format, so the kernel loads 32 bytes where
// a lane's fp4 / fp6 fragment has 16 / 24: the pad is whatever follows in
// the table (the next lane's fragment, the next section), never zeros, and
// nothing may depend on it.
constexpr int test_bytes(int set, int p) {
    return kLanes * (frag_bytes(set, p, 0) + frag_bytes(set, p, 1) +
                     (scaled(set) ? 8 : 0) + 4 * regs(set, p));
}
constexpr int test_offset(int set, int p, int t) {
    int off = 0;
    for (int q = 0; q < p; ++q) off += n_tests(set) * test_bytes(set, q);
    return t ? off + t * test_bytes(set, p) : off;  // p may be n_pipes(set)
}
constexpr int table_bytes(int set) { return test_offset(set, n_pipes(set), 0); }

static_assert(table_bytes(kBase) == cusweep::kTableBytes &&
                  test_offset(kBase, 3, 2) == cusweep::test_offset(3, 2),
              "the base set is sweep_table.h's");
static_assert(table_bytes(kMx) % 16 == 0 && table_bytes(kWide) % 16 == 0,
              "the kernel stages 16 bytes a thread");
static_assert(table_bytes(kMx) > 80 * 1024 && table_bytes(kMx) <= 160 * 1024 &&
                  table_bytes(kWide) > 80 * 1024 &&
                  table_bytes(kWide) <= 160 * 1024,
              "each set's table fits one block's LDS and fills over half of it");

// Dynamic LDS of a sweep block: over half of the CU's 160 KiB whatever the
// table's size, so two sweep blocks cannot share a CU.
constexpr int lds_bytes(int set) {
    return set == kBase                          ? cusweep::kTableBytes
           : table_bytes(set) > 80 * 1024 + 16 ? table_bytes(set)
                                               : 80 * 1024 + 16;
}

// ---- operand values ----

constexpr uint32_t hash32(uint32_t x) {
    x *= 2654435761u;
    x ^= x >> 15;
    x *= 2246822519u;
    x ^= x >> 13;
    x *= 3266489917u;
    x ^= x >> 16;
    return x;
}

// which: 0 = A (rc is the row), 1 = B (rc is the column)
constexpr uint32_t operand_hash(int set, int p, int t, int which, int rc, int slot) {
    return hash32((uint32_t)((((set * 8 + p) * 8 + t) * 2 + which) * 32 + rc) * 128u +
                  (uint32_t)slot);
}

// value * 2^shift of an element code, from the format's definition; every
// code the tables use gives an integer
inline int64_t decode_units(Fmt f, uint64_t code) {
    const FmtDesc &d = kFmt[f];
    if (f == I8) return (int8_t)(uint8_t)code;
    const bool neg = code >> (d.bits - 1) & 1;
    const int e = (int)(code >> d.M & ((1u << d.E) - 1));
    const uint64_t m = code & ((1ull << d.M) - 1);
    const uint64_t mant = e ? (1ull << d.M | m) : m;  // e == 0: subnormal
    const int exp2 = (e ? e : 1) - d.bias - d.M + d.shift;
    if (mant == 0) return 0;  // either zero
    uint64_t v;
    if (exp2 >= 0) {
        v = mant << exp2;
    } else {
        assert(-exp2 < 64 && (mant & ((1ull << -exp2) - 1)) == 0);
        v = mant >> -exp2;
    }
    return neg ? -(int64_t)v : (int64_t)v;
}

// the code of k * 2^-shift in f16 / f32 / f64 (a normal number)
inline uint64_t encode_units(Fmt f, int64_t k) {
    const FmtDesc &d = kFmt[f];
    if (k == 0) return 0;
    const uint64_t a = (uint64_t)(k < 0 ? -k : k);
    const int hb = 63 - __builtin_clzll(a);
    assert(hb <= d.M);
    const uint64_t e = (uint64_t)(hb - d.shift + d.bias);
    const uint64_t m = (a << (d.M - hb)) & ((1ull << d.M) - 1);
    return (uint64_t)(k < 0) << (d.bits - 1) | e << d.M | m;
}

// The element code of one slot.  Per format the codes are those whose
// value is a multiple of 2^-shift and small enough for the bound above:
//   fp4 e2m1  all 16 codes (0 .. 6, unit 1/2)
//   fp6 e2m3  all 64 codes (0 .. 7.5, unit 1/8)
//   bf6 e3m2  0 and exponents 2..5 (0.5 .. 7, unit 1/8), both signs
//   fp8 e4m3  0 and exponents 7..10 (1 .. 15, unit 1/8), both signs
//   bf8 e5m2  0 and exponents 15..18 (1 .. 14, unit 1/4), both signs
//   i8        all 256 codes
//   f16       k / 64, |k| < 2048 on one side and |k| <= 7 on the other
//   f32       k / 32, |k| < 2048 on one side and |k| < 512 on the other
//   f64       integers, |k| < 2^24, on both sides
// `narrow` is the side with the small range (f16 and f32: it alternates
// with the test, so both operands see every bit).  The integers k have a
// uniformly drawn bit length, so every exponent in range is as likely as
// any other and zero, one and the largest values all occur.
constexpr int64_t signed_of_bit_length(uint32_t h, int max_bits) {
    const int n = (int)(h % (uint32_t)(max_bits + 1));
    if (n == 0) return 0;
    const int64_t k = (int64_t)1 << (n - 1) | (int64_t)(h >> 8 & ((1u << (n - 1)) - 1));
    return h >> 7 & 1 ? -k : k;
}

inline uint64_t pick_code(Fmt f, bool narrow, uint32_t h) {
    const uint64_t sign = h >> 16 & 1;
    switch (f) {
    case FP4: return h & 15;
    case FP6: return h & 63;
    case BF6: { const uint32_t i = h % 17; return i ? sign << 5 | (7 + i) : 0; }
    case FP8: { const uint32_t i = h % 33; return i ? sign << 7 | (0x37 + i) : 0; }
    case BF8: { const uint32_t i = h % 17; return i ? sign << 7 | (0x3B + i) : 0; }
    case I8: return h & 255;
    case F16: return encode_units(f, signed_of_bit_length(h, narrow ? 3 : 11));
    case F32: return encode_units(f, signed_of_bit_length(h, narrow ? 9 : 11));
    case F64: return encode_units(f, signed_of_bit_length(h, 24));
    }
    return 0;
}

// ---- block scales (mx) ----

constexpr int kScaleLo = 126, kScaleHi = 128;  // true E8M0 scales: 1/2, 1, 2

// the true scale of the MX block (t, side, row or column, lane group)
constexpr int true_scale(int p, int t, int which, int rc, int group) {
    return kScaleLo +
           (int)(hash32(0x5CA1E000u + (uint32_t)((((p * 8 + t) * 2 + which) * 32 + rc) * 4 + group)) %
                 (uint32_t)(kScaleHi - kScaleLo + 1));
}

// The lane's scale word: the true scale in the byte its test's select
// reads, decoys 8 .. 15 away from it in the other three, so that a wrong
// byte select is off by a factor of at least 256.
constexpr uint32_t scale_word(int p, int t, int which, int rc, int group) {
    const int truth = true_scale(p, t, which, rc, group);
    const int live = byte_of_sel(which ? sel_b(t) : sel_a(t));
    const uint32_t h =
        hash32(0xDEC01000u + (uint32_t)((((p * 8 + t) * 2 + which) * 32 + rc) * 4 + group));
    uint32_t word = 0;
    for (int byte = 0; byte < 4; ++byte) {
        const int off = 8 + (int)(h >> (8 * byte) & 7);
        const int v = byte == live ? truth : (h >> (8 * byte + 3) & 1) ? truth + off : truth - off;
        word |= (uint32_t)v << (8 * byte);
    }
    return word;
}

// ---- one test vector ----

struct TestVector {
    std::vector<int64_t> A;           // M x K units of 2^-shift(a), by slot
    std::vector<int64_t> B;           // K x N units of 2^-shift(b)
    std::vector<int64_t> D;           // M x N units of 2^-unit_shift
    int unit_shift = 0;               // D = units * 2^-unit_shift
    int64_t abs_sum_max = 0;          // max over D of sum |a b| scale / u
    std::vector<uint8_t> a_frag;      // [64][frag_bytes A]
    std::vector<uint8_t> b_frag;      // [64][frag_bytes B]
    std::vector<uint32_t> scale_a;    // [64], mx only
    std::vector<uint32_t> scale_b;
    std::vector<uint32_t> expected;   // [64][regs], result register bits
};

// element j of a lane's fragment: bits [j * nbits, (j + 1) * nbits) of the
// fragment read as one little-endian bit string (fp4: low nibble first)
inline void put_bits(uint8_t *frag, int j, int nbits, uint64_t code) {
    for (int b = 0; b < nbits; ++b) {
        const int pos = j * nbits + b;
        if (code >> b & 1) frag[pos >> 3] |= (uint8_t)(1u << (pos & 7));
    }
}
inline uint64_t get_bits(const uint8_t *frag, int j, int nbits) {
    uint64_t code = 0;
    for (int b = 0; b < nbits; ++b) {
        const int pos = j * nbits + b;
        code |= (uint64_t)(frag[pos >> 3] >> (pos & 7) & 1) << b;
    }
    return code;
}

// result register bits of `units * 2^-unit_shift`: regs words at dst
inline void result_bits(Result r, int64_t units, int unit_shift, uint32_t *dst) {
    if (r == RI32) {
        dst[0] = (uint32_t)(int32_t)units;
    } else if (r == RF32) {
        const float f = (float)std::ldexp((double)units, -unit_shift);
        std::memcpy(dst, &f, 4);
    } else {
        const double f = std::ldexp((double)units, -unit_shift);
        std::memcpy(dst, &f, 8);  // low word first
    }
}

inline TestVector make_test(int set, int p, int t) {
    const PipeDesc &d = desc(set, p);
    const int J = ext_lane_elems(set, p), groups = kLanes / d.M;
    const int fa = ext_frag_bytes(set, p, 0), fb = ext_frag_bytes(set, p, 1);
    const int results = ext_results(set, p), words = ext_regs(set, p) / results;
    const bool a_narrow = t % 2 == 1;
    TestVector v;
    v.A.resize((size_t)d.M * d.K);
    v.B.resize((size_t)d.K * d.N);
    v.a_frag.assign((size_t)kLanes * fa, 0);
    v.b_frag.assign((size_t)kLanes * fb, 0);
    for (int l = 0; l < kLanes; ++l) {
        const int rc = l % d.M, group = l / d.M;
        for (int j = 0; j < J; ++j) {
            const int sa = slot_of(set, p, 0, group, j), sb = slot_of(set, p, 1, group, j);
            const uint64_t ca = pick_code(d.a, a_narrow, operand_hash(set, p, t, 0, rc, sa));
            const uint64_t cb = pick_code(d.b, !a_narrow, operand_hash(set, p, t, 1, rc, sb));
            put_bits(&v.a_frag[(size_t)l * fa], j, kFmt[d.a].bits, ca);
            put_bits(&v.b_frag[(size_t)l * fb], j, kFmt[d.b].bits, cb);
            v.A[(size_t)rc * d.K + sa] = decode_units(d.a, ca);
            v.B[(size_t)sb * d.N + rc] = decode_units(d.b, cb);
        }
        if (scaled(set)) {
            v.scale_a.push_back(scale_word(p, t, 0, rc, group));
            v.scale_b.push_back(scale_word(p, t, 1, rc, group));
        }
    }
    // block scales as integer weights 2^(sa + sb - 2 kScaleLo); the unit
    // absorbs 2^(2 kScaleLo - 254)
    v.unit_shift = kFmt[d.a].shift + kFmt[d.b].shift +
                   (scaled(set) ? 254 - 2 * kScaleLo : 0);
    v.D.assign((size_t)d.M * d.N, 0);
    for (int i = 0; i < d.M; ++i)
        for (int j = 0; j < d.N; ++j) {
            int64_t sum = 0, abs_sum = 0;
            for (int g = 0; g < groups; ++g) {
                const int w = scaled(set) ? true_scale(p, t, 0, i, g) +
                                                true_scale(p, t, 1, j, g) - 2 * kScaleLo
                                          : 0;
                for (int e = 0; e < J; ++e) {
                    const int s = g * J + e;
                    const int64_t prod =
                        v.A[(size_t)i * d.K + s] * v.B[(size_t)s * d.N + j] * ((int64_t)1 << w);
                    sum += prod;
                    abs_sum += prod < 0 ? -prod : prod;
                }
            }
            v.D[(size_t)i * d.N + j] = sum;
            if (abs_sum > v.abs_sum_max) v.abs_sum_max = abs_sum;
        }
    v.expected.assign((size_t)kLanes * ext_regs(set, p), 0);
    for (int l = 0; l < kLanes; ++l)
        for (int r = 0; r < results; ++r)
            result_bits(d.result,
                        v.D[(size_t)ext_result_row(set, p, l, r) * d.N + l % d.N],
                        v.unit_shift,
                        &v.expected[(size_t)l * ext_regs(set, p) + (size_t)r * words]);
    return v;
}

// the bound (c) of a result kind: sum |a b| scale / u must stay below it
constexpr int64_t exact_bound(Result r) {
    return r == RF32 ? (int64_t)1 << 23 : r == RI32 ? (int64_t)1 << 31 : (int64_t)1 << 52;
}

// the table_bytes(set) blob the kernel copies into LDS; the base set's is
// cusweep::build_table()
inline std::vector<uint8_t> build_table(int set) {
    if (set == kBase) return cusweep::build_table();
    std::vector<uint8_t> blob((size_t)table_bytes(set));
    for (int p = 0; p < n_pipes(set); ++p)
        for (int t = 0; t < kTests; ++t) {
            const TestVector v = make_test(set, p, t);
            uint8_t *dst = blob.data() + test_offset(set, p, t);
            std::memcpy(dst, v.a_frag.data(), v.a_frag.size());
            dst += v.a_frag.size();
            std::memcpy(dst, v.b_frag.data(), v.b_frag.size());
            dst += v.b_frag.size();
            if (scaled(set)) {
                std::memcpy(dst, v.scale_a.data(), v.scale_a.size() * 4);
                dst += v.scale_a.size() * 4;
                std::memcpy(dst, v.scale_b.data(), v.scale_b.size() * 4);
                dst += v.scale_b.size() * 4;
            }
            std::memcpy(dst, v.expected.data(), v.expected.size() * 4);
        }
    return blob;
}

}  // namespace cusweepx

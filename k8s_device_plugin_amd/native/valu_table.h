// VALU sweep tables: the ops of each set, the packed layout that the kernel
// (valu_kernels.h) and the host share, and the host-only generator that
// fills operands from a seeded hash and expected result bits from a host
// reference (fmaf / fma, integer arithmetic, an explicit round-to-nearest-
// even encoder, the statement of each lane permutation).  The expected bits
// of set trans are recorded from the hardware: valu_trans_gfx950.inc.
//
// Layout of one test of one op, 32-bit words:
//   operands  [L lanes][in_words]   a, b, c, old in that order, as wide as
//                                   the descriptor says
//   expected  [L lanes][regs]
// with L = 64, or 1 for set salu, whose operands are wave-uniform.  Tests
// of an op follow each other, ops follow each other, the table is padded to
// 16 bytes.
#pragma once

#include <cstdint>

#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace valusweep {

constexpr int kLanes = 64;
enum Set { kFma = 0, kInt, kCvt, kXlane, kSalu, kTrans, kSets };
constexpr const char *kSetName[kSets] = {"fma", "int", "cvt", "xlane", "salu", "trans"};

enum Kind {
    // fma
    FMA_F32, FMA_F64, PK_FMA_F32, PK_FMA_F16, ADD_F32, MUL_F32, ADD_F64, MUL_F64,
    MAXIMUM3_F32, MED3_I32,
    // int
    MUL_LO_U32, MUL_HI_U32, MUL_HI_I32, MAD_U64_U32, LSHLREV_B64, ALIGNBIT_B32,
    PERM_B32, BFE_U32, BFE_I32, BFI_B32, BCNT_U32_B32, FFBH_U32, DOT4_I32_I8,
    BITOP3_96, BITOP3_E8,
    // cvt
    CVT_F16_F32, CVT_F32_F16, CVT_PK_BF16_F32, CVT_F64_F32, CVT_F32_F64,
    CVT_I32_F32, CVT_F32_U32, CVT_PK_FP8_F32, CVT_PK_BF8_F32, CVT_F32_FP8,
    CVT_F32_BF8, CVT_SCALE_PK_FP4_F32,
    // xlane
    DPP_QUAD_1032, DPP_QUAD_3301_MASKED, DPP_ROW_SHR1, DPP_ROW_SHR15, DPP_ROW_ROR4,
    DPP_ROW_MIRROR_MASKED, DPP_ROW_HALF_MIRROR, DPP_ROW_BCAST15, DPP_ROW_BCAST31,
    SWIZZLE_BITMASK, SWIZZLE_QUAD, BPERMUTE, PERMUTE, READLANE, READFIRSTLANE,
    WRITELANE, PERMLANE16_SWAP, PERMLANE32_SWAP,
    // salu
    S_MUL_I32, S_MUL_HI_U32, S_ADD_ADDC_U32, S_LSHL_B64, S_BFE_U32, S_BFE_I64,
    S_BCNT1_I32_B64, S_FF1_I32_B64, S_FLBIT_I32_B64, S_CSELECT_B32,
    S_AND_SAVEEXEC_B64,
    // trans
    EXP_F32, LOG_F32, RCP_F32, RSQ_F32, SQRT_F32, SIN_F32, RCP_F64,
};

// the masks of the two masked DPP ops and the patterns of the swizzles
constexpr int kQuadMaskedRowMask = 0x5, kQuadMaskedBankMask = 0xF;
constexpr int kMirrorMaskedRowMask = 0xF, kMirrorMaskedBankMask = 0x9;
constexpr int kSwizzleBitmask = 0x1F | 0x02 << 5 | 0x15 << 10;  // and, or, xor
constexpr int kSwizzleQuad = 0x8000 | 0x1B;                     // [3,2,1,0]

constexpr uint32_t kAll = 0xFFFFFFFFu;

struct OpDesc {
    Kind kind;
    const char *name;      // unique over all sets
    const char *mnemonic;  // the machine instruction
    uint8_t w[4];          // words per lane of a, b, c, old (0 = not taken)
    uint8_t regs;          // result registers
    // bits that must be 0 somewhere and 1 somewhere over an op's vectors:
    // per operand (every word of it) and per result register
    uint32_t vary[4];
    uint32_t out_vary[4];
};

#define VS_ALL4 {kAll, kAll, kAll, kAll}

constexpr int kFmaOps = 10;
constexpr OpDesc kFmaDesc[kFmaOps] = {
    {FMA_F32, "v_fma_f32", "v_fma_f32", {1, 1, 1, 0}, 1, VS_ALL4, VS_ALL4},
    {FMA_F64, "v_fma_f64", "v_fma_f64", {2, 2, 2, 0}, 2, VS_ALL4, VS_ALL4},
    {PK_FMA_F32, "v_pk_fma_f32", "v_pk_fma_f32", {2, 2, 2, 0}, 2, VS_ALL4, VS_ALL4},
    {PK_FMA_F16, "v_pk_fma_f16", "v_pk_fma_f16", {1, 1, 1, 0}, 1, VS_ALL4, VS_ALL4},
    {ADD_F32, "v_add_f32", "v_add_f32", {1, 1, 0, 0}, 1, VS_ALL4, VS_ALL4},
    {MUL_F32, "v_mul_f32", "v_mul_f32", {1, 1, 0, 0}, 1, VS_ALL4, VS_ALL4},
    {ADD_F64, "v_add_f64", "v_add_f64", {2, 2, 0, 0}, 2, VS_ALL4, VS_ALL4},
    {MUL_F64, "v_mul_f64", "v_mul_f64", {2, 2, 0, 0}, 2, VS_ALL4, VS_ALL4},
    {MAXIMUM3_F32, "v_maximum3_f32", "v_maximum3_f32", {1, 1, 1, 0}, 1, VS_ALL4, VS_ALL4},
    {MED3_I32, "v_med3_i32", "v_med3_i32", {1, 1, 1, 0}, 1, VS_ALL4, VS_ALL4},
};

constexpr int kIntOps = 15;
constexpr OpDesc kIntDesc[kIntOps] = {
    {MUL_LO_U32, "v_mul_lo_u32", "v_mul_lo_u32", {1, 1, 0, 0}, 1, VS_ALL4, VS_ALL4},
    {MUL_HI_U32, "v_mul_hi_u32", "v_mul_hi_u32", {1, 1, 0, 0}, 1, VS_ALL4, VS_ALL4},
    {MUL_HI_I32, "v_mul_hi_i32", "v_mul_hi_i32", {1, 1, 0, 0}, 1, VS_ALL4, VS_ALL4},
    {MAD_U64_U32, "v_mad_u64_u32", "v_mad_u64_u32", {1, 1, 2, 0}, 2, VS_ALL4, VS_ALL4},
    {LSHLREV_B64, "v_lshlrev_b64", "v_lshlrev_b64", {1, 2, 0, 0}, 2, VS_ALL4, VS_ALL4},
    {ALIGNBIT_B32, "v_alignbit_b32", "v_alignbit_b32", {1, 1, 1, 0}, 1, VS_ALL4, VS_ALL4},
    // the selector's bytes are 0..15: a byte, a sign, 0x00 or 0xFF
    {PERM_B32, "v_perm_b32", "v_perm_b32", {1, 1, 1, 0}, 1,
     {kAll, kAll, 0x0F0F0F0Fu, kAll}, VS_ALL4},
    // the width is c & 31: at most 31 result bits
    {BFE_U32, "v_bfe_u32", "v_bfe_u32", {1, 1, 1, 0}, 1, VS_ALL4, {0x7FFFFFFFu, 0, 0, 0}},
    {BFE_I32, "v_bfe_i32", "v_bfe_i32", {1, 1, 1, 0}, 1, VS_ALL4, VS_ALL4},
    {BFI_B32, "v_bfi_b32", "v_bfi_b32", {1, 1, 1, 0}, 1, VS_ALL4, VS_ALL4},
    {BCNT_U32_B32, "v_bcnt_u32_b32", "v_bcnt_u32_b32", {1, 1, 0, 0}, 1, VS_ALL4, VS_ALL4},
    // 0..31, or all ones for a zero operand
    {FFBH_U32, "v_ffbh_u32", "v_ffbh_u32", {1, 0, 0, 0}, 1, VS_ALL4, VS_ALL4},
    {DOT4_I32_I8, "v_dot4_i32_i8", "v_dot4_i32_i8", {1, 1, 1, 0}, 1, VS_ALL4, VS_ALL4},
    {BITOP3_96, "v_bitop3_b32.0x96", "v_bitop3_b32", {1, 1, 1, 0}, 1, VS_ALL4, VS_ALL4},
    {BITOP3_E8, "v_bitop3_b32.0xe8", "v_bitop3_b32", {1, 1, 1, 0}, 1, VS_ALL4, VS_ALL4},
};

constexpr int kCvtOps = 12;
constexpr OpDesc kCvtDesc[kCvtOps] = {
    {CVT_F16_F32, "v_cvt_f16_f32", "v_cvt_f16_f32", {1, 0, 0, 0}, 1, VS_ALL4,
     {0xFFFFu, 0, 0, 0}},
    {CVT_F32_F16, "v_cvt_f32_f16", "v_cvt_f32_f16", {1, 0, 0, 0}, 1,
     {0xFFFFu, 0, 0, 0}, {0xFFFFE000u, 0, 0, 0}},
    {CVT_PK_BF16_F32, "v_cvt_pk_bf16_f32", "v_cvt_pk_bf16_f32", {1, 1, 0, 0}, 1,
     VS_ALL4, VS_ALL4},
    // 23 mantissa bits in 52: the low 29 result bits are zero
    {CVT_F64_F32, "v_cvt_f64_f32", "v_cvt_f64_f32", {1, 0, 0, 0}, 2, VS_ALL4,
     {0xE0000000u, kAll, 0, 0}},
    {CVT_F32_F64, "v_cvt_f32_f64", "v_cvt_f32_f64", {2, 0, 0, 0}, 1, VS_ALL4, VS_ALL4},
    {CVT_I32_F32, "v_cvt_i32_f32", "v_cvt_i32_f32", {1, 0, 0, 0}, 1, VS_ALL4, VS_ALL4},
    // never negative
    {CVT_F32_U32, "v_cvt_f32_u32", "v_cvt_f32_u32", {1, 0, 0, 0}, 1, VS_ALL4,
     {0x7FFFFFFFu, 0, 0, 0}},
    // result 0: word select 0 over old, result 1: word select 1
    {CVT_PK_FP8_F32, "v_cvt_pk_fp8_f32", "v_cvt_pk_fp8_f32", {1, 1, 0, 1}, 2,
     VS_ALL4, VS_ALL4},
    {CVT_PK_BF8_F32, "v_cvt_pk_bf8_f32", "v_cvt_pk_bf8_f32", {1, 1, 0, 1}, 2,
     VS_ALL4, VS_ALL4},
    // result r: byte select r; 3 / 2 mantissa bits in 23
    {CVT_F32_FP8, "v_cvt_f32_fp8", "v_cvt_f32_fp8", {1, 0, 0, 0}, 4, VS_ALL4,
     {0xFFF00000u, 0xFFF00000u, 0xFFF00000u, 0xFFF00000u}},
    {CVT_F32_BF8, "v_cvt_f32_bf8", "v_cvt_f32_bf8", {1, 0, 0, 0}, 4, VS_ALL4,
     {0xFFE00000u, 0xFFE00000u, 0xFFE00000u, 0xFFE00000u}},
    // c is the scale, 1/2, 1 or 2; result r: the byte written at position r
    {CVT_SCALE_PK_FP4_F32, "v_cvt_scalef32_pk_fp4_f32", "v_cvt_scalef32_pk_fp4_f32",
     {1, 1, 1, 1}, 4, {kAll, kAll, 0x7F800000u, kAll}, VS_ALL4},
};

constexpr int kXlaneOps = 18;
#define VS_DPP(kind, suffix) \
    {kind, "v_mov_b32_dpp." suffix, "v_mov_b32_dpp", {1, 0, 0, 1}, 1, VS_ALL4, VS_ALL4}
constexpr OpDesc kXlaneDesc[kXlaneOps] = {
    VS_DPP(DPP_QUAD_1032, "quad_perm_1032"),
    VS_DPP(DPP_QUAD_3301_MASKED, "quad_perm_3301_row_mask_5"),
    VS_DPP(DPP_ROW_SHR1, "row_shr_1"),
    VS_DPP(DPP_ROW_SHR15, "row_shr_15"),
    VS_DPP(DPP_ROW_ROR4, "row_ror_4"),
    VS_DPP(DPP_ROW_MIRROR_MASKED, "row_mirror_bank_mask_9"),
    VS_DPP(DPP_ROW_HALF_MIRROR, "row_half_mirror"),
    VS_DPP(DPP_ROW_BCAST15, "row_bcast_15"),
    VS_DPP(DPP_ROW_BCAST31, "row_bcast_31"),
    {SWIZZLE_BITMASK, "ds_swizzle_b32.bitmask", "ds_swizzle_b32", {1, 0, 0, 0}, 1,
     VS_ALL4, VS_ALL4},
    {SWIZZLE_QUAD, "ds_swizzle_b32.quad_3210", "ds_swizzle_b32", {1, 0, 0, 0}, 1,
     VS_ALL4, VS_ALL4},
    // b is the byte index of each lane
    {BPERMUTE, "ds_bpermute_b32", "ds_bpermute_b32", {1, 1, 0, 0}, 1, VS_ALL4, VS_ALL4},
    {PERMUTE, "ds_permute_b32", "ds_permute_b32", {1, 1, 0, 0}, 1, VS_ALL4, VS_ALL4},
    // b is the lane select, taken from the first lane
    {READLANE, "v_readlane_b32", "v_readlane_b32", {1, 1, 0, 0}, 1,
     {kAll, 0x3Fu, kAll, kAll}, VS_ALL4},
    {READFIRSTLANE, "v_readfirstlane_b32", "v_readfirstlane_b32", {1, 0, 0, 0}, 1,
     VS_ALL4, VS_ALL4},
    // a is the value and b the lane select, both taken from the first lane
    {WRITELANE, "v_writelane_b32", "v_writelane_b32", {1, 1, 0, 1}, 1,
     {kAll, 0x3Fu, kAll, kAll}, VS_ALL4},
    {PERMLANE16_SWAP, "v_permlane16_swap_b32", "v_permlane16_swap_b32", {1, 1, 0, 0}, 2,
     VS_ALL4, VS_ALL4},
    {PERMLANE32_SWAP, "v_permlane32_swap_b32", "v_permlane32_swap_b32", {1, 1, 0, 0}, 2,
     VS_ALL4, VS_ALL4},
};

constexpr int kSaluOps = 11;
constexpr OpDesc kSaluDesc[kSaluOps] = {
    {S_MUL_I32, "s_mul_i32", "s_mul_i32", {1, 1, 0, 0}, 1, VS_ALL4, VS_ALL4},
    {S_MUL_HI_U32, "s_mul_hi_u32", "s_mul_hi_u32", {1, 1, 0, 0}, 1, VS_ALL4, VS_ALL4},
    {S_ADD_ADDC_U32, "s_add_u32+s_addc_u32", "s_addc_u32", {2, 2, 0, 0}, 2, VS_ALL4, VS_ALL4},
    {S_LSHL_B64, "s_lshl_b64", "s_lshl_b64", {2, 1, 0, 0}, 2, VS_ALL4, VS_ALL4},
    // b: offset in bits 4:0 (5:0 for i64), width in bits 22:16, offset +
    // width within the operand and width >= 1
    {S_BFE_U32, "s_bfe_u32", "s_bfe_u32", {1, 1, 0, 0}, 1,
     {kAll, 0x003F001Fu, kAll, kAll}, VS_ALL4},
    {S_BFE_I64, "s_bfe_i64", "s_bfe_i64", {2, 1, 0, 0}, 2,
     {kAll, 0x007F003Fu, kAll, kAll}, VS_ALL4},
    // 0..64; 0..63 or all ones
    {S_BCNT1_I32_B64, "s_bcnt1_i32_b64", "s_bcnt1_i32_b64", {2, 0, 0, 0}, 1, VS_ALL4,
     {0x7Fu, 0, 0, 0}},
    {S_FF1_I32_B64, "s_ff1_i32_b64", "s_ff1_i32_b64", {2, 0, 0, 0}, 1, VS_ALL4, VS_ALL4},
    {S_FLBIT_I32_B64, "s_flbit_i32_b64", "s_flbit_i32_b64", {2, 0, 0, 0}, 1, VS_ALL4, VS_ALL4},
    // a < b (signed) ? c : old, after s_cmp_lt_i32
    {S_CSELECT_B32, "s_cselect_b32", "s_cselect_b32", {1, 1, 1, 1}, 1, VS_ALL4, VS_ALL4},
    // results 0, 1: the saved EXEC, all ones in a full wave; 2, 3: the EXEC
    // the instruction set, a & EXEC.  EXEC is restored right after.
    {S_AND_SAVEEXEC_B64, "s_and_saveexec_b64", "s_and_saveexec_b64", {2, 0, 0, 0}, 4,
     VS_ALL4, {0, 0, kAll, kAll}},
};

constexpr int kTransOps = 7;
// positive operands for log, rsq and sqrt; |x| in [2^-10, 1) for sin.  The
// result bits are the hardware's own (recorded): no coverage rule for them.
#define VS_TRANS(kind, name, vary_a) \
    {kind, name, name, {1, 0, 0, 0}, 1, {vary_a, kAll, kAll, kAll}, {0, 0, 0, 0}}
constexpr OpDesc kTransDesc[kTransOps] = {
    VS_TRANS(EXP_F32, "v_exp_f32", kAll),
    VS_TRANS(LOG_F32, "v_log_f32", 0x7FFFFFFFu),
    VS_TRANS(RCP_F32, "v_rcp_f32", kAll),
    VS_TRANS(RSQ_F32, "v_rsq_f32", 0x7FFFFFFFu),
    VS_TRANS(SQRT_F32, "v_sqrt_f32", 0x7FFFFFFFu),
    VS_TRANS(SIN_F32, "v_sin_f32", 0x87FFFFFFu),
    {RCP_F64, "v_rcp_f64", "v_rcp_f64", {2, 0, 0, 0}, 2, VS_ALL4, {0, 0, 0, 0}},
};

constexpr int n_ops(int set) {
    return set == kFma ? kFmaOps : set == kInt ? kIntOps : set == kCvt ? kCvtOps
           : set == kXlane ? kXlaneOps : set == kSalu ? kSaluOps : kTransOps;
}
constexpr const OpDesc &desc(int set, int op) {
    return set == kFma ? kFmaDesc[op] : set == kInt ? kIntDesc[op]
           : set == kCvt ? kCvtDesc[op] : set == kXlane ? kXlaneDesc[op]
           : set == kSalu ? kSaluDesc[op] : kTransDesc[op];
}
static_assert(kFmaOps <= 32 && kIntOps <= 32 && kCvtOps <= 32 && kXlaneOps <= 32 &&
                  kSaluOps <= 32 && kTransOps <= 32,
              "SweepRecord::fail_pipes has one bit per op");

// vectors per op: four of 64 lanes each; sixteen for the wave-uniform salu
constexpr int n_tests(int set) { return set == kSalu ? 16 : 4; }
constexpr int lanes(int set) { return set == kSalu ? 1 : kLanes; }
constexpr int in_words(int set, int op) {
    return desc(set, op).w[0] + desc(set, op).w[1] + desc(set, op).w[2] +
           desc(set, op).w[3];
}
// first word of operand `which` among a lane's operand words
constexpr int in_offset(int set, int op, int which) {
    int o = 0;
    for (int i = 0; i < which; ++i) o += desc(set, op).w[i];
    return o;
}
constexpr int regs(int set, int op) { return desc(set, op).regs; }
constexpr int test_bytes(int set, int op) {
    return lanes(set) * (in_words(set, op) + regs(set, op)) * 4;
}
constexpr int op_offset(int set, int op) {
    int o = 0;
    for (int i = 0; i < op; ++i) o += n_tests(set) * test_bytes(set, i);
    return o;
}
constexpr int test_offset(int set, int op, int t) {
    return op_offset(set, op) + t * test_bytes(set, op);
}
constexpr int table_bytes(int set) { return (op_offset(set, n_ops(set)) + 15) / 16 * 16; }
// Dynamic LDS of a sweep block: over half of the CU's 160 KiB whatever the
// table's size, so two sweep blocks cannot share a CU.
constexpr int lds_bytes(int set) {
    return table_bytes(set) > 80 * 1024 + 16 ? table_bytes(set) : 80 * 1024 + 16;
}
static_assert(lds_bytes(kFma) <= 160 * 1024 && lds_bytes(kInt) <= 160 * 1024 &&
                  lds_bytes(kCvt) <= 160 * 1024 && lds_bytes(kXlane) <= 160 * 1024 &&
                  lds_bytes(kSalu) <= 160 * 1024 && lds_bytes(kTrans) <= 160 * 1024,
              "a set's table fits one CU's LDS");

// recorded result words of set trans: [op][t][lane][reg]
constexpr int trans_words() {
    int n = 0;
    for (int op = 0; op < kTransOps; ++op)
        n += n_tests(kTrans) * kLanes * regs(kTrans, op);
    return n;
}

// ---------------- host only: operands and expected bits ----------------

inline const uint32_t *trans_recorded() {
    static const uint32_t words[] = {
#include "valu_trans_gfx950.inc"
    };
    static_assert(sizeof(words) / 4 == (size_t)trans_words(),
                  "valu_trans_gfx950.inc does not match the trans tables");
    return words;
}

constexpr uint32_t hash32(uint32_t x) {
    x *= 2654435761u;
    x ^= x >> 15;
    x *= 2246822519u;
    x ^= x >> 13;
    x *= 3266489917u;
    x ^= x >> 16;
    return x;
}
// draw j of (set, op, t, lane, operand word)
constexpr uint32_t draw(int set, int op, int t, int lane, int word, int j = 0) {
    return hash32(hash32((uint32_t)((((set * 32 + op) * 16 + t) * 64 + lane) * 8 + word)) +
                  0x9E3779B9u * (uint32_t)(j + 1));
}

inline float f32_of(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }
inline uint32_t bits_of(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }
inline double f64_of(uint64_t b) { double f; std::memcpy(&f, &b, 8); return f; }
inline uint64_t bits_of(double f) { uint64_t b; std::memcpy(&b, &f, 8); return b; }

// a normal number of hashed sign and full hashed mantissa, 2^emin <= |x| < 2^(emax+1)
inline uint32_t f32_in(uint32_t h, uint32_t h2, int emin, int emax) {
    const uint32_t e = (uint32_t)(127 + emin + (int)(h2 % (uint32_t)(emax - emin + 1)));
    return (h & 0x807FFFFFu) | e << 23;
}
inline uint64_t f64_in(uint32_t h, uint32_t h2, uint32_t h3, int emin, int emax) {
    const uint64_t e = (uint64_t)(1023 + emin + (int)(h2 % (uint32_t)(emax - emin + 1)));
    return ((uint64_t)(h & 0x800FFFFFu) << 32 | h3) | e << 52;
}
inline uint32_t f16_in(uint32_t h, uint32_t h2, int emin, int emax) {
    const uint32_t e = (uint32_t)(15 + emin + (int)(h2 % (uint32_t)(emax - emin + 1)));
    return (h & 0x83FFu) | e << 10;
}
// a hashed value of a uniformly drawn bit length 0..32
inline uint32_t of_bit_length(uint32_t h, uint32_t h2) {
    const int len = (int)(h2 % 33u);
    return len == 0 ? 0u : (h | 0x80000000u) >> (32 - len);
}

// x, finite and non-zero, to a format of ebits exponent and mbits mantissa
// bits, round to nearest even; the result must be a normal number of it
inline uint32_t encode_rne(double x, int ebits, int mbits, int bias, int max_code) {
    const uint32_t sign = std::signbit(x) ? 1u : 0u;
    int e = 0;
    const double m = std::frexp(std::fabs(x), &e);  // 0.5 <= m < 1
    // |x| = (2m) * 2^(e-1); scaled mantissa with mbits fraction bits
    double scaled = std::ldexp(m, mbits + 1);       // in [2^mbits, 2^(mbits+1))
    double fl = std::floor(scaled);
    const double rest = scaled - fl;
    if (rest > 0.5 || (rest == 0.5 && std::fmod(fl, 2.0) == 1.0)) fl += 1.0;
    int exp = e - 1;
    if (fl == std::ldexp(1.0, mbits + 1)) {
        fl = std::ldexp(1.0, mbits);
        ++exp;
    }
    const int biased = exp + bias;
    const uint32_t code = (uint32_t)biased << mbits | ((uint32_t)fl & ((1u << mbits) - 1));
    if (biased < 1 || biased >= (1 << ebits) || (int)code > max_code)
        throw std::logic_error("encode_rne: operand outside the normal range");
    return sign << (ebits + mbits) | code;
}
inline uint32_t to_f16(double x) { return encode_rne(x, 5, 10, 15, 0x7BFF); }
inline uint32_t to_bf16(double x) { return encode_rne(x, 8, 7, 127, 0x7F7F); }
inline uint32_t to_fp8(double x) { return encode_rne(x, 4, 3, 7, 0x7E); }   // OCP e4m3
inline uint32_t to_bf8(double x) { return encode_rne(x, 5, 2, 15, 0x7B); }  // OCP e5m2
inline uint32_t to_fp4(double x) { return encode_rne(x, 2, 1, 1, 0x7); }    // e2m1

// value of a small float code (denormals included, no inf / nan codes given)
inline double decode_small(uint32_t code, int ebits, int mbits, int bias) {
    const uint32_t m = code & ((1u << mbits) - 1);
    const int e = (int)(code >> mbits & ((1u << ebits) - 1));
    const double mag = e == 0 ? std::ldexp((double)m, 1 - bias - mbits)
                              : std::ldexp((double)(m | 1u << mbits), e - bias - mbits);
    return code >> (ebits + mbits) & 1 ? -mag : mag;
}
inline bool fp8_is_nan(uint32_t c) { return (c & 0x7F) == 0x7F; }
inline bool bf8_is_special(uint32_t c) { return (c & 0x7C) == 0x7C; }

// the lanes' low six bits: a bijection of 0..63 that differs per test
inline uint32_t lane_tag(int t, int lane) { return (uint32_t)(lane * 37 + t * 11 + 5) & 63u; }
// Cross-lane data: hashed above bit 8, pairwise distinct over the 64 lanes
// and over the operands a, b and old of one test.
inline uint32_t xlane_value(int op, int t, int lane, int which) {
    return (draw(kXlane, op, t, lane, which) & 0xFFFFFF00u) |
           (uint32_t)((which + t) & 3) << 6 | lane_tag(t, lane);
}
// the byte index of bpermute / permute: lane select in bits 7:2, the rest
// hashed.  A permutation of the lanes, except bpermute's test 3.
inline uint32_t xlane_index(int op, int t, int lane, bool permutation) {
    const uint32_t sel = permutation ? (uint32_t)(lane * 29 + 17 * t + 3) & 63u
                                     : draw(kXlane, op, t, lane, 1, 7) % 11u * 5u;
    return (draw(kXlane, op, t, lane, 1) & 0xFFFFFF03u) | sel << 2;
}

inline void gen_operands(int set, int op, int t, int lane, uint32_t *in) {
    const OpDesc &d = desc(set, op);
    const int n = in_words(set, op);
    auto h = [&](int word, int j = 0) { return draw(set, op, t, lane, word, j); };
    for (int i = 0; i < n; ++i) in[i] = h(i);
    auto put64 = [&](int at, uint64_t v) {
        in[at] = (uint32_t)v;
        in[at + 1] = (uint32_t)(v >> 32);
    };
    switch (d.kind) {
    case FMA_F32: case PK_FMA_F32: case ADD_F32: case MUL_F32: case MAXIMUM3_F32:
        for (int i = 0; i < n; ++i) in[i] = f32_in(h(i), h(i, 1), -8, 7);
        break;
    case FMA_F64: case ADD_F64: case MUL_F64:
        for (int i = 0; i < n; i += 2) put64(i, f64_in(h(i), h(i, 1), h(i + 1), -8, 7));
        break;
    case PK_FMA_F16:
        // c takes the product's sign: no cancellation into the denormals
        for (int half = 0; half < 2; ++half) {
            const uint32_t a = f16_in(h(0, half), h(0, 2 + half), -3, 3);
            const uint32_t b = f16_in(h(1, half), h(1, 2 + half), -3, 3);
            uint32_t c = f16_in(h(2, half), h(2, 2 + half), -3, 3);
            c = (c & 0x7FFFu) | ((a ^ b) & 0x8000u);
            if (half == 0) in[0] = in[1] = in[2] = 0;
            in[0] |= a << (16 * half);
            in[1] |= b << (16 * half);
            in[2] |= c << (16 * half);
        }
        break;
    case PERM_B32:
        in[2] &= 0x0F0F0F0Fu;
        break;
    case CVT_F16_F32: in[0] = f32_in(h(0), h(0, 1), -12, 14); break;
    case CVT_F32_F16: in[0] = f16_in(h(0), h(0, 1), -14, 15); break;
    case CVT_PK_BF16_F32:
        for (int i = 0; i < 2; ++i) in[i] = f32_in(h(i), h(i, 1), -20, 20);
        break;
    case CVT_F64_F32: in[0] = f32_in(h(0), h(0, 1), -20, 20); break;
    case CVT_F32_F64: put64(0, f64_in(h(0), h(0, 1), h(1), -20, 20)); break;
    case CVT_I32_F32: in[0] = f32_in(h(0), h(0, 1), -2, 30); break;
    case CVT_PK_FP8_F32:
        for (int i = 0; i < 2; ++i) in[i] = f32_in(h(i), h(i, 1), -6, 7);
        break;
    case CVT_PK_BF8_F32:
        for (int i = 0; i < 2; ++i) in[i] = f32_in(h(i), h(i, 1), -14, 14);
        break;
    case CVT_F32_FP8:
        for (int b = 0; b < 4; ++b)
            if (fp8_is_nan(in[0] >> (8 * b))) in[0] ^= 1u << (8 * b);
        break;
    case CVT_F32_BF8:
        for (int b = 0; b < 4; ++b)
            if (bf8_is_special(in[0] >> (8 * b))) in[0] ^= 0x40u << (8 * b);
        break;
    case CVT_SCALE_PK_FP4_F32: {
        // x / scale in [1, 6): mantissa 1.0 .. 1.5 at exponent 2, any below
        const int se = (int)(h(2) % 3u) - 1;  // scale 2^se
        for (int i = 0; i < 2; ++i) {
            const int e = (int)(h(i, 1) % 3u);
            uint32_t x = f32_in(h(i), 0, e, e);
            if (e == 2) x &= ~0x00400000u;  // below 1.5 * 4
            in[i] = x + ((uint32_t)se << 23);
        }
        in[2] = (uint32_t)(127 + se) << 23;
        break;
    }
    case S_BFE_U32: {
        // tests 0, 1: the whole word and its complement; 2: the top bit
        const uint32_t width = t < 2 ? 32u : t == 2 ? 1u : 1 + h(1) % 32u,
                       off = t == 2 ? 31u : h(1, 1) % (33u - width);
        in[1] = width << 16 | off;
        break;
    }
    case S_BFE_I64: {
        const uint32_t width = t < 2 ? 64u : t == 2 ? 1u : 1 + h(2) % 64u,
                       off = t == 2 ? 63u : h(2, 1) % (65u - width);
        in[2] = width << 16 | off;
        break;
    }
    case EXP_F32: {
        // [-20, 20]: 2^-8 <= |x| < 16, or 16 <= |x| <= 20
        uint32_t x = f32_in(h(0), h(0, 1), -8, 4);
        if ((x >> 23 & 0xFF) == 131) x &= ~0x00600000u;  // 16 .. 20
        in[0] = x;
        break;
    }
    case LOG_F32: case RSQ_F32: case SQRT_F32:
        in[0] = f32_in(h(0), h(0, 1), -20, 19) & 0x7FFFFFFFu;
        break;
    case RCP_F32: in[0] = f32_in(h(0), h(0, 1), -20, 19); break;
    case SIN_F32: in[0] = f32_in(h(0), h(0, 1), -10, -1); break;  // |x| < 1 revolution
    case RCP_F64: put64(0, f64_in(h(0), h(0, 1), h(1), -20, 19)); break;
    default:
        break;
    }
    if (set == kInt) {
        // a uniformly drawn bit length; lanes 0..3 hold the corners
        for (int i = 0; i < n; ++i) {
            const uint32_t corner[4] = {kAll, 0u, 0xAAAAAAAAu, 0x55555555u};
            in[i] = lane < 4 ? corner[(lane + (t & 1) * i) & 3] : of_bit_length(h(i), h(i, 1));
        }
        // lane 4: all ones, 0, 31 (the widest field from bit 0)
        if (lane == 4)
            for (int i = 0; i < n; ++i) in[i] = i == 0 ? kAll : i == 1 ? 0u : 31u;
        if (d.kind == PERM_B32) in[2] &= 0x0F0F0F0Fu;
    }
    if (d.kind == CVT_F32_U32)
        in[0] = lane == 0 ? kAll : lane == 1 ? 0u : of_bit_length(h(0), h(0, 1));
    if (set == kSalu && d.kind != S_BFE_U32 && d.kind != S_BFE_I64) {
        // tests 0, 1: all ones, zero; then hashed words and their complements
        for (int i = 0; i < n; ++i) {
            const uint32_t v = draw(set, op, t / 2, 0, i, 3);
            in[i] = t == 0 ? kAll : t == 1 ? 0u : t & 1 ? ~v : v;
        }
        if (d.kind == S_CSELECT_B32 && t >= 8) in[1] = in[0] ^ (1u << (t % 32));
        if (d.kind == S_LSHL_B64 && t >= 2) {
            // a pair (v, ~v) shares its count, so every result bit from the
            // count up toggles
            const uint32_t count[7] = {0, 1, 31, 32, 63, 5, 17};
            in[2] = (in[2] & ~63u) | count[(t - 2) / 2];
        }
    }
    if (set == kSalu && (d.kind == S_BFE_U32 || d.kind == S_BFE_I64))
        for (int i = 0; i < d.w[0]; ++i) {
            const uint32_t v = draw(set, op, t / 2, 0, i, 3);
            in[i] = t & 1 ? ~v : v;
        }
    if (set == kXlane) {
        int at = 0;
        for (int which = 0; which < 4; ++which)
            if (d.w[which]) in[at++] = xlane_value(op, t, lane, which);
        if (d.kind == BPERMUTE) in[1] = xlane_index(op, t, lane, t != 3);
        if (d.kind == PERMUTE) in[1] = xlane_index(op, t, lane, true);
        // the lane select: the corners first
        const uint32_t sel[4] = {0, 63, 31, 16};
        if (d.kind == READLANE || d.kind == WRITELANE)
            in[1] = (draw(kXlane, op, t, 0, 1) & 0xFFFFFFC0u) | sel[t];
        // the one lane that is read: a hashed word in tests 0 and 2, its
        // complement in 1 and 3, above the tag
        if ((d.kind == READLANE && lane == (int)sel[t]) ||
            (d.kind == READFIRSTLANE && lane == 0)) {
            const uint32_t p = draw(kXlane, op, t / 2, 0, 0, 5);
            in[0] = ((t & 1 ? ~p : p) & 0xFFFFFF00u) | (in[0] & 0xFFu);
        }
    }
}

inline int32_t sext(uint64_t v, int bits) {
    return (int32_t)((int64_t)(v << (64 - bits)) >> (64 - bits));
}

inline uint32_t perm_byte(uint64_t both, uint32_t sel) {
    if (sel <= 7) return (uint32_t)(both >> (8 * sel)) & 0xFF;
    if (sel <= 11) return both >> (16 * (sel - 8) + 15) & 1 ? 0xFFu : 0u;
    return sel == 12 ? 0u : 0xFFu;
}

// source lane of a DPP control, -1 where the lane keeps old
inline int dpp_source(Kind k, int l) {
    const int row = l & ~15, r = l & 15;
    auto masked = [&](int row_mask, int bank_mask) {
        return (row_mask >> (l >> 4) & 1) && (bank_mask >> (r >> 2) & 1);
    };
    switch (k) {
    case DPP_QUAD_1032: { const int q[4] = {1, 0, 3, 2}; return (l & ~3) + q[l & 3]; }
    case DPP_QUAD_3301_MASKED: {
        const int q[4] = {3, 3, 0, 1};
        return masked(kQuadMaskedRowMask, kQuadMaskedBankMask) ? (l & ~3) + q[l & 3] : -1;
    }
    case DPP_ROW_SHR1: return r >= 1 ? l - 1 : -1;
    case DPP_ROW_SHR15: return r >= 15 ? l - 15 : -1;
    case DPP_ROW_ROR4: return row | ((r - 4) & 15);
    case DPP_ROW_MIRROR_MASKED:
        return masked(kMirrorMaskedRowMask, kMirrorMaskedBankMask) ? row | (15 - r) : -1;
    case DPP_ROW_HALF_MIRROR: return (l & ~7) | (7 - (l & 7));
    // Lane 15 of each row to every lane of the next row; lane 31 to rows 2
    // and 3.  A lane without such a source takes its OWN lane of the source
    // register, not old: measured with valu_raw on MI355X (docs/health.md).
    case DPP_ROW_BCAST15: return l >= 16 ? row - 1 : l;
    case DPP_ROW_BCAST31: return l >= 32 ? 31 : l;
    default: return -1;
    }
}

// Expected result words of one test from its operand words: in is
// [L][in_words], out [L][regs].
inline void expected_of(int set, int op, const uint32_t *in, uint32_t *out) {
    const OpDesc &d = desc(set, op);
    const int L = lanes(set), NI = in_words(set, op), R = d.regs;
    const int oa = 0, ob = d.w[0], oc = ob + d.w[1], oo = oc + d.w[2];
    if (set == kXlane) {
        auto A = [&](int l) { return in[l * NI + oa]; };
        auto B = [&](int l) { return in[l * NI + ob]; };
        auto OLD = [&](int l) { return in[l * NI + oo]; };
        for (int l = 0; l < L; ++l) {
            uint32_t *o = out + l * R;
            switch (d.kind) {
            case SWIZZLE_BITMASK: {
                const int a = kSwizzleBitmask & 31, orm = kSwizzleBitmask >> 5 & 31,
                          x = kSwizzleBitmask >> 10 & 31;
                o[0] = A((l & 32) | ((((l & 31) & a) | orm) ^ x));
                break;
            }
            case SWIZZLE_QUAD: o[0] = A((l & ~3) | (kSwizzleQuad >> (2 * (l & 3)) & 3)); break;
            case BPERMUTE: o[0] = A((int)(B(l) >> 2 & 63)); break;
            case PERMUTE:
                for (int s = 0; s < L; ++s)
                    if ((int)(B(s) >> 2 & 63) == l) o[0] = A(s);
                break;
            case READLANE: o[0] = A((int)(B(0) & 63)); break;
            case READFIRSTLANE: o[0] = A(0); break;
            case WRITELANE: o[0] = l == (int)(B(0) & 63) ? A(0) : OLD(l); break;
            case PERMLANE16_SWAP:
                o[0] = (l >> 4 & 1) ? B(l - 16) : A(l);
                o[1] = (l >> 4 & 1) ? B(l) : A(l + 16);
                break;
            case PERMLANE32_SWAP:
                o[0] = l >= 32 ? B(l - 32) : A(l);
                o[1] = l >= 32 ? B(l) : A(l + 32);
                break;
            default: {
                const int s = dpp_source(d.kind, l);
                o[0] = s < 0 ? OLD(l) : A(s);
            }
            }
        }
        return;
    }
    if (set == kTrans) return;  // recorded, see build_table
    for (int l = 0; l < L; ++l) {
        const uint32_t *i = in + l * NI;
        uint32_t *o = out + l * R;
        const uint32_t a = i[oa], b = d.w[1] ? i[ob] : 0, c = d.w[2] ? i[oc] : 0,
                       old = d.w[3] ? i[oo] : 0;
        auto u64 = [&](int at) { return (uint64_t)i[at + 1] << 32 | i[at]; };
        auto out64 = [&](uint64_t v) {
            o[0] = (uint32_t)v;
            o[1] = (uint32_t)(v >> 32);
        };
        switch (d.kind) {
        case FMA_F32: o[0] = bits_of(std::fmaf(f32_of(a), f32_of(b), f32_of(c))); break;
        case FMA_F64:
            out64(bits_of(std::fma(f64_of(u64(oa)), f64_of(u64(ob)), f64_of(u64(oc)))));
            break;
        case PK_FMA_F32:
            for (int k = 0; k < 2; ++k)
                o[k] = bits_of(std::fmaf(f32_of(i[oa + k]), f32_of(i[ob + k]), f32_of(i[oc + k])));
            break;
        case PK_FMA_F16:
            o[0] = 0;
            for (int k = 0; k < 2; ++k) {
                auto v = [&](uint32_t w) { return decode_small(w >> (16 * k) & 0xFFFF, 5, 10, 15); };
                // exact in double: 22 product bits and 11 more within 2^12
                o[0] |= to_f16(v(a) * v(b) + v(c)) << (16 * k);
            }
            break;
        case ADD_F32: o[0] = bits_of(f32_of(a) + f32_of(b)); break;
        case MUL_F32: o[0] = bits_of(f32_of(a) * f32_of(b)); break;
        case ADD_F64: out64(bits_of(f64_of(u64(oa)) + f64_of(u64(ob)))); break;
        case MUL_F64: out64(bits_of(f64_of(u64(oa)) * f64_of(u64(ob)))); break;
        case MAXIMUM3_F32:
            o[0] = bits_of(std::fmax(f32_of(a), std::fmax(f32_of(b), f32_of(c))));
            break;
        case MED3_I32: {
            const int32_t x = (int32_t)a, y = (int32_t)b, z = (int32_t)c;
            const int32_t lo = x < y ? x : y, hi = x < y ? y : x;
            o[0] = (uint32_t)(z < lo ? lo : z > hi ? hi : z);
            break;
        }
        case MUL_LO_U32: case S_MUL_I32: o[0] = a * b; break;
        case MUL_HI_U32: case S_MUL_HI_U32: o[0] = (uint32_t)((uint64_t)a * b >> 32); break;
        case MUL_HI_I32:
            o[0] = (uint32_t)((uint64_t)((int64_t)(int32_t)a * (int32_t)b) >> 32);
            break;
        case MAD_U64_U32: out64((uint64_t)a * b + u64(oc)); break;
        case LSHLREV_B64: out64(u64(ob) << (a & 63)); break;
        case ALIGNBIT_B32: o[0] = (uint32_t)(((uint64_t)a << 32 | b) >> (c & 31)); break;
        case PERM_B32: {
            const uint64_t both = (uint64_t)a << 32 | b;
            o[0] = 0;
            for (int k = 0; k < 4; ++k) o[0] |= perm_byte(both, c >> (8 * k) & 0xFF) << (8 * k);
            break;
        }
        case BFE_U32: {
            const uint32_t off = b & 31, w = c & 31;
            o[0] = w ? (a >> off) & ((1u << w) - 1) : 0;
            break;
        }
        case BFE_I32: {
            const uint32_t off = b & 31, w = c & 31;
            if (!w) o[0] = 0;
            else if (off + w < 32) o[0] = (uint32_t)sext(a >> off, (int)w);
            else o[0] = (uint32_t)((int32_t)a >> off);
            break;
        }
        case BFI_B32: o[0] = (a & b) | (~a & c); break;
        case BCNT_U32_B32: o[0] = (uint32_t)__builtin_popcount(a) + b; break;
        case FFBH_U32: o[0] = a ? (uint32_t)__builtin_clz(a) : kAll; break;
        case DOT4_I32_I8: {
            uint32_t s = c;
            for (int k = 0; k < 4; ++k)
                s += (uint32_t)((int32_t)(int8_t)(a >> (8 * k)) * (int32_t)(int8_t)(b >> (8 * k)));
            o[0] = s;
            break;
        }
        case BITOP3_96: o[0] = a ^ b ^ c; break;
        case BITOP3_E8: o[0] = (a & b) | (a & c) | (b & c); break;
        case CVT_F16_F32: o[0] = to_f16((double)f32_of(a)); break;
        case CVT_F32_F16: o[0] = bits_of((float)decode_small(a & 0xFFFF, 5, 10, 15)); break;
        case CVT_PK_BF16_F32:
            o[0] = to_bf16((double)f32_of(a)) | to_bf16((double)f32_of(b)) << 16;
            break;
        case CVT_F64_F32: out64(bits_of((double)f32_of(a))); break;
        case CVT_F32_F64: o[0] = bits_of((float)f64_of(u64(oa))); break;
        case CVT_I32_F32: o[0] = (uint32_t)(int32_t)f32_of(a); break;  // toward zero
        case CVT_F32_U32: o[0] = bits_of((float)a); break;
        case CVT_PK_FP8_F32: case CVT_PK_BF8_F32: {
            const bool bf8 = d.kind == CVT_PK_BF8_F32;
            const double x = (double)f32_of(a), y = (double)f32_of(b);
            const uint32_t pair = bf8 ? to_bf8(x) | to_bf8(y) << 8 : to_fp8(x) | to_fp8(y) << 8;
            o[0] = (old & 0xFFFF0000u) | pair;
            o[1] = (old & 0x0000FFFFu) | pair << 16;
            break;
        }
        case CVT_F32_FP8:
            for (int k = 0; k < 4; ++k)
                o[k] = bits_of((float)decode_small(a >> (8 * k) & 0xFF, 4, 3, 7));
            break;
        case CVT_F32_BF8:
            for (int k = 0; k < 4; ++k)
                o[k] = bits_of((float)decode_small(a >> (8 * k) & 0xFF, 5, 2, 15));
            break;
        case CVT_SCALE_PK_FP4_F32: {
            const double s = (double)f32_of(c);
            const uint32_t byte = to_fp4((double)f32_of(a) / s) | to_fp4((double)f32_of(b) / s) << 4;
            for (int k = 0; k < 4; ++k)
                o[k] = (old & ~(0xFFu << (8 * k))) | byte << (8 * k);
            break;
        }
        case S_ADD_ADDC_U32: out64(u64(oa) + u64(ob)); break;
        case S_LSHL_B64: out64(u64(oa) << (b & 63)); break;
        case S_BFE_U32: {
            const uint32_t off = b & 31, w = b >> 16 & 0x7F;
            o[0] = w >= 32 ? a >> off : (a >> off) & ((1u << w) - 1);
            break;
        }
        case S_BFE_I64: {
            const uint32_t off = b & 63, w = b >> 16 & 0x7F;
            const uint64_t field = u64(oa) >> off;
            out64(w >= 64 ? field : (uint64_t)((int64_t)(field << (64 - w)) >> (64 - w)));
            break;
        }
        case S_BCNT1_I32_B64: o[0] = (uint32_t)__builtin_popcountll(u64(oa)); break;
        case S_FF1_I32_B64: o[0] = u64(oa) ? (uint32_t)__builtin_ctzll(u64(oa)) : kAll; break;
        case S_FLBIT_I32_B64: o[0] = u64(oa) ? (uint32_t)__builtin_clzll(u64(oa)) : kAll; break;
        case S_CSELECT_B32: o[0] = (int32_t)a < (int32_t)b ? c : old; break;
        case S_AND_SAVEEXEC_B64:
            o[0] = o[1] = kAll;
            o[2] = i[0];
            o[3] = i[1];
            break;
        default:
            throw std::logic_error("expected_of: no reference for this op");
        }
    }
}

struct TestVector {
    std::vector<uint32_t> in;        // [L][in_words]
    std::vector<uint32_t> expected;  // [L][regs]
};

inline TestVector make_test(int set, int op, int t) {
    const int L = lanes(set), NI = in_words(set, op), R = regs(set, op);
    TestVector v;
    v.in.resize((size_t)L * NI);
    v.expected.assign((size_t)L * R, 0);
    for (int l = 0; l < L; ++l) gen_operands(set, op, t, l, &v.in[(size_t)l * NI]);
    if (set == kTrans) {
        size_t at = 0;
        for (int p = 0; p < op; ++p) at += (size_t)n_tests(set) * kLanes * regs(set, p);
        at += (size_t)t * kLanes * R;
        for (size_t k = 0; k < v.expected.size(); ++k) v.expected[k] = trans_recorded()[at + k];
    } else {
        expected_of(set, op, v.in.data(), v.expected.data());
    }
    return v;
}

inline std::vector<uint8_t> build_table(int set) {
    std::vector<uint8_t> table((size_t)table_bytes(set), 0);
    for (int op = 0; op < n_ops(set); ++op)
        for (int t = 0; t < n_tests(set); ++t) {
            const TestVector v = make_test(set, op, t);
            uint8_t *at = table.data() + test_offset(set, op, t);
            std::memcpy(at, v.in.data(), v.in.size() * 4);
            std::memcpy(at + v.in.size() * 4, v.expected.data(), v.expected.size() * 4);
        }
    return table;
}

}  // namespace valusweep

// gfx950 device code of the VALU sweep: known-answer vector, conversion,
// cross-lane, scalar and transcendental ops on every SIMD of every CU, in
// the shape of cu_sweep_kernel (probe_kernels.h), whose record, wave state,
// compare step and inject hook it reuses.  The ops and the table layout are
// valu_table.h's.
//
// Every op is ONE named machine instruction: a builtin that lowers to it,
// or a one-instruction inline-asm helper.  A plain C++ expression will not
// do: at -O3 the compiler packs neighbouring f32 operations into v_pk_*,
// folds constants and picks another instruction for the same value.  Where
// an asm string pads (s_nop), the pad covers a hazard that the compiler
// does not see inside asm: a VALU write of a VGPR two states before a DPP
// read of it, an SALU write of EXEC before what follows.
#pragma once

#include "probe_kernels.h"
#include "valu_table.h"

namespace {

using u32x2v = __attribute__((ext_vector_type(2))) uint32_t;

#define VS_V3(text, r, x, y, z) \
    asm volatile(text " %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(y), "v"(z))
#define VS_V2(text, r, x, y) asm volatile(text " %0, %1, %2" : "=v"(r) : "v"(x), "v"(y))
#define VS_V1(text, r, x) asm volatile(text " %0, %1" : "=v"(r) : "v"(x))
#define VS_DPP_ASM(ctrl, old, src)                              \
    asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %1 " ctrl        \
                 : "+v"(old) : "v"(src))

// Op OP of set SET on this lane's operand words in (a, b, c, old in the
// descriptor's widths): the result register bits d.
template <int SET, int OP>
__device__ inline void valu_op(const uint32_t *in, uint32_t *d) {
    using namespace valusweep;
    constexpr OpDesc D = desc(SET, OP);
    constexpr Kind K = D.kind;
#if defined(__gfx950__)
    constexpr int OB = in_offset(SET, OP, 1), OC = in_offset(SET, OP, 2),
                  OO = in_offset(SET, OP, 3);
    const uint32_t a = in[0];
    uint32_t b = 0, c = 0, old = 0;
    if constexpr (D.w[1] > 0) b = in[OB];
    if constexpr (D.w[2] > 0) c = in[OC];
    if constexpr (D.w[3] > 0) old = in[OO];
    uint64_t a64 = 0, b64 = 0, c64 = 0;
    if constexpr (D.w[0] == 2) a64 = (uint64_t)in[1] << 32 | in[0];
    if constexpr (D.w[1] == 2) b64 = (uint64_t)in[OB + 1] << 32 | in[OB];
    if constexpr (D.w[2] == 2) c64 = (uint64_t)in[OC + 1] << 32 | in[OC];
    uint32_t r = 0;
    uint64_t r64 = 0;
    auto out64 = [&] {
        d[0] = (uint32_t)r64;
        d[1] = (uint32_t)(r64 >> 32);
    };

    // ---- fma ----
    if constexpr (K == FMA_F32) { VS_V3("v_fma_f32", r, a, b, c); d[0] = r; }
    else if constexpr (K == FMA_F64) { VS_V3("v_fma_f64", r64, a64, b64, c64); out64(); }
    else if constexpr (K == PK_FMA_F32) { VS_V3("v_pk_fma_f32", r64, a64, b64, c64); out64(); }
    else if constexpr (K == PK_FMA_F16) { VS_V3("v_pk_fma_f16", r, a, b, c); d[0] = r; }
    else if constexpr (K == ADD_F32) { VS_V2("v_add_f32", r, a, b); d[0] = r; }
    else if constexpr (K == MUL_F32) { VS_V2("v_mul_f32", r, a, b); d[0] = r; }
    else if constexpr (K == ADD_F64) { VS_V2("v_add_f64", r64, a64, b64); out64(); }
    else if constexpr (K == MUL_F64) { VS_V2("v_mul_f64", r64, a64, b64); out64(); }
    else if constexpr (K == MAXIMUM3_F32) { VS_V3("v_maximum3_f32", r, a, b, c); d[0] = r; }
    else if constexpr (K == MED3_I32) { VS_V3("v_med3_i32", r, a, b, c); d[0] = r; }
    // ---- int ----
    else if constexpr (K == MUL_LO_U32) { VS_V2("v_mul_lo_u32", r, a, b); d[0] = r; }
    else if constexpr (K == MUL_HI_U32) { VS_V2("v_mul_hi_u32", r, a, b); d[0] = r; }
    else if constexpr (K == MUL_HI_I32) { VS_V2("v_mul_hi_i32", r, a, b); d[0] = r; }
    else if constexpr (K == MAD_U64_U32) {
        asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %3"
                     : "=&v"(r64) : "v"(a), "v"(b), "v"(c64) : "vcc");
        out64();
    }
    else if constexpr (K == LSHLREV_B64) { VS_V2("v_lshlrev_b64", r64, a, b64); out64(); }
    else if constexpr (K == ALIGNBIT_B32) { VS_V3("v_alignbit_b32", r, a, b, c); d[0] = r; }
    else if constexpr (K == PERM_B32) { VS_V3("v_perm_b32", r, a, b, c); d[0] = r; }
    else if constexpr (K == BFE_U32) { VS_V3("v_bfe_u32", r, a, b, c); d[0] = r; }
    else if constexpr (K == BFE_I32) { VS_V3("v_bfe_i32", r, a, b, c); d[0] = r; }
    else if constexpr (K == BFI_B32) { VS_V3("v_bfi_b32", r, a, b, c); d[0] = r; }
    else if constexpr (K == BCNT_U32_B32) { VS_V2("v_bcnt_u32_b32", r, a, b); d[0] = r; }
    else if constexpr (K == FFBH_U32) { VS_V1("v_ffbh_u32", r, a); d[0] = r; }
    else if constexpr (K == DOT4_I32_I8) { VS_V3("v_dot4_i32_i8", r, a, b, c); d[0] = r; }
    else if constexpr (K == BITOP3_96) {
        asm volatile("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(r) : "v"(a), "v"(b), "v"(c));
        d[0] = r;
    }
    else if constexpr (K == BITOP3_E8) {
        asm volatile("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xe8" : "=v"(r) : "v"(a), "v"(b), "v"(c));
        d[0] = r;
    }
    // ---- cvt ----
    else if constexpr (K == CVT_F16_F32) { VS_V1("v_cvt_f16_f32", r, a); d[0] = r & 0xFFFFu; }
    else if constexpr (K == CVT_F32_F16) { VS_V1("v_cvt_f32_f16", r, a); d[0] = r; }
    else if constexpr (K == CVT_PK_BF16_F32) { VS_V2("v_cvt_pk_bf16_f32", r, a, b); d[0] = r; }
    else if constexpr (K == CVT_F64_F32) { VS_V1("v_cvt_f64_f32", r64, a); out64(); }
    else if constexpr (K == CVT_F32_F64) { VS_V1("v_cvt_f32_f64", r, a64); d[0] = r; }
    else if constexpr (K == CVT_I32_F32) { VS_V1("v_cvt_i32_f32", r, a); d[0] = r; }
    else if constexpr (K == CVT_F32_U32) { VS_V1("v_cvt_f32_u32", r, a); d[0] = r; }
    else if constexpr (K == CVT_PK_FP8_F32) {
        const float x = __uint_as_float(a), y = __uint_as_float(b);
        d[0] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(x, y, (int)old, false);
        d[1] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(x, y, (int)old, true);
    }
    else if constexpr (K == CVT_PK_BF8_F32) {
        const float x = __uint_as_float(a), y = __uint_as_float(b);
        d[0] = (uint32_t)__builtin_amdgcn_cvt_pk_bf8_f32(x, y, (int)old, false);
        d[1] = (uint32_t)__builtin_amdgcn_cvt_pk_bf8_f32(x, y, (int)old, true);
    }
    else if constexpr (K == CVT_F32_FP8) {
        d[0] = __float_as_uint(__builtin_amdgcn_cvt_f32_fp8((int)a, 0));
        d[1] = __float_as_uint(__builtin_amdgcn_cvt_f32_fp8((int)a, 1));
        d[2] = __float_as_uint(__builtin_amdgcn_cvt_f32_fp8((int)a, 2));
        d[3] = __float_as_uint(__builtin_amdgcn_cvt_f32_fp8((int)a, 3));
    }
    else if constexpr (K == CVT_F32_BF8) {
        d[0] = __float_as_uint(__builtin_amdgcn_cvt_f32_bf8((int)a, 0));
        d[1] = __float_as_uint(__builtin_amdgcn_cvt_f32_bf8((int)a, 1));
        d[2] = __float_as_uint(__builtin_amdgcn_cvt_f32_bf8((int)a, 2));
        d[3] = __float_as_uint(__builtin_amdgcn_cvt_f32_bf8((int)a, 3));
    }
    else if constexpr (K == CVT_SCALE_PK_FP4_F32) {
        const float x = __uint_as_float(a), y = __uint_as_float(b), s = __uint_as_float(c);
        d[0] = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(old, x, y, s, 0);
        d[1] = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(old, x, y, s, 1);
        d[2] = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(old, x, y, s, 2);
        d[3] = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(old, x, y, s, 3);
    }
    // ---- xlane ----
    else if constexpr (K == DPP_QUAD_1032) {
        VS_DPP_ASM("quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf", old, a); d[0] = old;
    }
    else if constexpr (K == DPP_QUAD_3301_MASKED) {
        static_assert(kQuadMaskedRowMask == 0x5 && kQuadMaskedBankMask == 0xF, "the asm text");
        VS_DPP_ASM("quad_perm:[3,3,0,1] row_mask:0x5 bank_mask:0xf", old, a); d[0] = old;
    }
    else if constexpr (K == DPP_ROW_SHR1) {
        VS_DPP_ASM("row_shr:1 row_mask:0xf bank_mask:0xf", old, a); d[0] = old;
    }
    else if constexpr (K == DPP_ROW_SHR15) {
        VS_DPP_ASM("row_shr:15 row_mask:0xf bank_mask:0xf", old, a); d[0] = old;
    }
    else if constexpr (K == DPP_ROW_ROR4) {
        VS_DPP_ASM("row_ror:4 row_mask:0xf bank_mask:0xf", old, a); d[0] = old;
    }
    else if constexpr (K == DPP_ROW_MIRROR_MASKED) {
        static_assert(kMirrorMaskedRowMask == 0xF && kMirrorMaskedBankMask == 0x9, "the asm text");
        VS_DPP_ASM("row_mirror row_mask:0xf bank_mask:0x9", old, a); d[0] = old;
    }
    else if constexpr (K == DPP_ROW_HALF_MIRROR) {
        VS_DPP_ASM("row_half_mirror row_mask:0xf bank_mask:0xf", old, a); d[0] = old;
    }
    else if constexpr (K == DPP_ROW_BCAST15) {
        VS_DPP_ASM("row_bcast:15 row_mask:0xf bank_mask:0xf", old, a); d[0] = old;
    }
    else if constexpr (K == DPP_ROW_BCAST31) {
        VS_DPP_ASM("row_bcast:31 row_mask:0xf bank_mask:0xf", old, a); d[0] = old;
    }
    else if constexpr (K == SWIZZLE_BITMASK)
        d[0] = (uint32_t)__builtin_amdgcn_ds_swizzle((int)a, kSwizzleBitmask);
    else if constexpr (K == SWIZZLE_QUAD)
        d[0] = (uint32_t)__builtin_amdgcn_ds_swizzle((int)a, kSwizzleQuad);
    else if constexpr (K == BPERMUTE)
        d[0] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)b, (int)a);
    else if constexpr (K == PERMUTE)
        d[0] = (uint32_t)__builtin_amdgcn_ds_permute((int)b, (int)a);
    else if constexpr (K == READLANE)
        d[0] = (uint32_t)__builtin_amdgcn_readlane(
            (int)a, __builtin_amdgcn_readfirstlane((int)b) & 63);
    else if constexpr (K == READFIRSTLANE)
        d[0] = (uint32_t)__builtin_amdgcn_readfirstlane((int)a);
    else if constexpr (K == WRITELANE) {
        // no builtin; two scalar sources, so the lane select goes through M0,
        // which is the compiler's: saved and put back in the same statement
        const uint32_t value = __builtin_amdgcn_readfirstlane(a),
                       select = __builtin_amdgcn_readfirstlane(b) & 63;
        uint32_t keep;
        asm volatile("s_mov_b32 %1, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                     "v_writelane_b32 %0, %2, m0\n\ts_mov_b32 m0, %1"
                     : "+v"(old), "=&s"(keep) : "s"(value), "s"(select));
        d[0] = old;
    }
    else if constexpr (K == PERMLANE16_SWAP) {
        const u32x2v o = __builtin_amdgcn_permlane16_swap(a, b, false, false);
        d[0] = o[0];
        d[1] = o[1];
    }
    else if constexpr (K == PERMLANE32_SWAP) {
        const u32x2v o = __builtin_amdgcn_permlane32_swap(a, b, false, false);
        d[0] = o[0];
        d[1] = o[1];
    }
    // ---- trans ----
    else if constexpr (K == EXP_F32) d[0] = __float_as_uint(__builtin_amdgcn_exp2f(__uint_as_float(a)));
    else if constexpr (K == LOG_F32) d[0] = __float_as_uint(__builtin_amdgcn_logf(__uint_as_float(a)));
    else if constexpr (K == RCP_F32) d[0] = __float_as_uint(__builtin_amdgcn_rcpf(__uint_as_float(a)));
    else if constexpr (K == RSQ_F32) d[0] = __float_as_uint(__builtin_amdgcn_rsqf(__uint_as_float(a)));
    else if constexpr (K == SQRT_F32) d[0] = __float_as_uint(__builtin_amdgcn_sqrtf(__uint_as_float(a)));
    else if constexpr (K == SIN_F32) d[0] = __float_as_uint(__builtin_amdgcn_sinf(__uint_as_float(a)));
    else if constexpr (K == RCP_F64) {
        r64 = (uint64_t)__double_as_longlong(__builtin_amdgcn_rcp(__longlong_as_double((long long)a64)));
        out64();
    }
    // ---- salu: wave-uniform operands, made scalar with readfirstlane ----
    else {
        const uint32_t sa = __builtin_amdgcn_readfirstlane(a),
                       sb = __builtin_amdgcn_readfirstlane(b),
                       sc = __builtin_amdgcn_readfirstlane(c),
                       so = __builtin_amdgcn_readfirstlane(old);
        uint32_t sa1 = 0, sb1 = 0;
        if constexpr (D.w[0] == 2) sa1 = __builtin_amdgcn_readfirstlane(in[1]);
        if constexpr (D.w[1] == 2) sb1 = __builtin_amdgcn_readfirstlane(in[OB + 1]);
        const uint64_t sa64 = (uint64_t)sa1 << 32 | sa;
        uint32_t s = 0, s1 = 0;
        uint64_t s64 = 0, t64 = 0;
        if constexpr (K == S_MUL_I32) {
            asm volatile("s_mul_i32 %0, %1, %2" : "=s"(s) : "s"(sa), "s"(sb));
            d[0] = s;
        } else if constexpr (K == S_MUL_HI_U32) {
            asm volatile("s_mul_hi_u32 %0, %1, %2" : "=s"(s) : "s"(sa), "s"(sb));
            d[0] = s;
        } else if constexpr (K == S_ADD_ADDC_U32) {
            asm volatile("s_add_u32 %0, %2, %4\n\ts_addc_u32 %1, %3, %5"
                         : "=&s"(s), "=&s"(s1)
                         : "s"(sa), "s"(sa1), "s"(sb), "s"(sb1) : "scc");
            d[0] = s;
            d[1] = s1;
        } else if constexpr (K == S_LSHL_B64) {
            asm volatile("s_lshl_b64 %0, %1, %2" : "=s"(s64) : "s"(sa64), "s"(sb) : "scc");
            d[0] = (uint32_t)s64;
            d[1] = (uint32_t)(s64 >> 32);
        } else if constexpr (K == S_BFE_U32) {
            asm volatile("s_bfe_u32 %0, %1, %2" : "=s"(s) : "s"(sa), "s"(sb) : "scc");
            d[0] = s;
        } else if constexpr (K == S_BFE_I64) {
            asm volatile("s_bfe_i64 %0, %1, %2" : "=s"(s64) : "s"(sa64), "s"(sb) : "scc");
            d[0] = (uint32_t)s64;
            d[1] = (uint32_t)(s64 >> 32);
        } else if constexpr (K == S_BCNT1_I32_B64) {
            asm volatile("s_bcnt1_i32_b64 %0, %1" : "=s"(s) : "s"(sa64) : "scc");
            d[0] = s;
        } else if constexpr (K == S_FF1_I32_B64) {
            asm volatile("s_ff1_i32_b64 %0, %1" : "=s"(s) : "s"(sa64));
            d[0] = s;
        } else if constexpr (K == S_FLBIT_I32_B64) {
            asm volatile("s_flbit_i32_b64 %0, %1" : "=s"(s) : "s"(sa64));
            d[0] = s;
        } else if constexpr (K == S_CSELECT_B32) {
            asm volatile("s_cmp_lt_i32 %1, %2\n\ts_cselect_b32 %0, %3, %4"
                         : "=s"(s) : "s"(sa), "s"(sb), "s"(sc), "s"(so) : "scc");
            d[0] = s;
        } else {
            static_assert(K == S_AND_SAVEEXEC_B64, "an op without device code");
            // EXEC is the saved mask again before anything else runs
            asm volatile("s_and_saveexec_b64 %0, %2\n\ts_mov_b64 %1, exec\n\t"
                         "s_mov_b64 exec, %0\n\ts_nop 4"
                         : "=&s"(s64), "=&s"(t64) : "s"(sa64) : "scc");
            d[0] = (uint32_t)s64;
            d[1] = (uint32_t)(s64 >> 32);
            d[2] = (uint32_t)t64;
            d[3] = (uint32_t)(t64 >> 32);
        }
        (void)sc;
        (void)so;
        (void)sb1;
    }
    (void)b; (void)c; (void)old; (void)a64; (void)b64; (void)c64; (void)r; (void)r64;
#else
    (void)K;
    for (int k = 0; k < D.regs; ++k) d[k] = in[0];
#endif
}

// register the inject hook flips: kSweepInjectReg where the op has it
constexpr int valu_inject_reg(int regs) {
    return kSweepInjectReg < regs ? kSweepInjectReg : regs - 1;
}

// every test of op OP of set SET
template <int SET, int OP>
__device__ inline void valu_sweep_op(const unsigned char *table, int lane, bool inject,
                                     SweepWaveState &st, SweepRecord *rec) {
    constexpr int NI = valusweep::in_words(SET, OP), R = valusweep::regs(SET, OP),
                  L = valusweep::lanes(SET);
    const int at = L == 1 ? 0 : lane;
    for (int t = 0; t < valusweep::n_tests(SET); ++t) {
        const uint32_t *base = reinterpret_cast<const uint32_t *>(
            table + valusweep::test_offset(SET, OP, t));
        uint32_t in[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            in[i] = base[at * NI + i];
            // opaque each round: nothing is folded or hoisted out of the reps loop
            asm volatile("" : "+v"(in[i]));
        }
        uint32_t d[R];
        valu_op<SET, OP>(in, d);
        sweep_check<R>(OP, t, lane, d, base + L * NI + at * R, inject,
                       valu_inject_reg(R), st, rec);
    }
}

template <int SET, int... OP>
__device__ inline void valu_sweep_ops(std::integer_sequence<int, OP...>,
                                      const unsigned char *table, int lane, bool mine,
                                      int inject_op, SweepWaveState &st, SweepRecord *rec) {
    (valu_sweep_op<SET, OP>(table, lane, mine && inject_op == OP, st, rec), ...);
}

// One 4-wave block per CU for op set SET (valusweep::Set).  The block
// copies the set's packed operand and expected-result table into LDS; the
// launch asks for valusweep::lds_bytes(SET) of dynamic LDS, more than half
// of the CU's 160 KiB, so no two sweep blocks share a CU.  Each wave reads
// where it runs from the hardware id registers, runs reps rounds of every
// op of the set on its SIMD (set salu: on its CU's scalar unit) and compares
// every result register bit for bit.  Records, coverage and the inject
// arguments are cu_sweep_kernel's, with an op in the place of a pipe.
template <int SET>
__global__ void __launch_bounds__(256)
valu_sweep_kernel(const uint4 *__restrict__ table, SweepRecord *records, int reps,
                  int inject_block, int inject_wave, int inject_op) {
    extern __shared__ uint4 sweep_lds[];
    for (int i = threadIdx.x; i < valusweep::table_bytes(SET) / 16; i += blockDim.x)
        sweep_lds[i] = table[i];
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    SweepRecord *rec = &records[blockIdx.x * 4 + wave];
    const uint32_t hw_id = __builtin_amdgcn_s_getreg(4 | 31 << 11);
    const uint32_t xcc_id = __builtin_amdgcn_s_getreg(20 | 3 << 11);
    const bool mine = (int)blockIdx.x == inject_block && wave == inject_wave;
    const unsigned char *tbl = reinterpret_cast<const unsigned char *>(sweep_lds);

    SweepWaveState st;
    for (int rep = 0; rep < reps; ++rep)
        valu_sweep_ops<SET>(std::make_integer_sequence<int, valusweep::n_ops(SET)>{}, tbl,
                            lane, mine, inject_op, st, rec);
    if (lane == 0) {
        rec->hw_id = hw_id;
        rec->xcc_id = xcc_id;
        rec->fail_pipes = st.fail_pipes;
        rec->bad_lanes_lo = (uint32_t)st.bad_lanes;
        rec->bad_lanes_hi = (uint32_t)(st.bad_lanes >> 32);
    }
}

// One wave, op OP of set SET once on caller-supplied operand words
// in[lane * in_words + i] (valu_raw): out[lane * regs + r].
template <int SET, int OP>
__global__ void __launch_bounds__(64)
valu_raw_kernel(const uint32_t *__restrict__ in_words, uint32_t *out) {
    constexpr int NI = valusweep::in_words(SET, OP), R = valusweep::regs(SET, OP);
    const int lane = threadIdx.x;
    uint32_t in[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        in[i] = in_words[lane * NI + i];
        asm volatile("" : "+v"(in[i]));
    }
    uint32_t d[R];
    valu_op<SET, OP>(in, d);
    for (int r = 0; r < R; ++r) out[lane * R + r] = d[r];
}

#undef VS_V3
#undef VS_V2
#undef VS_V1
#undef VS_DPP_ASM

}  // namespace

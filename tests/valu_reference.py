"""An independent statement of every VALU sweep op, for the tests.

Not a test module.  Nothing here shares code with the generator of
native/valu_table.h: floats are exact `fractions.Fraction`s rounded once by
an explicit round-to-nearest-even on integers, integer ops are Python integer
arithmetic, and the cross-lane ops are index arithmetic over the 64 lanes.

`REFERENCE[name](lanes)` takes one operand tuple per lane (the op's operand
words a, b, c, old in order, 64 lanes, or one for the scalar set) and returns
one result-word tuple per lane.
"""

from fractions import Fraction

M32 = 0xFFFFFFFF


# ---------------- floats as exact fractions ----------------

def decode(bits, ebits, mbits, bias):
    """Value of a binary float code (no inf / nan codes are given)."""
    m = bits & ((1 << mbits) - 1)
    e = bits >> mbits & ((1 << ebits) - 1)
    if e == 0:
        mag = Fraction(m, 1 << mbits) * Fraction(2) ** (1 - bias)
    else:
        mag = (1 + Fraction(m, 1 << mbits)) * Fraction(2) ** (e - bias)
    return -mag if bits >> (ebits + mbits) & 1 else mag


def f32(bits):
    return decode(bits, 8, 23, 127)


def f64(lo, hi):
    return decode(hi << 32 | lo, 11, 52, 1023)


def f16(bits):
    return decode(bits & 0xFFFF, 5, 10, 15)


def encode(x, ebits, mbits, bias, negative_zero=False):
    """x rounded once, to nearest, ties to even; the result is a normal
    number of the format, or zero."""
    if x == 0:
        return (1 << (ebits + mbits)) if negative_zero else 0
    sign = 1 if x < 0 else 0
    x = abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    assert Fraction(2) ** e <= x < Fraction(2) ** (e + 1)
    scaled = x / Fraction(2) ** (e - mbits)  # in [2^mbits, 2^(mbits+1))
    q, rest = divmod(scaled.numerator, scaled.denominator)
    twice = 2 * rest
    if twice > scaled.denominator or (twice == scaled.denominator and q & 1):
        q += 1
    if q == 1 << (mbits + 1):
        q >>= 1
        e += 1
    biased = e + bias
    assert 1 <= biased < (1 << ebits), "outside the normal range"
    return sign << (ebits + mbits) | biased << mbits | (q & ((1 << mbits) - 1))


def to_f32(x):
    return encode(x, 8, 23, 127)


def to_f64_words(x):
    code = encode(x, 11, 52, 1023)
    return code & M32, code >> 32


def s32(v):
    return v - (1 << 32) if v & 0x80000000 else v


def s8(v):
    v &= 0xFF
    return v - 256 if v & 0x80 else v


# ---------------- lane-local ops ----------------

def each(fn):
    return lambda lanes: [tuple(fn(*words)) for words in lanes]


def pk_fma_f16(a, b, c):
    out = 0
    for k in (0, 16):
        out |= encode(f16(a >> k) * f16(b >> k) + f16(c >> k), 5, 10, 15) << k
    return (out,)


def med3(a, b, c):
    return (sorted((s32(a), s32(b), s32(c)))[1] & M32,)


def perm_b32(a, b, sel):
    both = a << 32 | b
    out = 0
    for k in range(4):
        s = sel >> (8 * k) & 0xFF
        if s <= 7:
            byte = both >> (8 * s) & 0xFF
        elif s <= 11:
            byte = 0xFF if both >> (16 * (s - 8) + 15) & 1 else 0
        else:
            byte = 0 if s == 12 else 0xFF
        out |= byte << (8 * k)
    return (out,)


def bfe_i32(a, off, width):
    off &= 31
    width &= 31
    if width == 0:
        return (0,)
    if off + width < 32:
        field = a >> off & ((1 << width) - 1)
        if field >> (width - 1):
            field -= 1 << width
        return (field & M32,)
    return ((s32(a) >> off) & M32,)


def dot4(a, b, c):
    return ((c + sum(s8(a >> k) * s8(b >> k) for k in (0, 8, 16, 24))) & M32,)


def cvt_i32_f32(a):
    x = f32(a)  # toward zero
    n = abs(x).numerator // abs(x).denominator
    return ((-n if x < 0 else n) & M32,)


def cvt_f32_u32(a):
    return (to_f32(Fraction(a)),)


def cvt_pk8(ebits, mbits, bias):
    def fn(a, b, old):
        pair = encode(f32(a), ebits, mbits, bias) | encode(f32(b), ebits, mbits, bias) << 8
        return ((old & 0xFFFF0000) | pair, (old & 0x0000FFFF) | pair << 16)
    return fn


def cvt_from8(ebits, mbits, bias):
    def fn(a):
        out = []
        for k in range(4):
            code = a >> (8 * k) & 0xFF
            out.append(encode(decode(code, ebits, mbits, bias), 8, 23, 127,
                              negative_zero=bool(code & 0x80)))
        return out
    return fn


def cvt_fp4(a, b, scale, old):
    s = f32(scale)
    byte = encode(f32(a) / s, 2, 1, 1) | encode(f32(b) / s, 2, 1, 1) << 4
    return [(old & ~(0xFF << (8 * k)) & M32) | byte << (8 * k) for k in range(4)]


def s_bfe_u32(a, b):
    off, width = b & 31, b >> 16 & 0x7F
    return ((a >> off) & ((1 << width) - 1) & M32,)


def s_bfe_i64(lo, hi, b):
    off, width = b & 63, b >> 16 & 0x7F
    field = (hi << 32 | lo) >> off & ((1 << width) - 1)
    if width and field >> (width - 1):
        field -= 1 << width
    field &= (1 << 64) - 1
    return (field & M32, field >> 32)


def first_one(v, from_top):
    if v == 0:
        return M32
    if from_top:
        return 64 - v.bit_length()
    return (v & -v).bit_length() - 1


def u64_words(v):
    v &= (1 << 64) - 1
    return (v & M32, v >> 32)


LANE_LOCAL = {
    "v_fma_f32": lambda a, b, c: (to_f32(f32(a) * f32(b) + f32(c)),),
    "v_fma_f64": lambda a0, a1, b0, b1, c0, c1: to_f64_words(
        f64(a0, a1) * f64(b0, b1) + f64(c0, c1)),
    "v_pk_fma_f32": lambda a0, a1, b0, b1, c0, c1: (
        to_f32(f32(a0) * f32(b0) + f32(c0)), to_f32(f32(a1) * f32(b1) + f32(c1))),
    "v_pk_fma_f16": pk_fma_f16,
    "v_add_f32": lambda a, b: (to_f32(f32(a) + f32(b)),),
    "v_mul_f32": lambda a, b: (to_f32(f32(a) * f32(b)),),
    "v_add_f64": lambda a0, a1, b0, b1: to_f64_words(f64(a0, a1) + f64(b0, b1)),
    "v_mul_f64": lambda a0, a1, b0, b1: to_f64_words(f64(a0, a1) * f64(b0, b1)),
    "v_maximum3_f32": lambda a, b, c: (max((a, b, c), key=f32),),
    "v_med3_i32": med3,
    "v_mul_lo_u32": lambda a, b: (a * b & M32,),
    "v_mul_hi_u32": lambda a, b: (a * b >> 32,),
    "v_mul_hi_i32": lambda a, b: (s32(a) * s32(b) >> 32 & M32,),
    "v_mad_u64_u32": lambda a, b, c0, c1: u64_words(a * b + (c1 << 32 | c0)),
    "v_lshlrev_b64": lambda a, b0, b1: u64_words((b1 << 32 | b0) << (a & 63)),
    "v_alignbit_b32": lambda a, b, c: ((a << 32 | b) >> (c & 31) & M32,),
    "v_perm_b32": perm_b32,
    "v_bfe_u32": lambda a, off, w: (a >> (off & 31) & ((1 << (w & 31)) - 1),),
    "v_bfe_i32": bfe_i32,
    "v_bfi_b32": lambda m, a, b: ((m & a) | (~m & b & M32),),
    "v_bcnt_u32_b32": lambda a, b: ((bin(a).count("1") + b) & M32,),
    "v_ffbh_u32": lambda a: (32 - a.bit_length() if a else M32,),
    "v_dot4_i32_i8": dot4,
    "v_bitop3_b32.0x96": lambda a, b, c: (a ^ b ^ c,),
    "v_bitop3_b32.0xe8": lambda a, b, c: ((a & b) | (a & c) | (b & c),),
    "v_cvt_f16_f32": lambda a: (encode(f32(a), 5, 10, 15),),
    "v_cvt_f32_f16": lambda a: (to_f32(f16(a)),),
    "v_cvt_pk_bf16_f32": lambda a, b: (
        encode(f32(a), 8, 7, 127) | encode(f32(b), 8, 7, 127) << 16,),
    "v_cvt_f64_f32": lambda a: to_f64_words(f32(a)),
    "v_cvt_f32_f64": lambda a0, a1: (to_f32(f64(a0, a1)),),
    "v_cvt_i32_f32": cvt_i32_f32,
    "v_cvt_f32_u32": cvt_f32_u32,
    "v_cvt_pk_fp8_f32": cvt_pk8(4, 3, 7),
    "v_cvt_pk_bf8_f32": cvt_pk8(5, 2, 15),
    "v_cvt_f32_fp8": cvt_from8(4, 3, 7),
    "v_cvt_f32_bf8": cvt_from8(5, 2, 15),
    "v_cvt_scalef32_pk_fp4_f32": cvt_fp4,
    "s_mul_i32": lambda a, b: (a * b & M32,),
    "s_mul_hi_u32": lambda a, b: (a * b >> 32,),
    "s_add_u32+s_addc_u32": lambda a0, a1, b0, b1: u64_words(
        (a1 << 32 | a0) + (b1 << 32 | b0)),
    "s_lshl_b64": lambda a0, a1, b: u64_words((a1 << 32 | a0) << (b & 63)),
    "s_bfe_u32": s_bfe_u32,
    "s_bfe_i64": s_bfe_i64,
    "s_bcnt1_i32_b64": lambda a0, a1: (bin(a1 << 32 | a0).count("1"),),
    "s_ff1_i32_b64": lambda a0, a1: (first_one(a1 << 32 | a0, False),),
    "s_flbit_i32_b64": lambda a0, a1: (first_one(a1 << 32 | a0, True),),
    "s_cselect_b32": lambda a, b, c, old: (c if s32(a) < s32(b) else old,),
    # a full wave: the saved EXEC is all ones, the new one is the operand
    "s_and_saveexec_b64": lambda a0, a1: (M32, M32, a0, a1),
}


# ---------------- cross-lane ops: index arithmetic ----------------

def dpp(source):
    """v_mov_b32_dpp: lane l takes a[source(l)], or keeps old where source
    gives None (a lane without a source, or masked off)."""
    def fn(lanes):
        return [(lanes[source(l)][0] if source(l) is not None else lanes[l][1],)
                for l in range(64)]
    return fn


def masked(row_mask, bank_mask, source):
    def fn(l):
        row, bank = l // 16, l % 16 // 4
        if not (row_mask >> row & 1 and bank_mask >> bank & 1):
            return None
        return source(l)
    return fn


def swizzle_bitmask(and_mask, or_mask, xor_mask):
    def fn(lanes):
        return [(lanes[l // 32 * 32 + (((l % 32) & and_mask | or_mask) ^ xor_mask)][0],)
                for l in range(64)]
    return fn


def permute(lanes):
    out = [None] * 64
    for l, (a, index) in enumerate(lanes):
        out[index // 4 % 64] = (a,)
    return out


def writelane(lanes):
    value, select = lanes[0][0], lanes[0][1] % 64
    return [(value if l == select else lanes[l][2],) for l in range(64)]


def permlane_swap(width):
    # rows of `width` lanes: the odd rows of a change places with the even
    # rows of b
    def fn(lanes):
        out = []
        for l in range(64):
            odd = l // width % 2
            out.append((lanes[l - width][1] if odd else lanes[l][0],
                        lanes[l][1] if odd else lanes[l + width][0]))
        return out
    return fn


CROSS_LANE = {
    "v_mov_b32_dpp.quad_perm_1032": dpp(lambda l: l // 4 * 4 + (1, 0, 3, 2)[l % 4]),
    "v_mov_b32_dpp.quad_perm_3301_row_mask_5": dpp(
        masked(0x5, 0xF, lambda l: l // 4 * 4 + (3, 3, 0, 1)[l % 4])),
    "v_mov_b32_dpp.row_shr_1": dpp(lambda l: l - 1 if l % 16 >= 1 else None),
    "v_mov_b32_dpp.row_shr_15": dpp(lambda l: l - 15 if l % 16 >= 15 else None),
    "v_mov_b32_dpp.row_ror_4": dpp(lambda l: l // 16 * 16 + (l % 16 - 4) % 16),
    "v_mov_b32_dpp.row_mirror_bank_mask_9": dpp(
        masked(0xF, 0x9, lambda l: l // 16 * 16 + 15 - l % 16)),
    "v_mov_b32_dpp.row_half_mirror": dpp(lambda l: l // 8 * 8 + 7 - l % 8),
    # lane 15 of each row to the next row; lane 31 to rows 2 and 3; a lane
    # without such a source takes its own lane of a (seen on the hardware)
    "v_mov_b32_dpp.row_bcast_15": dpp(lambda l: l // 16 * 16 - 1 if l >= 16 else l),
    "v_mov_b32_dpp.row_bcast_31": dpp(lambda l: 31 if l >= 32 else l),
    "ds_swizzle_b32.bitmask": swizzle_bitmask(0x1F, 0x02, 0x15),
    "ds_swizzle_b32.quad_3210": lambda lanes: [
        (lanes[l // 4 * 4 + 3 - l % 4][0],) for l in range(64)],
    "ds_bpermute_b32": lambda lanes: [
        (lanes[lanes[l][1] // 4 % 64][0],) for l in range(64)],
    "ds_permute_b32": permute,
    "v_readlane_b32": lambda lanes: [(lanes[lanes[0][1] % 64][0],)] * 64,
    "v_readfirstlane_b32": lambda lanes: [(lanes[0][0],)] * 64,
    "v_writelane_b32": writelane,
    "v_permlane16_swap_b32": permlane_swap(16),
    "v_permlane32_swap_b32": permlane_swap(32),
}

REFERENCE = {name: each(fn) for name, fn in LANE_LOCAL.items()}
REFERENCE.update(CROSS_LANE)

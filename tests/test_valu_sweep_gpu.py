"""VALU sweep on the GPU: every op of every set on one wave against the
independent reference (tests/valu_reference.py) with the corners where an op
can go wrong, the recorded transcendental words, a healthy sweep and an
injected fault per set, and the probe policy end to end.

One wave or one launch each; the tables are checked on the CPU in
tests/test_valu_sweep.py.
"""

import struct

import pytest

import k8s_device_plugin_amd.native as native

from valu_reference import REFERENCE

pytestmark = pytest.mark.gpu

SETS = ("fma", "int", "cvt", "xlane", "salu", "trans")
MUST_HAVE = {"v_fma_f32", "v_fma_f64", "v_mul_hi_u32", "v_cvt_f16_f32",
             "v_cvt_pk_bf16_f32", "s_mul_hi_u32"}
XLANE_MNEMONICS = {"v_mov_b32_dpp", "ds_swizzle_b32", "ds_bpermute_b32",
                   "ds_permute_b32", "v_readlane_b32", "v_readfirstlane_b32",
                   "v_writelane_b32", "v_permlane16_swap_b32",
                   "v_permlane32_swap_b32"}
EDGE_LANES = (0, 15, 16, 31, 32, 63)

try:  # torch's HIP runtime must load first (see __graft_entry__.build)
    import torch  # noqa: F401
except ImportError:
    pass
_MOD = native.load_healthprobe(required=False)
_REFS = {s: _MOD.valu_sweep_reference(s) for s in SETS} if _MOD else {}
# (set, op descriptor) of every op the tables hold: none is left out
OPS = [(s, op) for s in SETS for op in _REFS.get(s, {}).get("ops", [])]
KNOWN_ANSWER_OPS = [(s, op) for s, op in OPS if s != "trans"]


@pytest.fixture(scope="module")
def mod():
    if _MOD is None:
        pytest.skip("_healthprobe extension not built")
    if _MOD.device_count() < 1:
        pytest.skip("no HIP device")
    return _MOD


def vectors_of(ref, op):
    lanes, n_in, regs = ref["lanes"], op["in_words"], op["regs"]
    for offset in op["offsets"]:
        words = struct.unpack_from(f"<{lanes * (n_in + regs)}I", ref["table"], offset)
        ins = [words[l * n_in:(l + 1) * n_in] for l in range(lanes)]
        at = lanes * n_in
        yield ins, [words[at + l * regs:at + (l + 1) * regs] for l in range(lanes)]


def run_raw(mod, op, lanes):
    """valu_raw of one op on 64 operand tuples -> 64 result tuples."""
    args, at = [], 0
    for width in op["widths"]:
        args.append(b"".join(struct.pack(f"<{width}I", *lane[at:at + width])
                             for lane in lanes) if width else None)
        at += width
    out = struct.unpack(f"<{64 * op['regs']}I", mod.valu_raw(0, op["name"], *args))
    return [out[l * op["regs"]:(l + 1) * op["regs"]] for l in range(64)]


def f32(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def f64(x):
    return struct.unpack("<II", struct.pack("<d", x))


U = 2.0 ** -23  # one f32 ulp at 1.0
ONES = 0xFFFFFFFF

# Operand tuples for the first lanes of an op's wave (the scalar ops: one
# launch each), on top of the table's first vector: the corners.
CORNERS = {
    # a tie that must round to even: up to 1 + 2u, down to 1
    "v_fma_f32": [(f32(1 + U), f32(1.0), f32(U / 2)), (f32(1.0), f32(1.0), f32(U / 2)),
                  (f32(1 + U), f32(1 + U), f32(-1.0))],  # exact 2u + u^2: no double rounding
    "v_fma_f64": [f64(1 + 2.0 ** -52) + f64(1.0) + f64(2.0 ** -53),
                  f64(1.0) + f64(1.0) + f64(2.0 ** -53)],
    "v_pk_fma_f32": [(f32(1 + U), f32(1.0), f32(1.0), f32(1.0), f32(U / 2), f32(U / 2))],
    # f16: 1 + 2^-10 + 2^-11 ties up to 1 + 2^-9; 1 + 2^-11 down to 1
    "v_pk_fma_f16": [(0x3C003C01, 0x3C003C00, 0x10001000)],
    "v_add_f32": [(f32(1 + U), f32(U / 2)), (f32(1.0), f32(U / 2))],
    "v_mul_f32": [(f32(1 + U), f32(1.5)), (f32(1 + 3 * U), f32(1.5))],  # 1.5 + 1.5u, 1.5 + 4.5u
    "v_add_f64": [f64(1 + 2.0 ** -52) + f64(2.0 ** -53), f64(1.0) + f64(2.0 ** -53)],
    "v_mul_f64": [f64(1 + 2.0 ** -52) + f64(1.5), f64(1 + 3 * 2.0 ** -52) + f64(1.5)],
    "v_maximum3_f32": [(f32(-1.0), f32(-2.0), f32(-3.0)), (f32(1.0), f32(2.0), f32(-3.0))],
    "v_med3_i32": [(ONES, 0, 1), (0x80000000, 0x7FFFFFFF, 0)],
    "v_mul_lo_u32": [(ONES, ONES), (0x10000, 0x10000)],
    "v_mul_hi_u32": [(ONES, ONES), (0x10000, 0x10000), (0x80000000, 2)],
    "v_mul_hi_i32": [(ONES, ONES), (0x80000000, 0x80000000), (0x80000000, 1)],
    # a carry out of the low word, and out of the whole result
    "v_mad_u64_u32": [(1, 1, ONES, 0), (ONES, ONES, ONES, ONES), (2, 0x80000000, 0, 1)],
    "v_lshlrev_b64": [(n, 0x80000001, 0x80000001) for n in (0, 31, 32, 63, 64)],
    "v_alignbit_b32": [(0x12345678, 0x9ABCDEF0, n) for n in (0, 31, 32, 63)],
    "v_perm_b32": [(0x80FF7F01, 0x7F80FE02, 0x0C0B0A09), (0x80FF7F01, 0x7F80FE02, 0x08070400),
                   (0x80FF7F01, 0x7F80FE02, 0x0F0E0D03)],
    "v_bfe_u32": [(ONES, 0, 31), (ONES, 31, 1), (ONES, 31, 31), (ONES, 5, 0), (ONES, 32, 33)],
    "v_bfe_i32": [(ONES, 0, 31), (0x80000000, 31, 1), (0x80000000, 31, 31), (ONES, 5, 0),
                  (0x40000000, 30, 1), (0x40000000, 30, 2)],
    "v_bfi_b32": [(ONES, 0x12345678, 0), (0, 0x12345678, 0x9ABCDEF0)],
    "v_bcnt_u32_b32": [(ONES, ONES), (0, 0), (ONES, 0)],
    "v_ffbh_u32": [(0,), (1,), (0x80000000,), (ONES,)],
    "v_dot4_i32_i8": [(0x80808080, 0x80808080, 0), (0x7F7F7F7F, 0x80808080, 0x7FFFFFFF),
                      (0xFF01FF01, 0x01FF01FF, ONES)],
    "v_bitop3_b32.0x96": [(0xF0F0F0F0, 0xCCCCCCCC, 0xAAAAAAAA)],  # every truth-table row
    "v_bitop3_b32.0xe8": [(0xF0F0F0F0, 0xCCCCCCCC, 0xAAAAAAAA)],
    # f16: ties at 1 + 2^-11 (down) and 1 + 3 * 2^-11 (up); the largest finite
    "v_cvt_f16_f32": [(f32(1 + 2.0 ** -11),), (f32(1 + 3 * 2.0 ** -11),), (f32(65504.0),),
                      (f32(2.0 ** -14),)],
    "v_cvt_f32_f16": [(0x3C00,), (0x7BFF,), (0x0400,), (0xFBFF,)],
    "v_cvt_pk_bf16_f32": [(f32(1 + 2.0 ** -8), f32(1 + 3 * 2.0 ** -8)),
                          (f32(-(1 + 2.0 ** -8)), f32(1 + 2.0 ** -8 + U))],
    "v_cvt_f64_f32": [(f32(1 + U),), (f32(-2.0 ** -20),)],
    "v_cvt_f32_f64": [f64(1 + 2.0 ** -24), f64(1 + 3 * 2.0 ** -24), f64(-(1 + 2.0 ** -24))],
    "v_cvt_i32_f32": [(f32(1.5),), (f32(-1.5),), (f32(2.5),), (f32(0.75),),
                      (f32(-2147483648.0),), (f32(2147483520.0),)],
    "v_cvt_f32_u32": [(2 ** 24 + 1,), (2 ** 24 + 3,), (ONES,), (0,), (0xFFFFFF7F,), (0xFFFFFF80,)],
    # e4m3: ties at 1 + 2^-4 (down) and 1 + 3 * 2^-4 (up); 448 is the largest
    "v_cvt_pk_fp8_f32": [(f32(1 + 2.0 ** -4), f32(1 + 3 * 2.0 ** -4), 0xA5A5A5A5),
                         (f32(448.0), f32(-2.0 ** -6), 0x5A5A5A5A)],
    "v_cvt_pk_bf8_f32": [(f32(1 + 2.0 ** -3), f32(1 + 3 * 2.0 ** -3), 0xA5A5A5A5),
                         (f32(57344.0), f32(-2.0 ** -14), 0x5A5A5A5A)],
    "v_cvt_f32_fp8": [(0x7E017F80 & 0xFEFFFEFF,), (0x08F80778,)],
    "v_cvt_f32_bf8": [(0x7B01FB80,), (0x04840378,)],
    # e2m1 ties: 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4; scales 1/2, 1, 2
    "v_cvt_scalef32_pk_fp4_f32": [
        (f32(1.25), f32(1.75), f32(1.0), 0xA5A5A5A5), (f32(2.5), f32(-3.5), f32(1.0), 0x5A5A5A5A),
        (f32(2.5), f32(10.0), f32(2.0), 0), (f32(-1.25), f32(3.0), f32(0.5), ONES),
        (f32(6.0), f32(1.0), f32(1.0), 0)],
    "s_mul_i32": [(ONES, ONES), (0x10000, 0x10000), (0x80000000, ONES)],
    "s_mul_hi_u32": [(ONES, ONES), (0x10000, 0x10000), (0x80000000, 2)],
    # a carry out of the low word, and out of the high word
    "s_add_u32+s_addc_u32": [(ONES, 0, 1, 0), (ONES, ONES, 1, 0), (0x80000000, 1, 0x80000000, 1)],
    "s_lshl_b64": [(0x80000001, 0x80000001, n) for n in (0, 31, 32, 63, 64)],
    "s_bfe_u32": [(0x89ABCDEF, 32 << 16), (0x89ABCDEF, 1 << 16 | 31), (0x89ABCDEF, 4 << 16 | 28)],
    "s_bfe_i64": [(0x89ABCDEF, 0x81234567, 64 << 16), (0, 0x80000000, 1 << 16 | 63),
                  (0x89ABCDEF, 0x81234567, 32 << 16 | 32), (0x89ABCDEF, 0x81234567, 8 << 16 | 24)],
    "s_bcnt1_i32_b64": [(0, 0), (ONES, ONES), (1, 0x80000000)],
    "s_ff1_i32_b64": [(0, 0), (0, 0x80000000), (1, 0), (0, 1)],
    "s_flbit_i32_b64": [(0, 0), (0, 0x80000000), (1, 0), (ONES, 0)],
    "s_cselect_b32": [(ONES, 0, 1, 2), (0, ONES, 1, 2), (5, 5, 1, 2), (0x80000000, 0x7FFFFFFF, 1, 2)],
    "s_and_saveexec_b64": [(0, 0), (ONES, ONES), (0x80000001, 0x80000001), (1, 0)],
}


def waves_of(set_name, op):
    """The operand waves one op is run on: lists of 64 operand tuples."""
    ref = _REFS[set_name]
    base = next(vectors_of(ref, op))[0]
    corners = CORNERS.get(op["name"], [])
    if set_name == "salu":
        return [[tuple(c)] * 64 for c in corners + [base[0]]]
    if set_name != "xlane":
        assert corners, op["name"]
        return [[tuple(c) for c in corners] + [tuple(b) for b in base[len(corners):]]]
    # cross-lane: numpy-style stated data, pairwise distinct over a, b and old
    a = [0x0A000000 + 0x01010101 * l for l in range(64)]
    b = [0x0B000000 + 0x00010203 * l + 1 for l in range(64)]
    old = [0x0C000000 + 0x01000001 * l + 2 for l in range(64)]
    name = op["mnemonic"]
    if name in ("ds_bpermute_b32", "ds_permute_b32"):
        # every edge lane is source and target: the reversal, and a rotation
        # by 16 with stray bits around the lane select
        waves = [[(a[l], (63 - l) * 4) for l in range(64)],
                 [(a[l], ((l + 16) % 64) * 4 | 0x3 | 0xABCD00 << 8) for l in range(64)]]
        if name == "ds_bpermute_b32":  # not a permutation: all read an edge lane
            waves += [[(a[l], EDGE_LANES[l % 6] * 4) for l in range(64)]]
        return waves
    if name == "v_readlane_b32":
        return [[(a[l], sel | 0xFFFFFFC0 * (sel & 1)) for l in range(64)] for sel in EDGE_LANES]
    if name == "v_writelane_b32":
        return [[(a[l], sel, old[l]) for l in range(64)] for sel in EDGE_LANES]
    if name == "v_readfirstlane_b32":
        return [[(a[l],) for l in range(64)]]
    if op["widths"][3]:  # DPP: a and old
        return [[(a[l], old[l]) for l in range(64)]]
    if op["widths"][1]:  # the swaps: a and b
        return [[(a[l], b[l]) for l in range(64)]]
    return [[(a[l],) for l in range(64)]]  # the swizzles


def test_the_op_list_is_whole():
    if _MOD is None:
        pytest.skip("_healthprobe extension not built")
    names = {op["name"] for _, op in OPS}
    assert MUST_HAVE <= names
    assert XLANE_MNEMONICS <= {op["mnemonic"] for op in _REFS["xlane"]["ops"]}
    for s in ("fma", "int", "cvt", "xlane"):
        assert len(_REFS[s]["ops"]) >= 8
    assert names - set(REFERENCE) == {op["name"] for op in _REFS["trans"]["ops"]}
    # every corner list belongs to an op
    assert set(CORNERS) <= names


@pytest.mark.parametrize("set_name,op", KNOWN_ANSWER_OPS or [pytest.param(
    None, None, marks=pytest.mark.skip(reason="_healthprobe extension not built"))],
    ids=[op["name"] for _, op in KNOWN_ANSWER_OPS] or None)
def test_valu_raw_equals_the_reference(mod, set_name, op):
    for wave in waves_of(set_name, op):
        lanes = wave[:1] if set_name == "salu" else wave
        want = [tuple(w) for w in REFERENCE[op["name"]](lanes)]
        if set_name == "salu":
            want = want * 64
        got = [tuple(g) for g in run_raw(mod, op, wave)]
        bad = [(l, wave[l], got[l], want[l]) for l in range(64) if got[l] != want[l]]
        print(op["name"], len(bad), "lanes differ")
        assert not bad, bad[:4]


def test_cross_lane_waves_touch_every_edge_lane():
    """Lanes 0, 15, 16, 31, 32 and 63 are a source and a target somewhere in
    every cross-lane op's waves, by the reference's own data flow."""
    if _MOD is None:
        pytest.skip("_healthprobe extension not built")
    for op in _REFS["xlane"]["ops"]:
        sources, targets = set(), set()
        for wave in waves_of("xlane", op):
            owner = {lane[0]: l for l, lane in enumerate(wave)}
            if op["widths"][1] and op["mnemonic"].startswith("v_permlane"):
                owner.update({lane[1]: l for l, lane in enumerate(wave)})
            for l, regs in enumerate(REFERENCE[op["name"]](wave)):
                for word in regs:
                    if word in owner and (owner[word] != l or op["regs"] == 2):
                        sources.add(owner[word])
                        targets.add(l)
        fixed_pattern = op["mnemonic"] in ("v_mov_b32_dpp", "ds_swizzle_b32",
                                           "v_readfirstlane_b32") or \
            op["mnemonic"].startswith("v_permlane")
        if fixed_pattern:
            # the instruction's own pattern decides; every lane is compared
            assert targets and sources, op["name"]
        elif op["mnemonic"] == "v_readlane_b32":
            assert set(EDGE_LANES) <= sources, op["name"]
        elif op["mnemonic"] == "v_writelane_b32":
            # the written lane is the one that no longer holds old
            written = {l for wave in waves_of("xlane", op)
                       for l, regs in enumerate(REFERENCE[op["name"]](wave))
                       if regs[0] != wave[l][2]}
            assert set(EDGE_LANES) <= written, op["name"]
        else:
            assert set(EDGE_LANES) <= sources and set(EDGE_LANES) <= targets, op["name"]


def test_a_row_mask_keeps_old(mod):
    op = next(o for o in _REFS["xlane"]["ops"]
              if o["name"] == "v_mov_b32_dpp.quad_perm_3301_row_mask_5")
    wave = waves_of("xlane", op)[0]
    got = run_raw(mod, op, wave)
    kept = [l for l in range(64) if got[l][0] == wave[l][1]]
    assert kept == list(range(16, 32)) + list(range(48, 64))  # rows 1 and 3


def test_trans_valu_raw_equals_the_recorded_file(mod):
    ref = _REFS["trans"]
    for op in ref["ops"]:
        for t, (ins, exp) in enumerate(vectors_of(ref, op)):
            got = [tuple(g) for g in run_raw(mod, op, ins)]
            assert got == [tuple(e) for e in exp], (op["name"], t)


@pytest.fixture(scope="module")
def healthy(mod):
    """One default sweep per set, shared."""
    return {s: mod.valu_sweep(0, 0, None, s) for s in SETS}


@pytest.mark.parametrize("op_set", SETS)
def test_healthy_sweep(mod, healthy, op_set):
    res = healthy[op_set]
    print(op_set, "sweep_ms", res["sweep_ms"], "launches", res["launches"])
    assert res["ok"] and res["bad"] == []
    assert res["coverage_complete"] and res["uncovered"] == []
    assert res["cus_covered"] == res["cu_count"]
    assert res["simds_covered"] == 4 * res["cu_count"]
    assert 1 <= res["launches"] <= 4
    assert res["op_set"] == op_set
    assert res["ops"] == [op["name"] for op in _REFS[op_set]["ops"]]
    assert res["reps"] >= _REFS[op_set]["default_reps"]
    assert set(res) >= {"ok", "coverage_complete", "cus_covered", "simds_covered",
                        "uncovered", "launches", "reps", "sweep_ms", "bad", "records"}


@pytest.mark.parametrize("op_set", SETS)
@pytest.mark.parametrize("where", ["first", "last"])
def test_injection_reports_exactly_that_simd(mod, healthy, op_set, where):
    ops = _REFS[op_set]["ops"]
    cu_count = healthy[op_set]["cu_count"]
    block, wave, index = (0, 0, 0) if where == "first" else (cu_count - 1, 3, len(ops) - 1)
    lane, reg, bit = _REFS[op_set]["inject"]
    res = mod.valu_sweep(0, 0, (block, wave, index), op_set)
    assert not res["ok"] and len(res["bad"]) == 1
    bad = res["bad"][0]
    # the SIMD that block's wave recorded, in the first launch
    hw_id, xcc_id = res["records"][block * 4 + wave][:2]
    assert (bad["xcc"], bad["se"], bad["sh"], bad["cu"], bad["simd"]) == \
        tuple(mod.decode_hw_id(hw_id, xcc_id))
    assert bad["ops"] == [ops[index]["name"]]
    assert bad["bad_lanes"] == 1 << lane
    first = bad["first"]
    assert first["op"] == ops[index]["name"] and first["t"] == 0
    assert first["lane"] == lane and first["reg"] == min(reg, ops[index]["regs"] - 1)
    assert first["got"] ^ first["expected"] == bit


def test_deep_health_probe(mod, monkeypatch):
    for env in (native.VALU_SWEEP_ENV, native.VALU_SWEEP_INJECT_ENV,
                native.CU_SWEEP_ENV, native.CU_SWEEP_INJECT_ENV):
        monkeypatch.delenv(env, raising=False)
    hbm = 1 << 26
    res = native.deep_health_probe(hbm_bytes=hbm)
    assert "valu_sweep" not in res and res["healthy"]

    res = native.deep_health_probe(hbm_bytes=hbm, valu_sweep="all", cu_sweep=True)
    assert res["healthy"], res["floor_violations"]
    assert tuple(res["valu_sweep"]) == SETS
    for s in SETS:
        assert res["valu_sweep"][s]["ok"] and res["valu_sweep"][s]["coverage_complete"]
    assert "warnings" not in res
    # the base CU sweep's result is what it was
    direct = mod.cu_sweep(0)
    base = res["cu_sweep"]
    assert base["ok"] and base["coverage_complete"] and base["pipe_set"] == "base"
    assert base["pipes"] == list(native.CU_SWEEP_PIPES["base"])
    assert set(base) == set(direct) == {
        "cu_count", "cus_covered", "simds_covered", "coverage_complete", "launches",
        "reps", "waves_checked", "pipe_set", "pipes", "bad", "uncovered", "records",
        "sweep_ms", "ok"}

    monkeypatch.setenv(native.VALU_SWEEP_INJECT_ENV, "1:2:v_cvt_pk_bf16_f32")
    res = native.deep_health_probe(hbm_bytes=hbm, valu_sweep="cvt,fma")
    assert not res["healthy"] and res["valu_sweep"]["fma"]["ok"]
    assert len(res["floor_violations"]) == 1
    line = res["floor_violations"][0]
    assert line.startswith("valu_sweep: xcc ") and line.endswith(" failed v_cvt_pk_bf16_f32")

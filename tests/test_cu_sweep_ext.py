"""The CU sweep's extra pipe sets, CPU side: the mx and wide known-answer
tables recomputed from their PACKED bytes with decoders written here from
the format definitions, the host table code under the sanitizers, argument
checks, the health policy and the plugin wiring (stubbed module).

The sweeps themselves run on the GPU: tests/test_cu_sweep_ext_gpu.py.
"""

import os
import shutil
import struct
import subprocess
from fractions import Fraction

import pytest

import k8s_device_plugin_amd.native as native
from k8s_device_plugin_amd.native import build as nb
from k8s_device_plugin_amd.plugin import AMDGPUPlugin
from k8s_device_plugin_amd.protos import deviceplugin as dp
from k8s_device_plugin_amd.testing.fakesysfs import build_mi355x_node

from deep_probe_stubs import Ctx as _Ctx
from deep_probe_stubs import dev_root as _dev_root
from deep_probe_stubs import cpx_plugin, gauge, stub_probe  # noqa: F401

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_DIR = os.path.join(REPO, "k8s_device_plugin_amd", "native")

BASE = ["bf16_16", "bf16_32", "f16_16", "fp8_16", "i8_16", "mxfp8_16"]
# name -> (M, N, K, A format, B format, result)
MX = {
    "mxfp4_16": (16, 16, 128, "fp4_e2m1", "fp4_e2m1", "f32"),
    "mxfp4_32": (32, 32, 64, "fp4_e2m1", "fp4_e2m1", "f32"),
    "mxfp6_16": (16, 16, 128, "fp6_e2m3", "fp6_e2m3", "f32"),
    "mxbf6_16": (16, 16, 128, "bf6_e3m2", "bf6_e3m2", "f32"),
    "mxfp8xfp4_16": (16, 16, 128, "fp8_e4m3", "fp4_e2m1", "f32"),
}
WIDE = {
    "bf8_16": (16, 16, 32, "bf8_e5m2", "bf8_e5m2", "f32"),
    "f16_32": (32, 32, 16, "f16", "f16", "f32"),
    "fp8_32": (32, 32, 16, "fp8_e4m3", "fp8_e4m3", "f32"),
    "i8_32": (32, 32, 32, "i8", "i8", "i32"),
    "f64_16": (16, 16, 4, "f64", "f64", "f64"),
    "f32_16": (16, 16, 4, "f32", "f32", "f32"),
}
SETS = {"mx": MX, "wide": WIDE}

# format -> (bits, exponent bits, mantissa bits, bias)
FORMATS = {
    "fp4_e2m1": (4, 2, 1, 1), "fp6_e2m3": (6, 2, 3, 1),
    "bf6_e3m2": (6, 3, 2, 3), "fp8_e4m3": (8, 4, 3, 7),
    "bf8_e5m2": (8, 5, 2, 15), "f16": (16, 5, 10, 15),
    "f32": (32, 8, 23, 127), "f64": (64, 11, 52, 1023), "i8": (8, 0, 0, 0),
}
# Documented in docs/health.md: the OR of all element codes a format's
# tables use (every bit that is 1 somewhere); their AND is 0 for every
# format (every bit is 0 somewhere).  f32 and f64 cannot toggle their low
# mantissa bits within the exactness bound.
TOGGLED = {
    "fp4_e2m1": 0xF, "fp6_e2m3": 0x3F, "bf6_e3m2": 0x3F, "fp8_e4m3": 0xFF,
    "bf8_e5m2": 0xFF, "i8": 0xFF, "f16": 0xFFFF, "f32": 0xFFFFE000,
    "f64": 0xFFFFFFFFE0000000,
}
BOUND = {"f32": 1 << 23, "i32": 1 << 31, "f64": 1 << 52}


def decode(fmt, code):
    """The exact value of an element code, from the format's definition."""
    bits, e_bits, m_bits, bias = FORMATS[fmt]
    if fmt == "i8":
        return Fraction(code - 256 if code & 0x80 else code)
    sign = -1 if code >> (bits - 1) & 1 else 1
    e = code >> m_bits & ((1 << e_bits) - 1)
    m = code & ((1 << m_bits) - 1)
    # no NaN or infinity in the tables: e4m3 has one NaN code per sign, the
    # IEEE-like formats reserve the top exponent, fp4 and fp6 have neither
    if fmt == "fp8_e4m3":
        assert code & 0x7F != 0x7F
    elif fmt not in ("fp4_e2m1", "fp6_e2m3", "bf6_e3m2"):
        assert e != (1 << e_bits) - 1
    if e == 0:
        return sign * Fraction(m, 1 << m_bits) * Fraction(2) ** (1 - bias)
    return sign * (1 + Fraction(m, 1 << m_bits)) * Fraction(2) ** (e - bias)


def _times_2_16(x):
    y = Fraction(x) * (1 << 16)
    assert y.denominator == 1
    return int(y)


def e8m0(byte):
    assert byte != 0xFF  # NaN
    return Fraction(2) ** (byte - 127)


def elements(fmt, frag, lane, frag_bytes, count):
    """The codes of a lane's fragment: element j is bits [j * bits,
    (j + 1) * bits) of the fragment as one little-endian bit string."""
    bits = FORMATS[fmt][0]
    word = int.from_bytes(frag[lane * frag_bytes:(lane + 1) * frag_bytes], "little")
    return [word >> (j * bits) & ((1 << bits) - 1) for j in range(count)]


def result_row(m, result, lane, r):
    """C/D lane maps; f64 has its own."""
    if result == "f64":
        return (lane >> 4) + 4 * r
    if m == 16:
        return 4 * (lane >> 4) + r
    return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)


def result_words(result, value):
    """The result registers of an exactly representable value."""
    if result == "i32":
        assert value.denominator == 1
        return [int(value) & 0xFFFFFFFF]
    if result == "f32":
        raw = struct.pack("<f", float(value))
        assert Fraction(struct.unpack("<f", raw)[0]) == value
        return [struct.unpack("<I", raw)[0]]
    assert Fraction(float(value)) == value
    lo, hi = struct.unpack("<II", struct.pack("<d", float(value)))
    return [lo, hi]  # low word first


# ---------------- reference tables (need the built extension) ----------------


@pytest.fixture(scope="module")
def probe_mod():
    try:  # torch's HIP runtime must load first (see __graft_entry__.build)
        import torch  # noqa: F401
    except ImportError:
        pass
    mod = native.load_healthprobe(required=False)
    if mod is None:
        pytest.skip("_healthprobe.so not built (no hipcc)")
    return mod


@pytest.fixture(scope="module")
def references(probe_mod):
    return {s: probe_mod.cu_sweep_reference(s) for s in SETS}


def _k_of(pipe, fmt, group, j):
    """The operand map: element j of lane group `group` is slot
    group * J + j, and A's (group, j) meets B's (group, j).  One exception,
    measured on MI355X: an 8-bit operand of the scaled 16x16x128 form holds
    k = 16 group + j (j < 16) and 64 + 16 group + (j - 16), a 4-bit one
    k = 32 group + j, and the two meet by k; the block scale of lane group g
    belongs to k = 32 g .. 32 g + 31."""
    m, _, k, fmt_a, fmt_b, _ = pipe["shape"]
    j_per_lane = k // (64 // m)
    if pipe["name"].startswith("mx") and fmt_a != fmt_b and FORMATS[fmt][0] == 8:
        return 16 * group + j if j < 16 else 64 + 16 * group + (j - 16)
    return group * j_per_lane + j


def _matrices(pipe, test, scaled):
    """A [M][K], B [K][N] as exact values by slot, and the per-block scale
    exponents sa [M][groups], sb [N][groups], from the packed bytes."""
    m, n, k, fmt_a, fmt_b, _ = pipe["shape"]
    groups = 64 // m
    j_per_lane = k // groups
    fa, fb = pipe["frag_bytes_a"], pipe["frag_bytes_b"]
    assert fa == j_per_lane * FORMATS[fmt_a][0] // 8
    assert fb == j_per_lane * FORMATS[fmt_b][0] // 8
    assert len(test["a_frag"]) == 64 * fa and len(test["b_frag"]) == 64 * fb
    a = [[None] * k for _ in range(m)]
    b = [[None] * n for _ in range(k)]
    codes = {fmt_a: [], fmt_b: []}
    sa = [[0] * groups for _ in range(m)]
    sb = [[0] * groups for _ in range(n)]
    for lane in range(64):
        rc, g = lane % m, lane // m
        ca = elements(fmt_a, test["a_frag"], lane, fa, j_per_lane)
        cb = elements(fmt_b, test["b_frag"], lane, fb, j_per_lane)
        codes[fmt_a] += ca
        codes[fmt_b] += cb
        for j in range(j_per_lane):
            a[rc][_k_of(pipe, fmt_a, g, j)] = decode(fmt_a, ca[j])
            b[_k_of(pipe, fmt_b, g, j)][rc] = decode(fmt_b, cb[j])
        if scaled:
            sel_a, sel_b = test["sel"]
            sa[rc][g] = test["scale_a"][lane] >> (8 * sel_a) & 0xFF
            sb[rc][g] = test["scale_b"][lane] >> (8 * sel_b) & 0xFF
    return a, b, sa, sb, codes


@pytest.mark.parametrize("pipe_set", ["mx", "wide"])
def test_expected_bits_are_the_exact_product_of_the_packed_bytes(references,
                                                                 pipe_set):
    ref = references[pipe_set]
    assert [p["name"] for p in ref["pipes"]] == list(SETS[pipe_set])
    assert ref["tests_per_pipe"] == 6
    # one block per CU: each set fits the LDS and the launch asks for more
    # than half of it
    assert ref["table_bytes"] <= 160 * 1024 == 163840
    assert ref["lds_bytes"] >= max(ref["table_bytes"], 80 * 1024 + 16)
    assert len(ref["table"]) == ref["table_bytes"]
    scaled = pipe_set == "mx"
    used = {}
    for p in ref["pipes"]:
        shape = SETS[pipe_set][p["name"]]
        m, n, k, fmt_a, fmt_b, result = shape
        assert (p["M"], p["N"], p["K"], p["a_format"], p["b_format"],
                p["result"]) == shape
        words = 2 if result == "f64" else 1
        assert p["regs"] == m * n // 64 * words
        p = dict(p, shape=shape)
        groups, j_per_lane = 64 // m, k // (64 // m)
        if scaled:
            assert j_per_lane == 32  # one lane holds exactly one MX block
        assert len(p["tests"]) == 6
        for t, test in enumerate(p["tests"]):
            where = f"{p['name']} t={t}"
            a, b, sa, sb, codes = _matrices(p, test, scaled)
            for fmt, cs in codes.items():
                used.setdefault(fmt, []).extend(cs)
            # exact integer arithmetic: every operand and every scale is a
            # multiple of 2^-16 (checked), so a product is one of 2^-48
            a = [[_times_2_16(x) for x in row] for row in a]
            b = [[_times_2_16(x) for x in row] for row in b]
            d = [[Fraction(0)] * n for _ in range(m)]
            unit = (1 << 48) >> test["unit_shift"]
            assert unit << test["unit_shift"] == 1 << 48
            worst = 0
            for i in range(m):
                for j in range(n):
                    total = abs_total = 0
                    for g in range(groups):
                        scale = _times_2_16(
                            e8m0(sa[i][g]) * e8m0(sb[j][g]) if scaled else 1)
                        for s in range(g * j_per_lane, (g + 1) * j_per_lane):
                            prod = a[i][s] * b[s][j] * scale
                            # (c): every product a multiple of one unit
                            assert prod % unit == 0, where
                            total += prod
                            abs_total += abs(prod)
                    d[i][j] = Fraction(total, 1 << 48)
                    worst = max(worst, abs_total // unit)
            # (c): sum |a b| scale / u below the result's exact range
            assert worst < BOUND[result], where
            assert worst == test["abs_sum_max"], where

            # a swapped, duplicated or shifted lane cannot give this tile
            assert len({tuple(r) for r in d}) == m, where
            assert len({tuple(c) for c in zip(*d)}) == n, where
            assert any(d[i][j] != d[j][i] for i in range(m) for j in range(n)), where

            # every result register of every lane, through the lane maps
            for lane in range(64):
                want = []
                for r in range(m * n // 64):
                    want += result_words(
                        result, d[result_row(m, result, lane, r)][lane % n])
                assert test["expected_bits"][lane] == want, (where, lane)

            # the blob holds the test where the kernel reads it
            at = test["offset"]
            for part in (test["a_frag"], test["b_frag"]):
                assert ref["table"][at:at + len(part)] == part, where
                at += len(part)
            if scaled:
                for part in (test["scale_a"], test["scale_b"]):
                    assert ref["table"][at:at + 256] == struct.pack("<64I", *part)
                    at += 256
            flat = [w for lane in test["expected_bits"] for w in lane]
            assert ref["table"][at:at + 4 * len(flat)] == struct.pack(
                f"<{len(flat)}I", *flat), where

    # (b): every bit of the element code is 1 somewhere and 0 somewhere
    for fmt, cs in used.items():
        every_or, every_and = 0, (1 << FORMATS[fmt][0]) - 1
        for c in cs:
            every_or |= c
            every_and &= c
        assert every_or == TOGGLED[fmt], (fmt, hex(every_or))
        assert every_and == 0, (fmt, hex(every_and))


def test_i8_uses_the_whole_range_and_f64_24_bit_integers(references):
    ref = references["wide"]
    by_name = {p["name"]: p for p in ref["pipes"]}
    i8, f64 = set(), []
    for test in by_name["i8_32"]["tests"]:
        i8 |= set(test["a_frag"]) | set(test["b_frag"])
    assert {0x80, 0x7F} <= i8 and len(i8) == 256
    for test in by_name["f64_16"]["tests"]:
        for lane in range(64):
            f64 += [decode("f64", c) for c in elements("f64", test["a_frag"], lane, 8, 1)]
    assert all(v.denominator == 1 and abs(v) < 1 << 24 for v in f64)
    assert max(abs(v) for v in f64) >= 1 << 23


def test_mx_scales_decoys_and_selects(references):
    ref = references["mx"]
    for p in ref["pipes"]:
        sels_a, sels_b = set(), set()
        for t, test in enumerate(p["tests"]):
            sel_a, sel_b = test["sel"]
            sels_a.add(sel_a)
            sels_b.add(sel_b)
            true_scales = {"a": {}, "b": {}}
            for side, sel in (("a", sel_a), ("b", sel_b)):
                words = test["scale_" + side]
                assert len(words) == 64
                for lane, word in enumerate(words):
                    lanes = [word >> (8 * k) & 0xFF for k in range(4)]
                    truth = lanes[sel]
                    assert 120 <= truth <= 134  # a small range around 127
                    true_scales[side][lane] = truth
                    for k in range(4):
                        if k != sel:  # off by a factor >= 256
                            assert abs(lanes[k] - truth) >= 8, (p["name"], t, lane)
                            assert lanes[k] != 0xFF
                # the scales are live: more than one value, and the blocks of
                # one row do not all share one
                assert len(set(true_scales[side].values())) > 1
            m = p["M"]
            rows_with_mixed_scales = sum(
                len({true_scales["a"][g * m + i] for g in range(64 // m)}) > 1
                for i in range(m))
            assert rows_with_mixed_scales > m // 2, (p["name"], t)
        # each of the four byte selects on each side at least once
        assert sels_a == sels_b == {0, 1, 2, 3}, p["name"]


def test_pad_bytes_after_narrow_fragments_are_not_zero(references):
    """The kernel loads 32 bytes where an fp4 / fp6 fragment has 16 / 24: the
    rest is whatever follows in the table, and it is not all zero."""
    ref = references["mx"]
    table = ref["table"]
    for p in ref["pipes"]:
        for test in p["tests"]:
            for which, fb in (("a", p["frag_bytes_a"]), ("b", p["frag_bytes_b"])):
                if fb == 32:
                    continue
                at = test["offset"] + (64 * p["frag_bytes_a"] if which == "b" else 0)
                pads = [table[at + lane * fb + fb:at + lane * fb + 32]
                        for lane in range(64)]
                assert all(len(x) == 32 - fb for x in pads)  # inside the table
                assert sum(any(x) for x in pads) > 48, (p["name"], which)


def test_base_reference_is_unchanged(probe_mod):
    base = probe_mod.cu_sweep_reference()
    assert base == probe_mod.cu_sweep_reference("base")
    assert [p["name"] for p in base["pipes"]] == BASE
    assert "pipe_set" not in base


def test_sweep_table_ext_is_a_build_input():
    assert os.path.join(nb.PKG_DIR, "sweep_table_ext.h") in nb._HIP_HEADERS


@pytest.mark.parametrize("kwargs", [
    {"pipe_set": "fp4"},
    {"pipe_set": ""},
    {"pipe_set": "mx", "inject": (0, 0, 5)},    # mx has 5 pipes
    {"pipe_set": "wide", "inject": (0, 0, 6)},  # wide has 6
    {"pipe_set": "base", "inject": (0, 0, 6)},
    {"pipe_set": "mx", "reps": -1},
])
def test_cu_sweep_rejects_bad_arguments(probe_mod, kwargs):
    """Rejected before any HIP call, so it holds without a GPU."""
    with pytest.raises(ValueError):
        probe_mod.cu_sweep(device=0, **kwargs)
    with pytest.raises(ValueError):
        probe_mod.cu_sweep_reference("sparse")


@pytest.mark.parametrize("args,kwargs", [
    (("mxfp4_17", bytes(1024), bytes(1024)), {}),              # unknown pipe
    (("mxfp4_16", bytes(1023), bytes(1024)), {}),              # A too short
    (("mxfp6_16", bytes(1536), bytes(2048)), {}),              # B too long
    (("mxfp8xfp4_16", bytes(1024), bytes(2048)), {}),          # swapped widths
    (("f64_16", bytes(512), bytes(256)), {}),
    (("mxfp4_16", bytes(1024), bytes(1024)), {"scale_a": bytes(64)}),
    (("mxfp4_16", bytes(1024), bytes(1024)), {"sel": (4, 0)}),
    (("f32_16", bytes(256), bytes(256)), {"scale_a": bytes(256)}),
])
def test_mfma_raw_rejects_bad_arguments(probe_mod, args, kwargs):
    """Names and lengths are checked before any HIP call."""
    with pytest.raises(ValueError):
        probe_mod.mfma_raw(0, *args, **kwargs)


# ---------------- host table code under the sanitizers ----------------


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_sweep_table_ext_under_sanitizers(tmp_path):
    """A stand-alone program (its own main) builds both tables and derives
    each expected word a second way from the packed bytes, under ASan +
    UBSan."""
    exe = str(tmp_path / "sweep_table_ext_check")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-static-libasan",
         "-static-libubsan", f"-I{NATIVE_DIR}",
         os.path.join(REPO, "tests", "native", "sweep_table_ext_check.cpp"),
         "-o", exe],
        check=True, capture_output=True, text=True,
    )
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ok" in run.stdout


# ---------------- policy (stubbed probe module) ----------------


def _sweep_result(pipe_set="base", bad=(), cu_count=256, cus_covered=None,
                  simds_covered=None):
    cus = cu_count if cus_covered is None else cus_covered
    simds = 4 * cus if simds_covered is None else simds_covered
    out = {
        "cu_count": cu_count,
        "cus_covered": cus,
        "simds_covered": simds,
        "coverage_complete": cus == cu_count and simds == 4 * cu_count,
        "launches": 1,
        "reps": 8,
        "waves_checked": 4 * cu_count,
        "pipe_set": pipe_set,
        "pipes": list(native.CU_SWEEP_PIPES[pipe_set]),
        "bad": list(bad),
        "uncovered": [],
        "records": [],
        "sweep_ms": 0.1,
        "ok": not bad,
    }
    return out


def _bad_simd(pipe, simd=2):
    return {
        "xcc": 3, "se": 1, "sh": 0, "cu": 7, "simd": simd, "pipes": [pipe],
        "bad_lanes": 1 << 5,
        "first": {"pipe": pipe, "t": 0, "lane": 5, "reg": 1,
                  "got": 0x41000008, "expected": 0x41000000},
    }


class _BaseOnlyStub:
    """The module as the base-only tests stub it: cu_sweep takes no
    pipe_set."""

    def __init__(self, bus_ids=()):
        self.calls = []
        self.sweeps = []  # (device, inject)
        self.bus_ids = list(bus_ids)

    def run_probe(self, device=0, hbm_bytes=0):
        self.calls.append(device)
        return {"wave_ok": True, "mfma_ok": True, "lds_ok": True,
                "hbm_copy_ok": True, "mfma_tflops": 2000.0,
                "hbm_gbps": 6200.0, "healthy": True}

    def cu_sweep(self, device=0, reps=0, inject=None):
        self.sweeps.append((device, inject))
        return _sweep_result()

    def pci_bus_ids(self):
        return self.bus_ids


class _ExtStub(_BaseOnlyStub):
    def __init__(self, results=None, bus_ids=()):
        super().__init__(bus_ids)
        self.results = results or {}  # (ordinal, pipe_set) -> sweep dict
        self.sweeps = []  # (device, pipe_set, inject)

    def cu_sweep(self, device=0, reps=0, inject=None, pipe_set="base"):
        self.sweeps.append((device, pipe_set, inject))
        return self.results.get((device, pipe_set)) or _sweep_result(pipe_set)


def test_extra_sets_are_off_by_default(stub_probe):
    mod = stub_probe(_BaseOnlyStub())  # would raise on a pipe_set keyword
    res = native.deep_health_probe(device=2, cu_sweep=True)
    assert mod.sweeps == [(2, None)]
    assert res["healthy"] and "cu_sweep_extra" not in res

    # and they need the CU sweep itself
    mod = stub_probe(_ExtStub())
    res = native.deep_health_probe(cu_sweep=False, cu_sweep_extra="all")
    assert mod.sweeps == [] and "cu_sweep_extra" not in res
    res = native.deep_health_probe(cu_sweep_extra="all")
    assert mod.sweeps == [] and "cu_sweep_extra" not in res


@pytest.mark.parametrize("arg,want", [
    ("all", ["mx", "wide"]),
    (["wide", "mx"], ["mx", "wide"]),
    (("wide",), ["wide"]),
    ("mx", ["mx"]),
    ("mx, wide", ["mx", "wide"]),
    ((), []),
    ("", []),
])
def test_extra_argument(stub_probe, arg, want):
    mod = stub_probe(_ExtStub())
    res = native.deep_health_probe(device=1, cu_sweep=True, cu_sweep_extra=arg)
    assert mod.sweeps == [(1, "base", None)] + [(1, s, None) for s in want]
    assert res["healthy"] and "warnings" not in res
    assert res["cu_sweep"]["pipes"] == BASE
    assert list(res.get("cu_sweep_extra", {})) == want
    for s in want:
        assert res["cu_sweep_extra"][s]["pipes"] == list(SETS[s])


def test_extra_env(stub_probe, monkeypatch):
    mod = stub_probe(_ExtStub())
    for value, want in (("", []), ("all", ["mx", "wide"]), ("wide", ["wide"]),
                        ("wide,mx", ["mx", "wide"])):
        monkeypatch.setenv(native.CU_SWEEP_EXTRA_ENV, value)
        mod.sweeps.clear()
        native.deep_health_probe(cu_sweep=True)
        assert [s for _, s, _ in mod.sweeps] == ["base"] + want, value
    # an explicit argument wins over the environment
    mod.sweeps.clear()
    native.deep_health_probe(cu_sweep=True, cu_sweep_extra=())
    assert [s for _, s, _ in mod.sweeps] == ["base"]


@pytest.mark.parametrize("bad", ["sparse", "mx,sparse", ["mx", "base"], "all,mx"])
def test_unknown_extra_set_is_an_error(stub_probe, monkeypatch, bad):
    stub_probe(_ExtStub())
    with pytest.raises(ValueError, match="cu_sweep_extra"):
        native.deep_health_probe(cu_sweep=True, cu_sweep_extra=bad)
    if isinstance(bad, str):
        monkeypatch.setenv(native.CU_SWEEP_EXTRA_ENV, bad)
        with pytest.raises(ValueError, match="cu_sweep_extra"):
            native.deep_health_probe(cu_sweep=True)


def test_bad_simd_in_an_extra_set_is_unhealthy_and_named(stub_probe):
    stub_probe(_ExtStub({(0, "mx"): _sweep_result("mx", [_bad_simd("mxfp4_16")])}))
    res = native.deep_health_probe(cu_sweep=True, cu_sweep_extra="all")
    assert not res["healthy"]
    assert res["floor_violations"] == [
        "cu_sweep: xcc 3 se 1 cu 7 simd 2 failed mxfp4_16"]
    assert res["cu_sweep"]["ok"] and res["cu_sweep_extra"]["wide"]["ok"]
    assert not res["cu_sweep_extra"]["mx"]["ok"]


def test_incomplete_but_clean_extra_set_only_warns(stub_probe):
    stub_probe(_ExtStub({
        (0, "mx"): _sweep_result("mx", cus_covered=250),
        (0, "base"): _sweep_result("base", cus_covered=255)}))
    res = native.deep_health_probe(cu_sweep=True, cu_sweep_extra=["mx"])
    assert res["healthy"] and res["floor_violations"] == []
    assert res["warnings"] == [
        "cu_sweep_incomplete: 255 of 256 CUs, 1020 SIMDs",
        "cu_sweep_incomplete[mx]: 250 of 256 CUs, 1000 SIMDs"]


@pytest.mark.parametrize("spec,want", [
    ("1:1:mxfp6_16", {"mx": (1, 1, 2)}),
    ("255:3:f32_16", {"wide": (255, 3, 5)}),
    ("0:0:i8_16", {"base": (0, 0, 4)}),
    ("7:2:3", {"base": (7, 2, 3)}),
])
def test_inject_by_name_reaches_the_set_that_owns_it(stub_probe, monkeypatch,
                                                     spec, want):
    mod = stub_probe(_ExtStub())
    monkeypatch.setenv(native.CU_SWEEP_INJECT_ENV, spec)
    native.deep_health_probe(cu_sweep=True, cu_sweep_extra="all")
    assert mod.sweeps == [(0, s, want.get(s)) for s in ("base", "mx", "wide")]


@pytest.mark.parametrize("spec", ["1:1:mxfp6", "1:mxfp6_16", "a:1:mxfp6_16"])
def test_inject_env_errors(stub_probe, monkeypatch, spec):
    stub_probe(_ExtStub())
    monkeypatch.setenv(native.CU_SWEEP_INJECT_ENV, spec)
    with pytest.raises(ValueError, match="block:wave:pipe"):
        native.deep_health_probe(cu_sweep=True)


# ---------------- plugin, metrics, CLI ----------------


def _cpx_plugin(tmp_path, stub_probe, results=None, **kwargs):
    return cpx_plugin(tmp_path, stub_probe,
                      lambda bus_ids: _ExtStub(results, bus_ids), **kwargs)


def _gauge(plugin):
    return [v for _, v in gauge(plugin, "amdgpu_dp_deep_probe_bad_simds")]


def test_plugin_runs_the_extra_sets_on_every_ordinal(tmp_path, stub_probe):
    plugin, mod, _ = _cpx_plugin(tmp_path, stub_probe, deep_probe_every=1,
                                 deep_cu_sweep=True,
                                 deep_cu_sweep_extra=("mx", "wide"))
    plugin.heartbeat()
    assert mod.calls == [0, 4]
    assert [(d, s) for d, s, _ in mod.sweeps] == [
        (d, s) for d in range(8) for s in ("base", "mx", "wide")]
    assert not plugin._deep_failed and _gauge(plugin) == [0.0]
    plugin.stop()


def test_plugin_without_the_extra_flag_passes_no_pipe_set(tmp_path, stub_probe):
    fs = build_mi355x_node(str(tmp_path / "n"), n_gpus=1)
    plugin = AMDGPUPlugin(resource="gpu", paths=fs.paths,
                          dev_root=_dev_root(tmp_path), deep_probe_every=1,
                          deep_cu_sweep=True)
    plugin.start()
    mod = stub_probe(_BaseOnlyStub())
    plugin.heartbeat()
    assert mod.sweeps == [(0, None)] and not plugin._deep_failed
    plugin.stop()


def test_plugin_bad_simd_in_an_extra_set_pins_the_gpu(tmp_path, stub_probe,
                                                      caplog):
    # ordinal 5 (GPU 1): the same SIMD fails in mx and in wide, another in wide
    results = {
        (5, "mx"): _sweep_result("mx", [_bad_simd("mxfp4_32")], cu_count=32),
        (5, "wide"): _sweep_result(
            "wide", [_bad_simd("f64_16"), _bad_simd("bf8_16", simd=0)],
            cu_count=32),
    }
    plugin, mod, phys = _cpx_plugin(tmp_path, stub_probe, results,
                                    deep_probe_every=1, deep_cu_sweep=True,
                                    deep_cu_sweep_extra=("mx", "wide"))
    stream = plugin.ListAndWatch(dp.Empty(), _Ctx())
    next(stream)
    with caplog.at_level("ERROR"):
        plugin.heartbeat()
    resp = next(stream)
    bad = {d.ID for d in resp.devices if d.health == "Unhealthy"}
    assert len(bad) == 4 and len(resp.devices) == 8
    assert {plugin.devices[i].dev_id for i in bad} == {phys[1]}
    assert plugin._deep_failed == {phys[1]}
    assert "cu_sweep: xcc 3 se 1 cu 7 simd 2 failed mxfp4_32 (hip device 5)" \
        in caplog.text
    assert "cu_sweep: xcc 3 se 1 cu 7 simd 0 failed bf8_16" in caplog.text
    # distinct SIMDs over all sets: simd 2 once, simd 0 once
    assert _gauge(plugin) == [2.0]

    mod.results.clear()
    plugin.heartbeat()
    resp = next(stream)
    assert all(d.health == "Healthy" for d in resp.devices)
    assert _gauge(plugin) == [0.0]
    plugin.stop()


def _run_cli(fake_node, monkeypatch, flags):
    import k8s_device_plugin_amd.plugin as plugin_pkg
    from k8s_device_plugin_amd.cli import device_plugin_main

    built = []

    class _Stop(Exception):
        pass

    class _CapturingManager:
        def __init__(self, factory, **kwargs):
            built.append(factory("gpu"))
            raise _Stop

    monkeypatch.setattr(plugin_pkg, "PluginManager", _CapturingManager)
    with pytest.raises(_Stop):
        device_plugin_main(["--sysroot", fake_node.paths.root,
                            "--deep-probe-every", "3"] + flags)
    return built[0]


@pytest.mark.parametrize("value,want", [("mx,wide", ("mx", "wide")),
                                        ("all", ("mx", "wide")),
                                        ("wide", ("wide",))])
def test_cli_flag_reaches_the_plugin(fake_mi355x_8, monkeypatch, value, want):
    plugin = _run_cli(fake_mi355x_8, monkeypatch,
                      ["--deep-probe-cu-sweep",
                       "--deep-probe-cu-sweep-extra", value])
    assert plugin.deep_cu_sweep is True
    assert tuple(plugin.deep_cu_sweep_extra) == want


def test_cli_default_is_no_extra_set(fake_mi355x_8, monkeypatch):
    plugin = _run_cli(fake_mi355x_8, monkeypatch, ["--deep-probe-cu-sweep"])
    assert tuple(plugin.deep_cu_sweep_extra) == ()


@pytest.mark.parametrize("flags", [
    ["--deep-probe-cu-sweep-extra", "mx"],  # needs --deep-probe-cu-sweep
    ["--deep-probe-cu-sweep", "--deep-probe-cu-sweep-extra", "sparse"],
])
def test_cli_flag_errors(fake_mi355x_8, capsys, flags):
    from k8s_device_plugin_amd.cli import device_plugin_main

    with pytest.raises(SystemExit) as exc:
        device_plugin_main(["--sysroot", fake_mi355x_8.paths.root] + flags)
    assert exc.value.code == 2
    assert "--deep-probe-cu-sweep-extra" in capsys.readouterr().err

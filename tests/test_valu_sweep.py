"""VALU sweep, CPU side: the tables of native/valu_table.h against an
independent reference (tests/valu_reference.py), the recorded transcendental
words against the correctly rounded values, the build inputs and argument
checks, the health policy and the plugin wiring (stubbed module), a
stand-alone sanitizer run of the generator and the mnemonics in the compiled
kernels.

The sweep itself runs on the GPU: tests/test_valu_sweep_gpu.py.
"""

import os
import re
import shutil
import struct
import subprocess

import pytest

import k8s_device_plugin_amd.native as native
from k8s_device_plugin_amd.native import build as nb
from k8s_device_plugin_amd.native import record_trans
from k8s_device_plugin_amd.plugin import AMDGPUPlugin
from k8s_device_plugin_amd.protos import deviceplugin as dp
from k8s_device_plugin_amd.testing.fakesysfs import build_mi355x_node

from deep_probe_stubs import Ctx as _Ctx
from deep_probe_stubs import cpx_plugin, gauge, stub_probe  # noqa: F401
from valu_reference import REFERENCE

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_DIR = os.path.join(REPO, "k8s_device_plugin_amd", "native")
SETS = ("fma", "int", "cvt", "xlane", "salu", "trans")
MUST_HAVE = {"v_fma_f32", "v_fma_f64", "v_mul_hi_u32", "v_cvt_f16_f32",
             "v_cvt_pk_bf16_f32", "s_mul_hi_u32"}
# the cross-lane instructions the xlane set must hold
XLANE_MNEMONICS = {"v_mov_b32_dpp", "ds_swizzle_b32", "ds_bpermute_b32",
                   "ds_permute_b32", "v_readlane_b32", "v_readfirstlane_b32",
                   "v_writelane_b32", "v_permlane16_swap_b32",
                   "v_permlane32_swap_b32"}

# Largest distance, in ulp, between the recorded word and the correctly
# rounded value, per op, as measured when valu_trans_gfx950.inc was recorded
# (profiles/valu_sweep_mi355x.md).  Asserted without margin: operands are
# fixed and the instructions deterministic.
TRANS_MAX_ULP = {
    "v_exp_f32": 1, "v_log_f32": 1, "v_rcp_f32": 1, "v_rsq_f32": 1,
    "v_sqrt_f32": 1, "v_sin_f32": 8, "v_rcp_f64": 208220308,
}


@pytest.fixture(scope="module")
def mod():
    try:  # torch's HIP runtime must load first (see __graft_entry__.build)
        import torch  # noqa: F401
    except ImportError:
        pass
    m = native.load_healthprobe(required=False)
    if m is None:
        pytest.skip("_healthprobe extension not built (no hipcc)")
    return m


@pytest.fixture(scope="module")
def refs(mod):
    return {s: mod.valu_sweep_reference(s) for s in SETS}


def vectors_of(ref, op):
    """Per test of one op: (operand tuples per lane, expected tuples per lane)."""
    lanes, n_in, regs = ref["lanes"], op["in_words"], op["regs"]
    for offset in op["offsets"]:
        words = struct.unpack_from(f"<{lanes * (n_in + regs)}I", ref["table"], offset)
        ins = [words[l * n_in:(l + 1) * n_in] for l in range(lanes)]
        at = lanes * n_in
        exp = [words[at + l * regs:at + (l + 1) * regs] for l in range(lanes)]
        yield ins, exp


# ---------------- tables ----------------


def test_sets_and_ops_that_may_not_be_dropped(refs):
    assert native.VALU_SWEEP_SETS == SETS
    names = [op["name"] for s in SETS for op in refs[s]["ops"]]
    assert len(names) == len(set(names))  # an injection by name finds one op
    assert MUST_HAVE <= set(names)
    assert XLANE_MNEMONICS <= {op["mnemonic"] for op in refs["xlane"]["ops"]}
    for s in ("fma", "int", "cvt", "xlane"):
        assert len(refs[s]["ops"]) >= 8
    for s in SETS:
        assert 1 <= len(refs[s]["ops"]) <= 32  # one bit each in the record
        assert refs[s]["tests_per_op"] >= 4
        assert set(REFERENCE) >= {op["name"] for op in refs[s]["ops"]} or s == "trans"


@pytest.mark.parametrize("op_set", [s for s in SETS if s != "trans"])
def test_expected_words_against_the_independent_reference(refs, op_set):
    ref = refs[op_set]
    for op in ref["ops"]:
        for t, (ins, exp) in enumerate(vectors_of(ref, op)):
            want = REFERENCE[op["name"]](ins)
            assert [tuple(w) for w in want] == [tuple(e) for e in exp], (op["name"], t)


@pytest.mark.parametrize("op_set", SETS)
def test_every_operand_and_result_bit_is_0_and_1_somewhere(refs, op_set):
    ref = refs[op_set]
    for op in ref["ops"]:
        n_in, regs = op["in_words"], op["regs"]
        ones, zeros = [0] * (n_in + regs), [0] * (n_in + regs)
        for ins, exp in vectors_of(ref, op):
            for words in (i + e for i, e in zip(ins, exp)):
                for k, w in enumerate(words):
                    ones[k] |= w
                    zeros[k] |= ~w & 0xFFFFFFFF
        masks = [op["vary"][which] for which, width in enumerate(op["widths"])
                 for _ in range(width)] + list(op["out_vary"][:regs])
        for k, mask in enumerate(masks):
            assert ones[k] & zeros[k] & mask == mask, (op["name"], k)


def test_vary_masks_leave_out_only_what_the_ranges_exclude(refs):
    """Whole words vary, but for the operands and results listed here."""
    narrowed = {op["name"] for s in SETS if s != "trans" for op in refs[s]["ops"]
                if any(op["vary"][w] != 0xFFFFFFFF for w in range(4) if op["widths"][w])
                or any(m != 0xFFFFFFFF for m in op["out_vary"][:op["regs"]])}
    assert narrowed == {
        "v_perm_b32", "v_bfe_u32", "v_cvt_f16_f32", "v_cvt_f32_f16",
        "v_cvt_f64_f32", "v_cvt_f32_u32", "v_cvt_f32_fp8", "v_cvt_f32_bf8",
        "v_cvt_scalef32_pk_fp4_f32", "v_readlane_b32", "v_writelane_b32",
        "s_bfe_u32", "s_bfe_i64", "s_bcnt1_i32_b64", "s_and_saveexec_b64"}


def test_xlane_values_are_pairwise_distinct(refs):
    ref = refs["xlane"]
    for op in ref["ops"]:
        data = [which for which in (0, 1, 3) if op["widths"][which]]
        if op["mnemonic"] in ("ds_bpermute_b32", "ds_permute_b32",
                              "v_readlane_b32", "v_writelane_b32"):
            data.remove(1)  # b is an index or a lane select there
        for t, (ins, _) in enumerate(vectors_of(ref, op)):
            at = {0: 0, 1: op["widths"][0], 3: op["in_words"] - 1}
            values = [ins[l][at[which]] for which in data for l in range(64)]
            assert len(set(values)) == len(values), (op["name"], t)
            if op["mnemonic"] in ("ds_bpermute_b32", "ds_permute_b32"):
                lanes = sorted(ins[l][1] // 4 % 64 for l in range(64))
                is_permutation = lanes == list(range(64))
                assert is_permutation == (
                    op["mnemonic"] == "ds_permute_b32" or t != 3), (op["name"], t)


@pytest.mark.parametrize("op_set", SETS)
def test_layout(refs, op_set):
    ref = refs[op_set]
    assert len(ref["table"]) == ref["table_bytes"] and ref["table_bytes"] % 16 == 0
    assert ref["table_bytes"] <= ref["lds_bytes"]
    # over half of a CU's 160 KiB: two sweep blocks cannot share a CU
    assert 80 * 1024 + 16 <= ref["lds_bytes"] <= 160 * 1024
    spans = []
    for op in ref["ops"]:
        size = ref["lanes"] * (op["in_words"] + op["regs"]) * 4
        assert len(op["offsets"]) == ref["tests_per_op"]
        assert sum(op["widths"]) == op["in_words"] and 1 <= op["regs"] <= 4
        spans += [(o, o + size) for o in op["offsets"]]
    spans.sort()
    assert spans[0][0] == 0 and spans[-1][1] <= ref["table_bytes"]
    for (_, end), (start, _) in zip(spans, spans[1:]):
        assert end <= start  # no overlap


def test_recorded_trans_words_are_within_the_measured_ulp(refs):
    ref = refs["trans"]
    recorded = []
    for op in ref["ops"]:
        for _, exp in vectors_of(ref, op):
            recorded += [w for lane in exp for w in lane]
    assert any(recorded), "valu_trans_gfx950.inc holds no recording"
    worst = record_trans.max_ulp_per_op(ref, recorded)
    print(worst)
    assert worst == TRANS_MAX_ULP
    # the file's own comment says the same
    with open(os.path.join(NATIVE_DIR, "valu_trans_gfx950.inc")) as f:
        stated = dict(re.findall(r"^//   (\w+): (\d+)$", f.read(), re.M))
    assert {k: int(v) for k, v in stated.items()} == TRANS_MAX_ULP


def test_trans_operands_stay_in_their_ranges(refs):
    ref = refs["trans"]
    span = {"v_exp_f32": (-20, 20), "v_sin_f32": (-1, 1)}
    for op in ref["ops"]:
        for ins, _ in vectors_of(ref, op):
            for words in ins:
                if op["name"] == "v_rcp_f64":
                    x = struct.unpack("<d", struct.pack("<II", *words))[0]
                else:
                    x = struct.unpack("<f", struct.pack("<I", *words))[0]
                lo, hi = span.get(op["name"], (-2.0 ** 20, 2.0 ** 20))
                assert lo <= x <= hi and x != 0
                if op["name"] in ("v_log_f32", "v_rsq_f32", "v_sqrt_f32"):
                    assert x > 0


# ---------------- build and arguments ----------------


def test_valu_headers_are_build_inputs():
    for name in ("valu_kernels.h", "valu_table.h", "valu_trans_gfx950.inc"):
        assert os.path.join(nb.PKG_DIR, name) in nb._HIP_HEADERS


def test_argument_errors_come_before_any_hip_call(mod):
    with pytest.raises(ValueError, match="op_set must be"):
        mod.valu_sweep(0, 0, None, "base")
    with pytest.raises(ValueError, match="op_set must be"):
        mod.valu_sweep_reference("all")
    with pytest.raises(ValueError, match="reps"):
        mod.valu_sweep(0, -1, None, "fma")
    with pytest.raises(ValueError, match="reps"):
        mod.valu_sweep(0, 65537, None, "fma")
    with pytest.raises(ValueError, match=r"inject must be \(block, wave, op\)"):
        mod.valu_sweep(0, 0, (0, 0), "fma")
    for inject in ((-1, 0, 0), (0, 4, 0), (0, 0, 10), (0, 0, -1)):
        with pytest.raises(ValueError, match="inject"):
            mod.valu_sweep(0, 0, inject, "fma")
    word = b"\0" * 256
    with pytest.raises(ValueError, match="unknown op"):
        mod.valu_raw(0, "v_nop", word)
    with pytest.raises(ValueError, match="takes b"):
        mod.valu_raw(0, "v_fma_f32", word)
    with pytest.raises(ValueError, match="takes no c"):
        mod.valu_raw(0, "v_add_f32", word, word, word)
    with pytest.raises(ValueError, match="takes no old"):
        mod.valu_raw(0, "v_fma_f32", word, word, word, word)
    with pytest.raises(ValueError, match="64 lanes x 1 words, 256 bytes"):
        mod.valu_raw(0, "v_fma_f32", word, word, word[:-4])
    with pytest.raises(ValueError, match="64 lanes x 2 words, 512 bytes"):
        mod.valu_raw(0, "v_fma_f64", word, word * 2, word * 2)
    with pytest.raises(ValueError, match="must be bytes"):
        mod.valu_raw(0, "v_ffbh_u32", 5)


# ---------------- policy (stubbed module) ----------------

BDF = "0000:05:00.0"
_BAD_SIMD = {"xcc": 3, "se": 1, "sh": 0, "cu": 7, "simd": 2,
             "ops": ["v_fma_f32", "v_pk_fma_f32"], "bad_lanes": 1 << 5,
             "first": {"op": "v_fma_f32", "t": 0, "lane": 5, "reg": 0,
                       "got": 9, "expected": 1}}
_BAD_LINE = "valu_sweep: xcc 3 se 1 cu 7 simd 2 failed v_fma_f32, v_pk_fma_f32"
_OPS = {"fma": ["v_fma_f32", "v_fma_f64", "v_pk_fma_f32"],
        "int": ["v_mul_hi_u32"], "cvt": ["v_cvt_f16_f32"],
        "xlane": ["ds_bpermute_b32"], "salu": ["s_mul_i32", "s_mul_hi_u32"],
        "trans": ["v_exp_f32"]}


def _sweep_result(bad=(), cu_count=256, cus_covered=None, simds=None):
    cus = cu_count if cus_covered is None else cus_covered
    simds = 4 * cus if simds is None else simds
    return {"cu_count": cu_count, "cus_covered": cus, "simds_covered": simds,
            "coverage_complete": simds == 4 * cu_count, "launches": 1, "reps": 8,
            "uncovered": [], "bad": list(bad), "records": [], "sweep_ms": 0.1,
            "ok": not bad}


class _ValuStub:
    """run_probe of a healthy GPU plus valu_sweep; no cu_sweep, no lds_sweep."""

    def __init__(self, results=None, bus_ids=(BDF,)):
        self.results = results or {}  # (device, set) or set -> sweep dict
        self.calls, self.sweeps = [], []
        self._bus_ids = list(bus_ids)

    def run_probe(self, device=0, hbm_bytes=1 << 30):
        self.calls.append(device)
        return {"healthy": True, "mfma_tflops": 2000.0, "hbm_gbps": 5000.0,
                "hbm_copy_ok": True, "hbm_mismatches": 0, "hbm_first_bad": -1}

    def pci_bus_ids(self):
        return self._bus_ids

    def valu_sweep_reference(self, op_set="fma"):
        if op_set not in _OPS:
            raise ValueError(op_set)
        return {"ops": [{"name": n} for n in _OPS[op_set]]}

    def valu_sweep(self, device=0, reps=0, inject=None, op_set="fma"):
        self.sweeps.append((device, op_set, inject))
        res = self.results.get((device, op_set)) or self.results.get(op_set)
        return dict(res or _sweep_result())


def test_off_by_default(stub_probe):
    mod = stub_probe(_ValuStub())
    res = native.deep_health_probe()
    assert "valu_sweep" not in res and res["healthy"] and mod.sweeps == []
    assert sorted(res) == sorted(list(_ValuStub().run_probe()) +
                                 ["floors", "floor_violations"])


@pytest.mark.parametrize("spec,want", [
    (None, ()), (False, ()), ("", ()), ("0", ()), (True, SETS), ("all", SETS),
    ("1", SETS), ("salu,fma", ("fma", "salu")), (["trans"], ("trans",)),
    (" Int , cvt ", ("int", "cvt")),
])
def test_set_parsing(stub_probe, spec, want):
    stub_probe(_ValuStub())
    assert native.valu_sweep_sets(spec) == want


@pytest.mark.parametrize("env,want", [
    ("", ()), ("0", ()), ("1", SETS), ("all", SETS), ("xlane,int", ("int", "xlane")),
])
def test_environment_parsing(stub_probe, monkeypatch, env, want):
    mod = stub_probe(_ValuStub())
    monkeypatch.setenv(native.VALU_SWEEP_ENV, env)
    res = native.deep_health_probe()
    assert [s for _, s, _ in mod.sweeps] == list(want)
    assert list(res.get("valu_sweep", {})) == list(want)
    # an explicit argument wins over the environment
    mod.sweeps.clear()
    assert "valu_sweep" not in native.deep_health_probe(valu_sweep=False)
    assert mod.sweeps == []


@pytest.mark.parametrize("spec", ["mx", "fma,base", "all,fma", ["nope"]])
def test_unknown_set_is_an_error(stub_probe, monkeypatch, spec):
    mod = stub_probe(_ValuStub())
    with pytest.raises(ValueError, match="valu_sweep"):
        native.deep_health_probe(valu_sweep=spec)
    assert mod.calls == []  # before anything ran
    if isinstance(spec, str):
        monkeypatch.setenv(native.VALU_SWEEP_ENV, spec)
        with pytest.raises(ValueError, match="valu_sweep"):
            native.deep_health_probe()


def test_cu_sweep_extra_sets_are_untouched():
    assert native.CU_SWEEP_EXTRA_SETS == ("mx", "wide")
    assert native.cu_sweep_extra_sets("all") == ("mx", "wide")


def test_bad_simd_is_named_and_unhealthy(stub_probe):
    mod = stub_probe(_ValuStub({"fma": _sweep_result(bad=[_BAD_SIMD])}))
    res = native.deep_health_probe(valu_sweep="fma,int")
    assert not res["healthy"]
    assert res["floor_violations"] == [_BAD_LINE]
    assert list(res["valu_sweep"]) == ["fma", "int"]
    assert res["valu_sweep"]["int"]["ok"] and "warnings" not in res
    assert [(d, s) for d, s, _ in mod.sweeps] == [(0, "fma"), (0, "int")]


def test_salu_wording(stub_probe):
    bad = dict(_BAD_SIMD, ops=["s_mul_hi_u32"])
    stub_probe(_ValuStub({"salu": _sweep_result(bad=[bad])}))
    res = native.deep_health_probe(valu_sweep=["salu"])
    assert not res["healthy"]
    assert res["floor_violations"] == [
        "valu_sweep: xcc 3 se 1 cu 7 scalar unit failed s_mul_hi_u32 "
        "(seen by simd 2)"]


def test_one_line_per_bad_simd_and_set(stub_probe):
    other = dict(_BAD_SIMD, simd=0, ops=["v_fma_f64"])
    stub_probe(_ValuStub({
        "fma": _sweep_result(bad=[other, _BAD_SIMD]),
        "cvt": _sweep_result(bad=[dict(_BAD_SIMD, ops=["v_cvt_f16_f32"])])}))
    res = native.deep_health_probe(valu_sweep=True)
    assert res["floor_violations"] == [
        "valu_sweep: xcc 3 se 1 cu 7 simd 0 failed v_fma_f64", _BAD_LINE,
        "valu_sweep: xcc 3 se 1 cu 7 simd 2 failed v_cvt_f16_f32"]


def test_incomplete_but_clean_only_warns(stub_probe):
    stub_probe(_ValuStub({"fma": _sweep_result(cus_covered=255, simds=1019)}))
    res = native.deep_health_probe(valu_sweep="fma,trans")
    assert res["healthy"] and res["floor_violations"] == []
    assert res["warnings"] == ["valu_sweep_incomplete[fma]: 255 of 256 CUs, 1019 SIMDs"]
    # bad and incomplete: the violation, no warning
    stub_probe(_ValuStub({"fma": _sweep_result(bad=[_BAD_SIMD], cus_covered=255)}))
    res = native.deep_health_probe(valu_sweep="fma")
    assert not res["healthy"] and "warnings" not in res


def test_inject_by_name_reaches_the_set_that_owns_the_op(stub_probe, monkeypatch):
    mod = stub_probe(_ValuStub())
    monkeypatch.setenv(native.VALU_SWEEP_INJECT_ENV, "3:1:s_mul_hi_u32")
    native.deep_health_probe(valu_sweep="all")
    assert mod.sweeps == [(0, s, (3, 1, 1) if s == "salu" else None) for s in SETS]
    mod.sweeps.clear()
    monkeypatch.setenv(native.VALU_SWEEP_INJECT_ENV, "0:0:v_pk_fma_f32")
    native.deep_health_probe(valu_sweep="fma")
    assert mod.sweeps == [(0, "fma", (0, 0, 2))]


@pytest.mark.parametrize("spec", ["1:2", "a:0:v_fma_f32", "0:0:v_nop", "0:0:1",
                                  "0:0:v_fma_f32:9"])
def test_inject_errors(stub_probe, monkeypatch, spec):
    stub_probe(_ValuStub())
    monkeypatch.setenv(native.VALU_SWEEP_INJECT_ENV, spec)
    with pytest.raises(ValueError, match="AMDXDP_VALU_SWEEP_INJECT=.*block:wave:op"):
        native.deep_health_probe(valu_sweep="fma")
    # the variable alone turns nothing on
    assert "valu_sweep" not in native.deep_health_probe()


# ---------------- plugin, metrics, CLI ----------------


def _cpx_plugin(tmp_path, stub_probe, bad=None, **kwargs):
    results = {}
    if bad is not None:
        results[bad] = _sweep_result(bad=[_BAD_SIMD], cu_count=32)
    return cpx_plugin(tmp_path, stub_probe,
                      lambda bus_ids: _ValuStub(results, bus_ids=bus_ids), **kwargs)


def _gauge(plugin, name="amdgpu_dp_deep_probe_bad_valu_simds"):
    return gauge(plugin, name)


def test_plugin_sweeps_every_ordinal_of_the_gpu(tmp_path, stub_probe):
    plugin, mod, _ = _cpx_plugin(tmp_path, stub_probe, deep_probe_every=1,
                                 deep_valu_sweep=("fma", "salu"))
    plugin.heartbeat()
    assert mod.calls == [0, 4]  # the full probe once per physical GPU
    assert [(d, s) for d, s, _ in mod.sweeps] == [
        (d, s) for d in range(8) for s in ("fma", "salu")]
    assert not plugin._deep_failed
    assert plugin._sweep_bad_simds == {} and plugin._sweep_bad_lds_cus == {}
    plugin.stop()


def test_plugin_without_the_flag_does_not_sweep(tmp_path, stub_probe):
    plugin, mod, _ = _cpx_plugin(tmp_path, stub_probe, deep_probe_every=1)
    plugin.heartbeat()
    assert mod.calls == [0, 4] and mod.sweeps == []
    assert plugin._sweep_bad_valu_simds == {}
    assert _gauge(plugin) == [({"resource": "gpu"}, 0.0)]
    plugin.stop()


def test_plugin_bad_simd_pins_that_gpu_only_and_recovers(tmp_path, stub_probe, caplog):
    plugin, mod, phys = _cpx_plugin(tmp_path, stub_probe, bad=(6, "fma"),
                                    deep_probe_every=1, deep_valu_sweep=("fma", "cvt"))
    stream = plugin.ListAndWatch(dp.Empty(), _Ctx())
    next(stream)
    with caplog.at_level("ERROR"):
        plugin.heartbeat()
    resp = next(stream)
    bad = {d.ID for d in resp.devices if d.health == "Unhealthy"}
    assert len(bad) == 4 and len(resp.devices) == 8
    assert {plugin.devices[i].dev_id for i in bad} == {phys[1]}
    assert plugin._deep_failed == {phys[1]}
    assert _BAD_LINE + " (hip device 6)" in caplog.text
    assert plugin._sweep_bad_valu_simds == {phys[0]: 0, phys[1]: 1}
    assert _gauge(plugin) == [({"resource": "gpu"}, 1.0)]
    assert _gauge(plugin, "amdgpu_dp_deep_probe_bad_simds") == [({"resource": "gpu"}, 0.0)]

    # recovery: the next sweep is clean -> unpinned, gauge back to 0
    mod.results.clear()
    plugin.heartbeat()
    resp = next(stream)
    assert all(d.health == "Healthy" for d in resp.devices)
    assert _gauge(plugin) == [({"resource": "gpu"}, 0.0)]
    plugin.stop()


def test_plugin_result_and_the_probe_itself_not_sweeping(tmp_path, stub_probe,
                                                         monkeypatch):
    plugin, mod, phys = _cpx_plugin(tmp_path, stub_probe, bad=(1, "salu"),
                                    deep_probe_every=1, deep_valu_sweep=("salu",))
    # the flag rules: the environment does not add a second sweep in the probe
    monkeypatch.setenv(native.VALU_SWEEP_ENV, "all")
    res = plugin._deep_probe(next(d for d in plugin.devices.values()
                                  if d.dev_id == phys[0]))
    assert [(d, s) for d, s, _ in mod.sweeps] == [(d, "salu") for d in range(4)]
    assert sorted(res["valu_sweep"]["salu"]) == [0, 1, 2, 3]
    assert not res["healthy"]
    assert res["floor_violations"] == [
        "valu_sweep: xcc 3 se 1 cu 7 scalar unit failed v_fma_f32, v_pk_fma_f32 "
        "(seen by simd 2) (hip device 1)"]
    plugin.stop()


def test_prestart_deep_aborts_on_a_bad_simd(tmp_path, stub_probe):
    import grpc

    fs = build_mi355x_node(str(tmp_path / "n"), n_gpus=1)
    mod = stub_probe(_ValuStub({"fma": _sweep_result(bad=[_BAD_SIMD])}))
    plugin = AMDGPUPlugin(resource="gpu", paths=fs.paths, prestart_probe=True,
                          prestart_deep=True, deep_valu_sweep=("fma",),
                          dev_root=fs.paths.root + "/dev")
    plugin.start()
    dev = next(iter(plugin.devices.values()))
    dri = os.path.join(fs.paths.root, "dev", "dri")
    os.makedirs(dri, exist_ok=True)
    open(os.path.join(dri, f"renderD{dev.render_d}"), "w").close()

    class _AbortCtx:
        code = None

        def abort(self, code, msg):
            self.code = code
            raise RuntimeError(f"aborted: {msg}")

    ctx = _AbortCtx()
    req = dp.PreStartContainerRequest(devices_ids=[dev.id])
    with pytest.raises(RuntimeError, match="valu_sweep: xcc 3 se 1 cu 7 simd 2"):
        plugin.PreStartContainer(req, ctx)
    assert ctx.code == grpc.StatusCode.FAILED_PRECONDITION
    assert mod.calls == [0] and [(d, s) for d, s, _ in mod.sweeps] == [(0, "fma")]
    plugin.stop()


def _plugin_built_by_cli(fake, monkeypatch, flags):
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
        device_plugin_main(["--sysroot", fake.paths.root,
                            "--deep-probe-every", "3"] + flags)
    return built[0]


@pytest.mark.parametrize("flags,want", [
    ([], ()),
    (["--deep-probe-valu-sweep"], SETS),
    (["--deep-probe-valu-sweep", "all"], SETS),
    (["--deep-probe-valu-sweep", "salu,fma"], ("fma", "salu")),
    (["--deep-probe-valu-sweep=trans"], ("trans",)),
    (["--deep-probe-valu-sweep", "--deep-probe-lds-sweep"], SETS),
])
def test_cli_flag_reaches_the_plugin(fake_mi355x_8, monkeypatch, flags, want):
    plugin = _plugin_built_by_cli(fake_mi355x_8, monkeypatch, flags)
    assert plugin.deep_valu_sweep == want
    assert plugin.deep_cu_sweep is False and plugin.deep_cu_sweep_extra == ()
    assert plugin.deep_lds_sweep is ("--deep-probe-lds-sweep" in flags)
    assert plugin.deep_probe_every == 3


def test_cli_rejects_an_unknown_set(fake_mi355x_8, capsys):
    from k8s_device_plugin_amd.cli import device_plugin_main

    with pytest.raises(SystemExit) as e:
        device_plugin_main(["--sysroot", fake_mi355x_8.paths.root,
                            "--deep-probe-valu-sweep", "fma,mx"])
    assert e.value.code == 2
    assert "--deep-probe-valu-sweep: valu_sweep: unknown op set 'mx'" in capsys.readouterr().err


# ---------------- the generator under the sanitizers ----------------


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_valu_table_under_sanitizers(tmp_path):
    """A stand-alone program (its own main) generates every table and checks
    the expected words again, under ASan + UBSan."""
    exe = str(tmp_path / "valu_table_check")
    # the runtimes are linked statically: the dynamic ASan runtime refuses
    # to start wherever the environment preloads any other library
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-static-libasan",
         "-static-libubsan", f"-I{NATIVE_DIR}",
         os.path.join(REPO, "tests", "native", "valu_table_check.cpp"),
         "-o", exe],
        check=True, capture_output=True, text=True,
    )
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ok" in run.stdout


# ---------------- the instructions in the compiled kernels ----------------


@pytest.mark.skipif(not os.path.exists(nb.HIPCC), reason="no hipcc")
def test_every_descriptor_mnemonic_is_in_the_compiled_kernels(refs, tmp_path):
    """A compiler upgrade that lowers an op to another instruction is seen."""
    out = str(tmp_path / "valu_kernels.s")
    subprocess.run(
        [nb.HIPCC, f"--offload-arch={nb.GFX_ARCH}", "--cuda-device-only", "-S",
         "-O3", "-std=c++17", f"-I{NATIVE_DIR}",
         os.path.join(REPO, "tests", "native", "valu_kernels_tu.hip"), "-o", out],
        check=True, capture_output=True, text=True,
    )
    with open(out) as f:
        code = [line.split(";")[0].split() for line in f]
    seen = {fields[0].rsplit("_e32", 1)[0].rsplit("_e64", 1)[0]
            for fields in code if fields}
    # an op whose name is two instructions names both
    wanted = {m for s in SETS for op in refs[s]["ops"]
              for m in [op["mnemonic"]] + op["name"].split(".")[0].split("+")}
    assert wanted - seen == set()

"""Every opt-in sweep of the deep probe at once, with exact values: the order
and wording of violations, warnings, extension calls, log records and gauges,
for native.deep_health_probe and for AMDGPUPlugin._deep_probe (stubbed
module, CPU only).  The per-sweep files test each sweep on its own.
"""

import logging

import pytest

import k8s_device_plugin_amd.native as native

from deep_probe_stubs import cpx_plugin, gauge, stub_probe  # noqa: F401

BDF = "0000:05:00.0"
PROBE = {"wave_ok": True, "mfma_ok": True, "lds_ok": True, "hbm_copy_ok": True,
         "hbm_mismatches": 0, "hbm_first_bad": -1, "mfma_tflops": 2000.0,
         "hbm_gbps": 6200.0, "healthy": True}


def _simd(names, simd=2, key="pipes"):
    return {"xcc": 3, "se": 1, "sh": 0, "cu": 7, "simd": simd, key: list(names)}


_BAD_CU = {"xcc": 3, "se": 1, "sh": 0, "cu": 7, "mismatches": 2,
           "first": {"path": "b128", "pattern": "checker", "step": 1,
                     "element": 5120, "word": 2, "got": 0x55555155,
                     "expected": 0x55555555}}
_LDS_LINE = ("lds_sweep: xcc 3 se 1 cu 7: 2 bad accesses (path b128 pattern "
             "checker step 1, element 5120, bits 0x00000400 in word 2)")


def _sweep(bad=(), cu_count=256, cus_covered=None, simds=None):
    cus = cu_count if cus_covered is None else cus_covered
    simds = 4 * cus if simds is None else simds
    return {"cu_count": cu_count, "cus_covered": cus, "simds_covered": simds,
            "coverage_complete": cus == cu_count and simds == 4 * cu_count,
            "bad": list(bad), "sweep_ms": 0.1, "ok": not bad}


class _AllStub:
    """Every entry the policy calls, each call logged with its keywords.
    results: (entry, device, set or None) -> sweep dict."""

    def __init__(self, results=None, bus_ids=(BDF,), during_lds=None):
        self.results = results or {}
        self.bus_ids = list(bus_ids)
        self.during_lds = during_lds
        self.log = []

    def _call(self, entry, kwargs, which=None):
        self.log.append((entry, kwargs))
        res = self.results.get((entry, kwargs["device"], which))
        return dict(res or _sweep(cu_count=32))

    def run_probe(self, **kwargs):
        self.log.append(("run_probe", kwargs))
        return dict(PROBE)

    def pci_bus_ids(self):
        self.log.append(("pci_bus_ids", {}))
        return self.bus_ids

    def cu_sweep(self, **kwargs):
        return self._call("cu_sweep", kwargs, kwargs.get("pipe_set", "base"))

    def lds_sweep(self, **kwargs):
        if self.during_lds:
            self.during_lds()
        return self._call("lds_sweep", kwargs)

    def valu_sweep(self, **kwargs):
        return self._call("valu_sweep", kwargs, kwargs["op_set"])


def _write_gfx_ecc(sysroot, ue, ce):
    d = sysroot / "sys" / "bus" / "pci" / "devices" / BDF / "ras"
    d.mkdir(parents=True, exist_ok=True)
    (d / "gfx_err_count").write_text(f"ue: {ue}\nce: {ce}\n")


def test_deep_health_probe_with_every_sweep(stub_probe, tmp_path):
    _write_gfx_ecc(tmp_path, 0, 3)
    mod = stub_probe(_AllStub({
        ("cu_sweep", 0, "base"): _sweep([_simd(["fp8_16"])]),
        ("cu_sweep", 0, "mx"): _sweep(cus_covered=250),
        ("cu_sweep", 0, "wide"): _sweep([_simd(["f64_16"]),
                                         _simd(["bf8_16"], simd=0)]),
        ("lds_sweep", 0, None): _sweep([_BAD_CU]),
        ("valu_sweep", 0, "fma"): _sweep(
            [_simd(["v_fma_f32", "v_pk_fma_f32"], key="ops")]),
        ("valu_sweep", 0, "salu"): _sweep([_simd(["s_mul_hi_u32"], key="ops")]),
        ("valu_sweep", 0, "trans"): _sweep(cus_covered=255, simds=1019),
    }, during_lds=lambda: _write_gfx_ecc(tmp_path, 0, 4)))
    res = native.deep_health_probe(cu_sweep=True, cu_sweep_extra="all",
                                   lds_sweep=True, valu_sweep=True,
                                   sysroot=str(tmp_path))
    assert res["floor_violations"] == [
        "cu_sweep: xcc 3 se 1 cu 7 simd 2 failed fp8_16",
        "cu_sweep: xcc 3 se 1 cu 7 simd 2 failed f64_16",
        "cu_sweep: xcc 3 se 1 cu 7 simd 0 failed bf8_16",
        _LDS_LINE,
        "valu_sweep: xcc 3 se 1 cu 7 simd 2 failed v_fma_f32, v_pk_fma_f32",
        "valu_sweep: xcc 3 se 1 cu 7 scalar unit failed s_mul_hi_u32 "
        "(seen by simd 2)",
    ]
    assert res["warnings"] == [
        "cu_sweep_incomplete[mx]: 250 of 256 CUs, 1000 SIMDs",
        "lds_sweep_ecc: 1 corrected gfx ECC errors during the sweep",
        "valu_sweep_incomplete[trans]: 255 of 256 CUs, 1019 SIMDs",
    ]
    assert res["healthy"] is False
    assert set(res) == set(PROBE) | {
        "floors", "floor_violations", "warnings", "cu_sweep", "cu_sweep_extra",
        "lds_sweep", "valu_sweep"}
    assert "cu_count" in res["cu_sweep"] and "cu_count" in res["lds_sweep"]
    assert list(res["cu_sweep_extra"]) == ["mx", "wide"]
    assert list(res["valu_sweep"]) == list(native.VALU_SWEEP_SETS)
    for sets in (res["cu_sweep_extra"], res["valu_sweep"]):
        assert all(isinstance(s, dict) and "cu_count" in s for s in sets.values())
    assert res["lds_sweep"]["ecc"] == {"before": {"ue": 0, "ce": 3},
                                       "after": {"ue": 0, "ce": 4}}
    assert res["lds_sweep"]["violations"] == [_LDS_LINE]
    assert res["lds_sweep"]["warnings"] == [res["warnings"][1]]
    # base goes without a pipe_set keyword: a module from before the extra
    # sets has no such parameter
    assert mod.log == [
        ("run_probe", {"device": 0, "hbm_bytes": 1 << 30}),
        ("cu_sweep", {"device": 0, "inject": None}),
        ("cu_sweep", {"device": 0, "inject": None, "pipe_set": "mx"}),
        ("cu_sweep", {"device": 0, "inject": None, "pipe_set": "wide"}),
        ("pci_bus_ids", {}),
        ("lds_sweep", {"device": 0, "corrupt": None}),
    ] + [("valu_sweep", {"device": 0, "inject": None, "op_set": s})
         for s in native.VALU_SWEEP_SETS]


_PLUGIN_LOGGER = "k8s_device_plugin_amd.plugin.server"


def _plugin_records(caplog):
    return [(r.levelname, r.getMessage()) for r in caplog.records
            if r.name == _PLUGIN_LOGGER]


def test_plugin_deep_probe_with_every_sweep(tmp_path, stub_probe, caplog):
    results = {
        ("cu_sweep", 5, "base"): _sweep([_simd(["fp8_16"])], 32),
        ("cu_sweep", 5, "wide"): _sweep([_simd(["f64_16"]),
                                         _simd(["bf8_16"], simd=0)], 32),
        ("cu_sweep", 6, "mx"): _sweep(cu_count=32, cus_covered=30),
        ("lds_sweep", 4, None): _sweep(cu_count=32, cus_covered=30),
        ("lds_sweep", 6, None): _sweep([_BAD_CU], 32),
        ("lds_sweep", 7, None): _sweep([_BAD_CU], 32),
        ("valu_sweep", 4, "fma"): _sweep(
            [_simd(["v_fma_f32", "v_pk_fma_f32"], key="ops")], 32),
        ("valu_sweep", 4, "salu"): _sweep(
            [_simd(["s_mul_hi_u32"], key="ops")], 32),
        ("valu_sweep", 7, "fma"): _sweep(cu_count=32, cus_covered=31, simds=123),
    }
    plugin, mod, phys = cpx_plugin(
        tmp_path, stub_probe, lambda bus_ids: _AllStub(results, bus_ids),
        deep_probe_every=1, deep_cu_sweep=True,
        deep_cu_sweep_extra=("mx", "wide"), deep_lds_sweep=True,
        deep_valu_sweep=("fma", "salu"))
    with caplog.at_level(logging.INFO, logger=_PLUGIN_LOGGER):
        plugin.heartbeat()
    violations = [
        "cu_sweep: xcc 3 se 1 cu 7 simd 2 failed fp8_16 (hip device 5)",
        "cu_sweep: xcc 3 se 1 cu 7 simd 2 failed f64_16 (hip device 5)",
        "cu_sweep: xcc 3 se 1 cu 7 simd 0 failed bf8_16 (hip device 5)",
        _LDS_LINE + " (hip device 6)",
        _LDS_LINE + " (hip device 7)",
        "valu_sweep: xcc 3 se 1 cu 7 simd 2 failed v_fma_f32, v_pk_fma_f32 "
        "(hip device 4)",
        "valu_sweep: xcc 3 se 1 cu 7 scalar unit failed s_mul_hi_u32 "
        "(seen by simd 2) (hip device 4)",
    ]
    on = f"deep probe on {phys[1]}: "
    assert _plugin_records(caplog) == [
        ("ERROR", on + violations[0]),
        ("ERROR", on + violations[1]),
        ("ERROR", on + violations[2]),
        ("WARNING", on + "cu_sweep (mx pipes) reached 30 of 32 CUs on hip device 6"),
        ("WARNING", on + "lds_sweep_incomplete: 30 of 32 CUs (hip device 4)"),
        ("ERROR", on + violations[3]),
        ("ERROR", on + violations[4]),
        ("ERROR", on + violations[5]),
        ("ERROR", on + violations[6]),
        ("WARNING", on + "valu_sweep_incomplete[fma]: 31 of 32 CUs, 123 SIMDs "
                         "(hip device 7)"),
        ("ERROR", f"deep probe UNHEALTHY on {phys[1]}: violations={violations}"),
    ]
    assert plugin._deep_failed == {phys[1]}
    # a SIMD bad in two sets counts once; the LDS count is a plain sum
    assert plugin._sweep_bad_simds == {phys[0]: 0, phys[1]: 2}
    assert plugin._sweep_bad_lds_cus == {phys[0]: 0, phys[1]: 2}
    assert plugin._sweep_bad_valu_simds == {phys[0]: 0, phys[1]: 1}
    label = {"resource": "gpu"}
    assert gauge(plugin, "amdgpu_dp_deep_probe_failed_gpus") == [(label, 1.0)]
    assert gauge(plugin, "amdgpu_dp_deep_probe_bad_simds") == [(label, 2.0)]
    assert gauge(plugin, "amdgpu_dp_deep_probe_bad_lds_cus") == [(label, 2.0)]
    assert gauge(plugin, "amdgpu_dp_deep_probe_bad_valu_simds") == [(label, 1.0)]

    # per GPU: the probe itself on the first ordinal with the flagged sweeps
    # off, then sweep by sweep, each over every ordinal (and set)
    def calls(first):
        ordinals = range(first, first + 4)
        return (
            [("pci_bus_ids", {}),
             ("run_probe", {"device": first, "hbm_bytes": 1 << 30})]
            + [("cu_sweep", dict({"device": d, "inject": None},
                                 **({} if s == "base" else {"pipe_set": s})))
               for d in ordinals for s in ("base", "mx", "wide")]
            + [c for d in ordinals
               for c in (("pci_bus_ids", {}),
                         ("lds_sweep", {"device": d, "corrupt": None}))]
            + [("valu_sweep", {"device": d, "inject": None, "op_set": s})
               for d in ordinals for s in ("fma", "salu")])
    assert mod.log == calls(0) + calls(4)

    mod.log.clear()
    res = plugin._deep_probe(next(d for d in plugin.devices.values()
                                  if d.dev_id == phys[1]))
    assert res["healthy"] is False and res["floor_violations"] == violations
    assert set(res) == set(PROBE) | {
        "floors", "floor_violations", "cu_sweep", "cu_sweep_extra",
        "lds_sweep", "valu_sweep"}
    ordinals = [4, 5, 6, 7]
    assert list(res["cu_sweep"]) == list(res["lds_sweep"]) == ordinals
    assert list(res["cu_sweep_extra"]) == ["mx", "wide"]
    assert list(res["valu_sweep"]) == ["fma", "salu"]
    for sets in (res["cu_sweep_extra"], res["valu_sweep"]):
        assert all(list(per_ordinal) == ordinals for per_ordinal in sets.values())
    assert res["cu_sweep"][5]["bad"] and res["cu_sweep_extra"]["wide"][5]["bad"]
    assert res["lds_sweep"][6]["violations"] == [_LDS_LINE]
    assert res["valu_sweep"]["salu"][4]["bad"]
    assert mod.log == calls(4)
    plugin.stop()


def test_plugin_leaves_a_sweep_without_its_flag_to_the_environment(
        tmp_path, stub_probe, monkeypatch):
    plugin, mod, phys = cpx_plugin(
        tmp_path, stub_probe, lambda bus_ids: _AllStub(
            {("lds_sweep", 4, None): _sweep([_BAD_CU], 32)}, bus_ids),
        deep_probe_every=1, deep_cu_sweep=True, deep_lds_sweep=False)
    monkeypatch.setenv(native.LDS_SWEEP_ENV, "1")
    plugin.heartbeat()
    # the probe runs the sweep itself, on the first ordinal of each GPU only
    assert [k["device"] for e, k in mod.log if e == "lds_sweep"] == [0, 4]
    assert [k["device"] for e, k in mod.log if e == "cu_sweep"] == list(range(8))
    assert plugin._sweep_bad_lds_cus == {}
    assert plugin._sweep_bad_simds == {phys[0]: 0, phys[1]: 0}
    assert plugin._deep_failed == {phys[1]}
    assert gauge(plugin, "amdgpu_dp_deep_probe_bad_lds_cus") == [
        ({"resource": "gpu"}, 0.0)]
    res = plugin._deep_probe(next(d for d in plugin.devices.values()
                                  if d.dev_id == phys[1]))
    assert res["floor_violations"] == [_LDS_LINE]  # no hip device suffix
    assert "cu_count" in res["lds_sweep"] and list(res["cu_sweep"]) == [4, 5, 6, 7]
    plugin.stop()

"""LDS sweep, CPU side: the schedule of native/lds_march.h (under the
sanitizers and against numpy), the argument checks, the health policy and
the plugin wiring (stubbed module).

The sweep itself runs on the GPU: tests/test_lds_sweep_gpu.py.
"""

import os
import shutil
import subprocess

import numpy as np
import pytest

import k8s_device_plugin_amd.native as native
from k8s_device_plugin_amd.native import build as nb
from k8s_device_plugin_amd.plugin import AMDGPUPlugin
from k8s_device_plugin_amd.protos import deviceplugin as dp
from k8s_device_plugin_amd.testing.fakesysfs import build_mi355x_node

from deep_probe_stubs import Ctx as _Ctx
from deep_probe_stubs import ProbeOnlyStub as _ProbeOnlyStub
from deep_probe_stubs import cpx_plugin, gauge, stub_probe  # noqa: F401

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_DIR = os.path.join(REPO, "k8s_device_plugin_amd", "native")

PATHS = ["b128", "b64", "b32", "dma", "tr16"]
ACCESS_BYTES = {"b128": 16, "b64": 8, "b32": 4, "dma": 16, "tr16": 8}
SIZES = [16, 2048, 2064, 65536, 67584, 163840]


def covered(path, lds_bytes):
    unit = {"dma": 1024, "tr16": 2048}.get(path, 1)
    return lds_bytes // unit * unit


# ---------------- the header ----------------


def test_lds_march_is_a_build_input():
    assert os.path.join(nb.PKG_DIR, "lds_march.h") in nb._HIP_HEADERS


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_lds_march_under_sanitizers(tmp_path):
    """A stand-alone program (its own main) runs the schedule on a model of
    one CU's LDS with injected faults, under ASan + UBSan."""
    exe = str(tmp_path / "lds_march_check")
    # the runtimes are linked statically: the dynamic ASan runtime refuses
    # to start wherever the environment preloads any other library
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-static-libasan",
         "-static-libubsan", f"-I{NATIVE_DIR}",
         os.path.join(REPO, "tests", "native", "lds_march_check.cpp"),
         "-o", exe],
        check=True, capture_output=True, text=True,
    )
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ok" in run.stdout


# ---------------- the reference entry (needs the built extension) ----------------


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


@pytest.mark.parametrize("lds_bytes", SIZES[:5])
def test_reference_paths_and_rotation(probe_mod, lds_bytes):
    ref = probe_mod.lds_sweep_reference(lds_bytes)
    assert [p["name"] for p in ref["paths"]] == PATHS
    assert ref["default_reps"] >= 1 and ref["threads"] == 256
    want_patterns = {"b128": ["address", "solid", "checker", "random"],
                     "b64": ["address"], "b32": ["address"],
                     "dma": ["random"], "tr16": ["address"]}
    want_after = {"b128": [0, 1, 2], "b64": [0, 1, 2], "b32": [0, 1, 2],
                  "dma": [1], "tr16": [0]}
    for p in ref["paths"]:
        name = p["name"]
        assert p["bytes"] == covered(name, lds_bytes), name
        assert p["access_bytes"] == ACCESS_BYTES[name]
        assert p["accesses"] == p["bytes"] // ACCESS_BYTES[name]
        assert p["default_patterns"] == want_patterns[name]
        assert p["corruptible_after"] == want_after[name]
        # In step s access a belongs to thread ((a % 256) + 64 s) % 256;
        # work item j is access j, in the march's descending step 2 access
        # n - 1 - j.
        n = p["accesses"]
        j = np.arange(n)
        got = np.array(p["thread_of_item"]).reshape(p["steps"], n)
        for s in range(p["steps"]):
            a = n - 1 - j if name in ("b128", "b64", "b32") and s == 2 else j
            assert np.array_equal(got[s], (a % 256 + 64 * s) % 256), (name, s)
        # so a cell's reader in step s + 1 sits one wave after its writer
        if name in ("b128", "b64", "b32") and n:
            thread_of_access = np.empty_like(got)
            for s in range(4):
                a = n - 1 - j if s == 2 else j
                thread_of_access[s, a] = got[s]
            waves = thread_of_access // 64
            for s in range(3):
                assert np.all((waves[s + 1] - waves[s]) % 4 == 1), (name, s)


def test_reference_tr16_is_the_transposition_of_4x16_tiles(probe_mod):
    src = np.array(probe_mod.lds_sweep_reference(2048)["tr16_source"])
    assert src.shape == (256, 4)
    # one round: 16 tiles of 128 bytes, each 4 rows x 16 columns of 16-bit
    # values; offsets[tile, row, column]
    offsets = np.arange(0, 2048, 2).reshape(16, 4, 16)
    # lanes 16g .. 16g+15 take tile g column-wise: lane i column i, its
    # element q from row q
    want = offsets.transpose(0, 2, 1).reshape(256, 4)
    assert np.array_equal(src, want)
    assert sorted(src.ravel()) == list(range(0, 2048, 2))  # each value once


@pytest.mark.parametrize("lds_bytes", [0, 8, 24, -16, (1 << 22) + 16])
def test_reference_rejects_bad_sizes(probe_mod, lds_bytes):
    with pytest.raises(ValueError):
        probe_mod.lds_sweep_reference(lds_bytes)


_FLIP = (0, "b128", "address", 0, "flip", 0, 0, 0)


@pytest.mark.parametrize("kwargs", [
    {"lds_bytes": 8},
    {"lds_bytes": 24},
    {"lds_bytes": -16},
    {"lds_bytes": (1 << 30) + 16},
    {"blocks": -1},
    {"blocks": 65537},
    {"reps": -1},
    {"reps": 65537},
    {"paths": ["b256"]},
    {"paths": ["b128", "b128"]},
    {"paths": []},
    {"paths": 3},
    {"patterns": ["stripes"]},
    {"patterns": ["solid", "solid"]},
    {"patterns": []},
    {"corrupt": 3},
    {"corrupt": ()},
    {"corrupt": _FLIP[:7]},                                   # flip needs 8
    {"corrupt": (0, "b128", "address", 0, "alias", 0, 1, 2)},  # alias needs 7
    {"corrupt": (0, "b128", "address", 0, "smudge", 0, 0, 0)},
    {"corrupt": (-1,) + _FLIP[1:]},
    {"blocks": 2, "corrupt": (2,) + _FLIP[1:]},
    {"corrupt": (0, "b256") + _FLIP[2:]},
    {"corrupt": (0, "b128", "stripes") + _FLIP[3:]},
    {"paths": ["b64"], "corrupt": _FLIP},                      # path not run
    {"corrupt": (0, "b64", "solid", 0, "flip", 0, 0, 0)},      # pattern not run
    {"patterns": ["solid"], "corrupt": _FLIP},
    {"corrupt": (0, "dma", "address", 1, "flip", 0, 0, 0)},    # dma is random
    {"corrupt": (0, "b128", "address", 3, "flip", 0, 0, 0)},   # nothing reads after
    {"corrupt": (0, "b128", "address", -1, "flip", 0, 0, 0)},
    {"corrupt": (0, "dma", "random", 0, "flip", 0, 0, 0)},     # the fill overwrites
    {"corrupt": (0, "dma", "random", 2, "flip", 0, 0, 0)},
    {"corrupt": (0, "tr16", "address", 1, "flip", 0, 0, 0)},
    {"corrupt": (0, "b128", "address", 0, "flip", 0, 4, 0)},
    {"corrupt": (0, "b128", "address", 0, "flip", 0, 0, 32)},
    {"corrupt": (0, "b128", "address", 0, "flip", -1, 0, 0)},
    {"lds_bytes": 2064, "corrupt": (0, "b128", "address", 0, "flip", 129, 0, 0)},
    # elements 128 of 2064 bytes is outside what dma and tr16 cover
    {"lds_bytes": 2064, "corrupt": (0, "dma", "random", 1, "flip", 128, 0, 0)},
    {"lds_bytes": 2064, "corrupt": (0, "tr16", "address", 0, "flip", 128, 0, 0)},
    {"lds_bytes": 2064, "corrupt": (0, "b128", "address", 0, "alias", 0, 0)},
    {"lds_bytes": 2064, "corrupt": (0, "b128", "address", 0, "alias", 0, 129)},
    {"lds_bytes": 2064, "corrupt": (0, "b128", "address", 0, "alias", 0, -1)},
    {"lds_bytes": 2064, "corrupt": (0, "tr16", "address", 0, "alias", 0, 128)},
])
def test_lds_sweep_rejects_bad_arguments(probe_mod, kwargs):
    """Rejected before any HIP call, so it holds without a GPU."""
    with pytest.raises(ValueError):
        probe_mod.lds_sweep(device=0, **kwargs)


# ---------------- policy (stubbed probe module) ----------------


def _lds_result(bad=(), cu_count=256, cus_covered=None):
    cus = cu_count if cus_covered is None else cus_covered
    return {
        "cu_count": cu_count,
        "cus_covered": cus,
        "coverage_complete": cus == cu_count,
        "placement_consistent": True,
        "uncovered": cu_count - cus,
        "launches": 1,
        "reps": 2,
        "blocks": cu_count,
        "lds_bytes": 163840,
        "lds_bytes_per_cu": 163840,
        "paths": {p: 163840 for p in PATHS},
        "patterns": {},
        "seed": 0x5EED,
        "mismatches": sum(b["mismatches"] for b in bad),
        "bad": list(bad),
        "records": [],
        "sweep_ms": 0.8,
        "ok": not bad,
    }


_BAD_CU = {
    "xcc": 3, "se": 1, "sh": 0, "cu": 7, "mismatches": 2,
    "bad_bits": (0, 0, 0x400, 0),
    "first": {"path": "b128", "pattern": "checker", "step": 1,
              "element": 5120, "word": 2, "got": 0x55555155,
              "expected": 0x55555555},
}
_BAD_LINE = ("lds_sweep: xcc 3 se 1 cu 7: 2 bad accesses (path b128 pattern "
             "checker step 1, element 5120, bits 0x00000400 in word 2)")

BDF = "0000:05:00.0"


class _CuSweepStub(_ProbeOnlyStub):
    """The module as it was at the parent commit: no lds_sweep."""

    def __init__(self, cu_result=None, bus_ids=()):
        super().__init__()
        self.cu_result = cu_result
        self.bus_ids = list(bus_ids)
        self.cu_sweeps = []

    def cu_sweep(self, device=0, reps=0, inject=None):
        self.cu_sweeps.append(device)
        return self.cu_result or {
            "cu_count": 256, "cus_covered": 256, "simds_covered": 1024,
            "coverage_complete": True, "bad": [], "ok": True}

    def pci_bus_ids(self):
        return self.bus_ids


class _LdsStub(_CuSweepStub):
    def __init__(self, results=None, bus_ids=(BDF,), cu_result=None,
                 during=None):
        super().__init__(cu_result, bus_ids)
        self.results = results or {}  # ordinal -> sweep dict
        self.sweeps = []  # (device, corrupt)
        self.during = during  # called while the sweep "runs"

    def lds_sweep(self, device=0, lds_bytes=0, blocks=0, reps=0, paths=None,
                  patterns=None, seed=0x5EED, corrupt=None):
        self.sweeps.append((device, corrupt))
        if self.during:
            self.during()
        return dict(self.results.get(device) or _lds_result())


def test_off_is_key_for_key_as_before(stub_probe):
    mod = stub_probe(_ProbeOnlyStub())  # has no lds_sweep attribute at all
    res = native.deep_health_probe()
    assert sorted(res) == sorted(
        list(_ProbeOnlyStub().run_probe()) + ["floors", "floor_violations"])
    assert res["healthy"] and res["floor_violations"] == []
    assert mod.calls == [0]

    # a module of the parent commit, with the CU sweep on, is fine too
    mod = stub_probe(_CuSweepStub())
    res = native.deep_health_probe(cu_sweep=True, lds_sweep=False)
    assert "lds_sweep" not in res and "warnings" not in res
    assert mod.cu_sweeps == [0]

    mod = stub_probe(_LdsStub())
    res = native.deep_health_probe(lds_sweep=False)
    assert mod.sweeps == [] and "lds_sweep" not in res


def test_on_and_clean(stub_probe, tmp_path):
    mod = stub_probe(_LdsStub(bus_ids=["x"] * 4))
    res = native.deep_health_probe(device=3, lds_sweep=True,
                                   sysroot=str(tmp_path))
    assert mod.sweeps == [(3, None)]
    assert res["healthy"] and res["floor_violations"] == []
    assert res["lds_sweep"]["ok"] and "warnings" not in res
    assert res["lds_sweep"]["violations"] == []
    assert res["lds_sweep"]["ecc"] is None  # no counter file here


def test_bad_cu_is_unhealthy_and_named(stub_probe, tmp_path):
    stub_probe(_LdsStub({0: _lds_result(bad=[_BAD_CU])}))
    res = native.deep_health_probe(lds_sweep=True, sysroot=str(tmp_path))
    assert not res["healthy"]
    assert res["floor_violations"] == [_BAD_LINE]
    assert native.lds_sweep_violations(res["lds_sweep"]) == [_BAD_LINE]
    assert res["lds_sweep"]["bad"][0]["first"]["element"] == 5120


def test_incomplete_but_clean_only_warns(stub_probe, tmp_path):
    stub_probe(_LdsStub({0: _lds_result(cus_covered=250)}))
    res = native.deep_health_probe(lds_sweep=True, sysroot=str(tmp_path))
    assert res["healthy"] and res["floor_violations"] == []
    assert res["warnings"] == ["lds_sweep_incomplete: 250 of 256 CUs"]


def test_incomplete_warning_coexists_with_the_cu_sweeps(stub_probe, tmp_path):
    cu = {"cu_count": 256, "cus_covered": 255, "simds_covered": 1020,
          "coverage_complete": False, "bad": [], "ok": True}
    stub_probe(_LdsStub({0: _lds_result(cus_covered=250)}, cu_result=cu))
    res = native.deep_health_probe(cu_sweep=True, lds_sweep=True,
                                   sysroot=str(tmp_path))
    assert res["healthy"]
    assert res["warnings"] == [
        "cu_sweep_incomplete: 255 of 256 CUs, 1020 SIMDs",
        "lds_sweep_incomplete: 250 of 256 CUs",
    ]


def test_env_toggle_and_argument_precedence(stub_probe, monkeypatch, tmp_path):
    mod = stub_probe(_LdsStub())
    for value, on in (("0", False), ("", False), (" 0 ", False), ("1", True)):
        monkeypatch.setenv(native.LDS_SWEEP_ENV, value)
        assert native.lds_sweep_enabled() is on, value
        mod.sweeps.clear()
        res = native.deep_health_probe(sysroot=str(tmp_path))
        assert ("lds_sweep" in res) == on, value
        assert bool(mod.sweeps) == on, value
    # an explicit argument wins over the environment, both ways
    mod.sweeps.clear()
    assert "lds_sweep" not in native.deep_health_probe(lds_sweep=False)
    assert mod.sweeps == []
    monkeypatch.setenv(native.LDS_SWEEP_ENV, "0")
    assert "lds_sweep" in native.deep_health_probe(lds_sweep=True,
                                                   sysroot=str(tmp_path))
    # and the CU sweep's switch is another one
    monkeypatch.setenv(native.CU_SWEEP_ENV, "1")
    res = native.deep_health_probe(sysroot=str(tmp_path))
    assert "cu_sweep" in res and "lds_sweep" not in res


def test_inject_env_is_parsed_and_passed(stub_probe, monkeypatch, tmp_path):
    mod = stub_probe(_LdsStub())
    monkeypatch.setenv(native.LDS_SWEEP_INJECT_ENV, "1:7:2:10")
    native.deep_health_probe(lds_sweep=True, sysroot=str(tmp_path))
    assert mod.sweeps == [(0, (1, "b128", "address", 0, "flip", 7, 2, 10))]
    for bad in ("1:2:3", "1:2:3:4:5", "a:b:c:d", "1,2,3,4"):
        monkeypatch.setenv(native.LDS_SWEEP_INJECT_ENV, bad)
        with pytest.raises(ValueError, match="block:element:word:bit"):
            native.deep_health_probe(lds_sweep=True, sysroot=str(tmp_path))


# ---------------- the gfx RAS counters ----------------


def _write_ecc(sysroot, ue, ce, block="gfx"):
    d = sysroot / "sys" / "bus" / "pci" / "devices" / BDF / "ras"
    d.mkdir(parents=True, exist_ok=True)
    (d / f"{block}_err_count").write_text(f"ue: {ue}\nce: {ce}\n")


def test_gfx_err_count_unchanged_is_reported_and_clean(stub_probe, tmp_path):
    _write_ecc(tmp_path, 0, 3)
    _write_ecc(tmp_path, 9, 9, block="umc")  # not the file the sweep reads
    stub_probe(_LdsStub())
    res = native.deep_health_probe(lds_sweep=True, sysroot=str(tmp_path))
    assert res["healthy"] and "warnings" not in res
    assert res["lds_sweep"]["ecc"] == {"before": {"ue": 0, "ce": 3},
                                       "after": {"ue": 0, "ce": 3}}


def test_gfx_ce_rise_warns_and_ue_rise_is_a_violation(stub_probe, tmp_path):
    _write_ecc(tmp_path, 0, 3)
    stub_probe(_LdsStub(during=lambda: _write_ecc(tmp_path, 0, 5)))
    res = native.deep_health_probe(lds_sweep=True, sysroot=str(tmp_path))
    assert res["healthy"] and res["floor_violations"] == []
    assert res["warnings"] == [
        "lds_sweep_ecc: 2 corrected gfx ECC errors during the sweep"]

    _write_ecc(tmp_path, 0, 3)
    stub_probe(_LdsStub(during=lambda: _write_ecc(tmp_path, 1, 3)))
    res = native.deep_health_probe(lds_sweep=True, sysroot=str(tmp_path))
    assert not res["healthy"]
    assert res["floor_violations"] == [
        "lds_sweep: 1 uncorrectable gfx ECC errors during the sweep"]


def test_unreadable_gfx_err_count_is_none(stub_probe, tmp_path):
    path = tmp_path / "sys/bus/pci/devices" / BDF / "ras" / "gfx_err_count"
    path.parent.mkdir(parents=True)
    path.write_text("ue: many\n")
    stub_probe(_LdsStub())
    res = native.deep_health_probe(lds_sweep=True, sysroot=str(tmp_path))
    assert res["lds_sweep"]["ecc"] is None and res["healthy"]
    # a module that cannot name the device's bus id: the same
    stub_probe(_LdsStub(bus_ids=[]))
    res = native.deep_health_probe(lds_sweep=True, sysroot=str(tmp_path))
    assert res["lds_sweep"]["ecc"] is None and res["healthy"]


def test_read_ecc_counts_default_is_umc(tmp_path):
    _write_ecc(tmp_path, 1, 2, block="umc")
    _write_ecc(tmp_path, 3, 4, block="gfx")
    assert native.read_ecc_counts(BDF, str(tmp_path)) == {"ue": 1, "ce": 2}
    assert native.read_ecc_counts(BDF, str(tmp_path), "umc") == {"ue": 1, "ce": 2}
    assert native.read_ecc_counts(BDF, str(tmp_path), block="gfx") == {
        "ue": 3, "ce": 4}
    assert native.read_ecc_counts(BDF, str(tmp_path), "sdma") is None


# ---------------- plugin, metrics, CLI ----------------


def _cpx_plugin(tmp_path, stub_probe, bad_ordinal=None, **kwargs):
    results = {}
    if bad_ordinal is not None:
        results[bad_ordinal] = _lds_result(bad=[_BAD_CU], cu_count=32)
    return cpx_plugin(tmp_path, stub_probe,
                      lambda bus_ids: _LdsStub(results, bus_ids=bus_ids), **kwargs)


def test_plugin_sweeps_every_ordinal_of_the_gpu(tmp_path, stub_probe):
    plugin, mod, phys = _cpx_plugin(tmp_path, stub_probe, deep_probe_every=1,
                                    deep_lds_sweep=True)
    plugin.heartbeat()
    # the full probe once per physical GPU, on its first ordinal ...
    assert mod.calls == [0, 4]
    # ... and the LDS sweep on every partition of each; no CU sweep
    assert [d for d, _ in mod.sweeps] == [0, 1, 2, 3, 4, 5, 6, 7]
    assert mod.cu_sweeps == []
    assert not plugin._deep_failed
    assert plugin._sweep_bad_simds == {}
    plugin.stop()


def test_plugin_without_the_flag_does_not_sweep(tmp_path, stub_probe):
    plugin, mod, _ = _cpx_plugin(tmp_path, stub_probe, deep_probe_every=1)
    plugin.heartbeat()
    assert mod.calls == [0, 4] and mod.sweeps == [] and mod.cu_sweeps == []
    assert plugin._sweep_bad_lds_cus == {}
    assert [v for _, v in
            gauge(plugin, "amdgpu_dp_deep_probe_bad_lds_cus")] == [0.0]
    plugin.stop()


def test_plugin_bad_cu_pins_that_gpu_only_and_recovers(tmp_path, stub_probe,
                                                       caplog):
    plugin, mod, phys = _cpx_plugin(tmp_path, stub_probe, bad_ordinal=6,
                                    deep_probe_every=1, deep_lds_sweep=True)
    stream = plugin.ListAndWatch(dp.Empty(), _Ctx())
    next(stream)
    with caplog.at_level("ERROR"):
        plugin.heartbeat()
    resp = next(stream)
    health = {d.ID: d.health for d in resp.devices}
    bad = {i for i, h in health.items() if h == "Unhealthy"}
    assert len(bad) == 4 and len(health) == 8
    assert {plugin.devices[i].dev_id for i in bad} == {phys[1]}
    assert plugin._deep_failed == {phys[1]}
    assert _BAD_LINE + " (hip device 6)" in caplog.text

    # the gauge reports the bad CUs of the last sweep, per resource
    assert gauge(plugin, "amdgpu_dp_deep_probe_bad_lds_cus") == [
        ({"resource": "gpu"}, 1.0)]
    assert [v for _, v in
            gauge(plugin, "amdgpu_dp_deep_probe_bad_simds")] == [0.0]

    # recovery: the next sweep is clean -> unpinned, gauge back to 0
    mod.results.clear()
    plugin.heartbeat()
    resp = next(stream)
    assert all(d.health == "Healthy" for d in resp.devices)
    assert sum(plugin._sweep_bad_lds_cus.values()) == 0
    plugin.stop()


def test_both_sweep_flags_work_together(tmp_path, stub_probe):
    plugin, mod, phys = _cpx_plugin(tmp_path, stub_probe, bad_ordinal=1,
                                    deep_probe_every=1, deep_cu_sweep=True,
                                    deep_lds_sweep=True)
    plugin.heartbeat()
    assert mod.calls == [0, 4]
    assert mod.cu_sweeps == [0, 1, 2, 3, 4, 5, 6, 7]
    assert [d for d, _ in mod.sweeps] == [0, 1, 2, 3, 4, 5, 6, 7]
    assert plugin._deep_failed == {phys[0]}
    assert plugin._sweep_bad_simds == {phys[0]: 0, phys[1]: 0}
    assert plugin._sweep_bad_lds_cus == {phys[0]: 1, phys[1]: 0}
    res = plugin._deep_probe(next(d for d in plugin.devices.values()
                                  if d.dev_id == phys[0]))
    assert sorted(res["cu_sweep"]) == sorted(res["lds_sweep"]) == [0, 1, 2, 3]
    assert res["floor_violations"] == [_BAD_LINE + " (hip device 1)"]
    plugin.stop()


def test_prestart_deep_aborts_on_a_bad_cu(tmp_path, stub_probe):
    import grpc

    fs = build_mi355x_node(str(tmp_path / "n"), n_gpus=1)
    mod = stub_probe(_LdsStub({0: _lds_result(bad=[_BAD_CU])}))
    plugin = AMDGPUPlugin(resource="gpu", paths=fs.paths, prestart_probe=True,
                          prestart_deep=True, deep_lds_sweep=True,
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
    with pytest.raises(RuntimeError, match="lds_sweep: xcc 3 se 1 cu 7: 2 bad"):
        plugin.PreStartContainer(req, ctx)
    assert ctx.code == grpc.StatusCode.FAILED_PRECONDITION
    assert mod.calls == [0] and [d for d, _ in mod.sweeps] == [0]
    plugin.stop()


@pytest.mark.parametrize("flags,cu,lds", [
    ([], False, False),
    (["--deep-probe-lds-sweep"], False, True),
    (["--deep-probe-cu-sweep", "--deep-probe-lds-sweep"], True, True),
])
def test_cli_flag_reaches_the_plugin(fake_mi355x_8, monkeypatch, flags, cu, lds):
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
        device_plugin_main(["--sysroot", fake_mi355x_8.paths.root,
                            "--deep-probe-every", "3"] + flags)
    assert built[0].deep_lds_sweep is lds
    assert built[0].deep_cu_sweep is cu
    assert built[0].deep_probe_every == 3

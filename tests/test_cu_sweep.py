"""CU sweep, CPU side: the known-answer tables, the host table code under
the sanitizers, the health policy and the plugin wiring (stubbed module).

The sweep itself runs on the GPU: tests/test_cu_sweep_gpu.py.
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

PIPES = {  # name -> (M, N, K)
    "bf16_16": (16, 16, 32),
    "bf16_32": (32, 32, 16),
    "f16_16": (16, 16, 32),
    "fp8_16": (16, 16, 32),
    "i8_16": (16, 16, 64),
    "mxfp8_16": (16, 16, 128),
}


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
def reference(probe_mod):
    return probe_mod.cu_sweep_reference()


def _result_row(m, lane, reg):
    """C/D lane map, the same for every dtype."""
    if m == 16:
        return 4 * (lane >> 4) + reg
    return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)


def test_reference_lists_every_pipe(reference):
    got = {p["name"]: (p["M"], p["N"], p["K"]) for p in reference["pipes"]}
    assert got == PIPES
    assert reference["tests_per_pipe"] >= 1
    for p in reference["pipes"]:
        assert len(p["tests"]) == reference["tests_per_pipe"]
    # one block per CU: more than half of the CU's 160 KiB of LDS
    assert 80 * 1024 < reference["table_bytes"] <= 160 * 1024


def test_reference_expected_fragments_are_the_product(reference):
    for p in reference["pipes"]:
        m, n, k = p["M"], p["N"], p["K"]
        regs = m * n // 64
        assert p["regs"] == regs
        for t, test in enumerate(p["tests"]):
            where = f"{p['name']} t={t}"
            a = np.array(test["A"], dtype=np.int64)
            b = np.array(test["B"], dtype=np.int64)
            assert a.shape == (m, k) and b.shape == (k, n), where
            assert np.abs(a).max() <= 2 and np.abs(b).max() <= 2, where
            d = a @ b
            assert np.abs(d).max() < 512, where

            # a swapped, duplicated or shifted lane cannot give this tile
            assert len({tuple(r) for r in d}) == m, where
            assert len({tuple(c) for c in d.T}) == n, where
            assert not np.array_equal(d, d.T), where

            want = np.empty((64, regs), dtype=np.int64)
            for lane in range(64):
                for reg in range(regs):
                    want[lane, reg] = d[_result_row(m, lane, reg), lane % n]
            got = np.array(test["expected"])
            assert got.shape == (64, regs), where
            assert np.array_equal(got, want), where

            # and the bits the kernel compares are those values' encodings
            bits = np.array(test["expected_bits"], dtype=np.uint32)
            if p["int_result"]:
                enc = want.astype(np.int32).view(np.uint32)
            else:
                enc = want.astype(np.float32).view(np.uint32)
            assert np.array_equal(bits, enc), where


_FP8_E4M3 = {0xC0: -2, 0xB8: -1, 0x00: 0, 0x38: 1, 0x40: 2}


def _decode_frag(name, raw):
    """[64][J] integer values of a packed per-lane fragment."""
    buf = np.frombuffer(raw, dtype=np.uint8).reshape(64, -1)
    if name.startswith("bf16"):
        u = buf.view(np.uint16).astype(np.uint32) << 16
        return u.view(np.float32).astype(np.int64)
    if name.startswith("f16"):
        return buf.view(np.float16).astype(np.int64)
    if name.startswith("i8"):
        return buf.view(np.int8).astype(np.int64)
    return np.vectorize(_FP8_E4M3.__getitem__)(buf).astype(np.int64)


def test_reference_packed_fragments_follow_the_slot_map(reference):
    """Lane l holds row/col l % M and slots (l // M) * J + j."""
    for p in reference["pipes"]:
        m, n, k = p["M"], p["N"], p["K"]
        j_per_lane = k // (64 // m)
        for t, test in enumerate(p["tests"]):
            a = np.array(test["A"], dtype=np.int64)
            b = np.array(test["B"], dtype=np.int64)
            fa = _decode_frag(p["name"], test["a_frag"])
            fb = _decode_frag(p["name"], test["b_frag"])
            assert fa.shape == fb.shape == (64, j_per_lane), p["name"]
            for lane in range(64):
                s0 = (lane // m) * j_per_lane
                assert np.array_equal(fa[lane], a[lane % m, s0:s0 + j_per_lane])
                assert np.array_equal(fb[lane], b[s0:s0 + j_per_lane, lane % n])


def test_decode_hw_id(probe_mod):
    # SIMD_ID 5:4, CU_ID 11:8, SH_ID 12, SE_ID 14:13; other fields ignored
    hw = 0b11 << 30 | 0xA << 16 | 2 << 13 | 1 << 12 | 9 << 8 | 1 << 6 | 3 << 4 | 7
    assert probe_mod.decode_hw_id(hw, 5) == (5, 2, 1, 9, 3)
    assert probe_mod.decode_hw_id(0, 0) == (0, 0, 0, 0, 0)
    # bit 15 is not part of SE_ID on gfx942 / gfx950
    assert probe_mod.decode_hw_id(1 << 15, 0) == (0, 0, 0, 0, 0)


@pytest.mark.parametrize("kwargs", [
    {"reps": -1},
    {"inject": (0, 4, 0)},
    {"inject": (0, 0, 6)},
    {"inject": (-1, 0, 0)},
    {"inject": (0, 0)},
])
def test_cu_sweep_rejects_bad_arguments(probe_mod, kwargs):
    """Rejected before any HIP call, so it holds without a GPU."""
    with pytest.raises(ValueError):
        probe_mod.cu_sweep(device=0, **kwargs)


def test_sweep_table_is_a_build_input():
    assert os.path.join(nb.PKG_DIR, "sweep_table.h") in nb._HIP_HEADERS


# ---------------- host table code under the sanitizers ----------------


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_sweep_table_under_sanitizers(tmp_path):
    """A stand-alone program (its own main) builds every table and derives
    each expected fragment a second way, under ASan + UBSan."""
    exe = str(tmp_path / "sweep_table_check")
    # the runtimes are linked statically: the dynamic ASan runtime refuses
    # to start wherever the environment preloads any other library
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-static-libasan",
         "-static-libubsan", f"-I{NATIVE_DIR}",
         os.path.join(REPO, "tests", "native", "sweep_table_check.cpp"),
         "-o", exe],
        check=True, capture_output=True, text=True,
    )
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ok" in run.stdout


# ---------------- policy (stubbed probe module) ----------------


def _sweep_result(bad=(), cu_count=256, cus_covered=None, simds_covered=None):
    cus = cu_count if cus_covered is None else cus_covered
    simds = 4 * cus if simds_covered is None else simds_covered
    return {
        "cu_count": cu_count,
        "cus_covered": cus,
        "simds_covered": simds,
        "coverage_complete": cus == cu_count and simds == 4 * cu_count,
        "launches": 1,
        "reps": 8,
        "waves_checked": 4 * cu_count,
        "pipes": list(PIPES),
        "bad": list(bad),
        "uncovered": [],
        "records": [],
        "sweep_ms": 0.1,
        "ok": not bad,
    }


_BAD_SIMD = {
    "xcc": 3, "se": 1, "sh": 0, "cu": 7, "simd": 2, "pipes": ["fp8_16"],
    "bad_lanes": 1 << 5,
    "first": {"pipe": "fp8_16", "t": 0, "lane": 5, "reg": 1,
              "got": 0x41000008, "expected": 0x41000000},
}


class _SweepStub(_ProbeOnlyStub):
    def __init__(self, results=None, bus_ids=()):
        super().__init__()
        self.results = results or {}  # ordinal -> sweep dict
        self.bus_ids = list(bus_ids)
        self.sweeps = []  # (device, inject)

    def cu_sweep(self, device=0, reps=0, inject=None):
        self.sweeps.append((device, inject))
        return self.results.get(device) or _sweep_result()

    def pci_bus_ids(self):
        return self.bus_ids


def test_sweep_off_never_touches_cu_sweep(stub_probe):
    mod = stub_probe(_ProbeOnlyStub())  # has no cu_sweep attribute at all
    res = native.deep_health_probe()
    assert res["healthy"] and res["floor_violations"] == []
    assert "cu_sweep" not in res and "warnings" not in res
    assert mod.calls == [0]

    mod = stub_probe(_SweepStub())
    res = native.deep_health_probe(cu_sweep=False)
    assert mod.sweeps == [] and "cu_sweep" not in res


def test_sweep_on_clean(stub_probe):
    mod = stub_probe(_SweepStub())
    res = native.deep_health_probe(device=3, cu_sweep=True)
    assert mod.sweeps == [(3, None)]
    assert res["healthy"] and res["floor_violations"] == []
    assert res["cu_sweep"]["ok"] and "warnings" not in res


def test_sweep_bad_simd_is_unhealthy_and_named(stub_probe):
    stub_probe(_SweepStub({0: _sweep_result(bad=[_BAD_SIMD])}))
    res = native.deep_health_probe(cu_sweep=True)
    assert not res["healthy"]
    assert res["floor_violations"] == [
        "cu_sweep: xcc 3 se 1 cu 7 simd 2 failed fp8_16"
    ]
    assert res["cu_sweep"]["bad"][0]["first"]["lane"] == 5


def test_sweep_incomplete_but_clean_only_warns(stub_probe):
    stub_probe(_SweepStub({0: _sweep_result(cus_covered=250)}))
    res = native.deep_health_probe(cu_sweep=True)
    assert res["healthy"] and res["floor_violations"] == []
    assert len(res["warnings"]) == 1
    assert res["warnings"][0].startswith("cu_sweep_incomplete: 250 of 256 CUs")


def test_sweep_env_toggle(stub_probe, monkeypatch):
    mod = stub_probe(_SweepStub())
    for value, on in (("0", False), ("", False), ("1", True)):
        monkeypatch.setenv(native.CU_SWEEP_ENV, value)
        mod.sweeps.clear()
        res = native.deep_health_probe()
        assert ("cu_sweep" in res) == on, value
        assert bool(mod.sweeps) == on, value
    # an explicit argument wins over the environment
    mod.sweeps.clear()
    assert "cu_sweep" not in native.deep_health_probe(cu_sweep=False)
    assert mod.sweeps == []


def test_sweep_inject_env_is_parsed_and_passed(stub_probe, monkeypatch):
    mod = stub_probe(_SweepStub())
    monkeypatch.setenv(native.CU_SWEEP_INJECT_ENV, "255:3:5")
    native.deep_health_probe(cu_sweep=True)
    assert mod.sweeps == [(0, (255, 3, 5))]
    monkeypatch.setenv(native.CU_SWEEP_INJECT_ENV, "1:2")
    with pytest.raises(ValueError, match="block:wave:pipe"):
        native.deep_health_probe(cu_sweep=True)


# ---------------- plugin, metrics, CLI ----------------


def _cpx_plugin(tmp_path, stub_probe, bad_ordinal=None, **kwargs):
    results = {}
    if bad_ordinal is not None:
        results[bad_ordinal] = _sweep_result(bad=[_BAD_SIMD], cu_count=32)
    return cpx_plugin(tmp_path, stub_probe,
                      lambda bus_ids: _SweepStub(results, bus_ids), **kwargs)


def test_plugin_sweeps_every_ordinal_of_the_gpu(tmp_path, stub_probe):
    plugin, mod, phys = _cpx_plugin(tmp_path, stub_probe, deep_probe_every=1,
                                    deep_cu_sweep=True)
    plugin.heartbeat()
    # the full probe once per physical GPU, on its first ordinal ...
    assert mod.calls == [0, 4]
    # ... and the sweep on every partition of each
    assert [d for d, _ in mod.sweeps] == [0, 1, 2, 3, 4, 5, 6, 7]
    assert not plugin._deep_failed
    plugin.stop()


def test_plugin_without_the_flag_does_not_sweep(tmp_path, stub_probe):
    plugin, mod, _ = _cpx_plugin(tmp_path, stub_probe, deep_probe_every=1)
    plugin.heartbeat()
    assert mod.calls == [0, 4] and mod.sweeps == []
    assert plugin._sweep_bad_simds == {}
    plugin.stop()


def test_plugin_bad_simd_pins_that_gpu_only(tmp_path, stub_probe, caplog):
    plugin, mod, phys = _cpx_plugin(tmp_path, stub_probe, bad_ordinal=2,
                                    deep_probe_every=1, deep_cu_sweep=True)
    stream = plugin.ListAndWatch(dp.Empty(), _Ctx())
    next(stream)
    with caplog.at_level("ERROR"):
        plugin.heartbeat()
    resp = next(stream)
    health = {d.ID: d.health for d in resp.devices}
    bad = {i for i, h in health.items() if h == "Unhealthy"}
    assert len(bad) == 4 and len(health) == 8
    assert {plugin.devices[i].dev_id for i in bad} == {phys[0]}
    assert plugin._deep_failed == {phys[0]}
    assert "cu_sweep: xcc 3 se 1 cu 7 simd 2 failed fp8_16" in caplog.text

    # the gauge reports the bad SIMDs of the last sweep, per resource
    assert gauge(plugin, "amdgpu_dp_deep_probe_bad_simds") == [
        ({"resource": "gpu"}, 1.0)]

    # recovery: the next sweep is clean -> unpinned, gauge back to 0
    mod.results.clear()
    plugin.heartbeat()
    resp = next(stream)
    assert all(d.health == "Healthy" for d in resp.devices)
    assert sum(plugin._sweep_bad_simds.values()) == 0
    plugin.stop()


def test_prestart_deep_aborts_on_a_bad_simd(tmp_path, stub_probe):
    import grpc

    fs = build_mi355x_node(str(tmp_path / "n"), n_gpus=1)
    mod = stub_probe(_SweepStub({0: _sweep_result(bad=[_BAD_SIMD])}))
    plugin = AMDGPUPlugin(resource="gpu", paths=fs.paths, prestart_probe=True,
                          prestart_deep=True, deep_cu_sweep=True,
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
    with pytest.raises(RuntimeError, match="cu_sweep: xcc 3 se 1 cu 7 simd 2"):
        plugin.PreStartContainer(req, ctx)
    assert ctx.code == grpc.StatusCode.FAILED_PRECONDITION
    assert mod.calls == [0] and [d for d, _ in mod.sweeps] == [0]
    plugin.stop()


def test_gauge_is_zero_while_the_sweep_is_off(tmp_path, stub_probe):
    plugin, _, _ = _cpx_plugin(tmp_path, stub_probe, deep_probe_every=1)
    plugin.heartbeat()
    assert [v for _, v in
            gauge(plugin, "amdgpu_dp_deep_probe_bad_simds")] == [0.0]
    plugin.stop()


@pytest.mark.parametrize("flag,want", [([], False),
                                       (["--deep-probe-cu-sweep"], True)])
def test_cli_flag_reaches_the_plugin(fake_mi355x_8, monkeypatch, flag, want):
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
                            "--deep-probe-every", "3"] + flag)
    assert built[0].deep_cu_sweep is want
    assert built[0].deep_probe_every == 3

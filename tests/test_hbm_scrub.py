"""The HBM scrub, CPU side: the march header under the host sanitizers behind
a faulty-memory model, hbm_march_reference against a numpy statement of each
pattern, the argument checks of hbm_scrub (they reject before any HIP call),
and the health policy, the ECC counters, the env switch and the console
script against a stub module.

The kernels themselves run on the GPU: tests/test_hbm_scrub_gpu.py.
"""

import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import k8s_device_plugin_amd.native as native
from k8s_device_plugin_amd import cli
from k8s_device_plugin_amd.native import build as nb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_DIR = os.path.join(REPO, "k8s_device_plugin_amd", "native")

PATTERNS = ["address", "solid", "checker", "random"]


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


def test_hbm_march_is_a_build_input():
    assert os.path.join(nb.PKG_DIR, "hbm_march.h") in nb._HIP_HEADERS


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_hbm_march_under_sanitizers(tmp_path):
    """A stand-alone program (its own main) runs the header's march over a
    faulty-memory model under ASan + UBSan: clean memory gives 0, a stuck or
    slow bit is found by every pattern, an address alias by address and
    random, and by solid and checker only while the march is sequential."""
    exe = str(tmp_path / "hbm_march_check")
    # static runtimes, as for hbm_pattern_check (tests/test_probe_kernels.py)
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-static-libasan",
         "-static-libubsan", f"-I{NATIVE_DIR}",
         os.path.join(REPO, "tests", "native", "hbm_march_check.cpp"),
         "-o", exe],
        check=True, capture_output=True, text=True,
    )
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ok" in run.stdout


# ---------------- the patterns, stated here in numpy ----------------

GAMMA = np.uint64(0x9E3779B97F4A7C15)


def _mix64(z):
    """splitmix64's output function on a uint64 array (wrapping)."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def numpy_pattern(pattern, seed, start, count):
    """[count][4] uint32: the pattern before any inversion."""
    i = np.uint64(start) + np.arange(count, dtype=np.uint64)
    lo32 = np.uint64(0xFFFFFFFF)
    if pattern == "address":
        lo = i & lo32
        words = [lo, i >> np.uint64(32), ~lo & lo32, _mix64(i + GAMMA) >> np.uint64(32)]
    elif pattern == "solid":
        words = [np.zeros(count, dtype=np.uint64)] * 4
    elif pattern == "checker":
        words = [np.full(count, 0x55555555, dtype=np.uint64)] * 4
    else:
        s = np.uint64(seed) + (np.uint64(2) * i + np.uint64(1)) * GAMMA
        a, b = _mix64(s), _mix64(s + GAMMA)
        words = [a & lo32, a >> np.uint64(32), b & lo32, b >> np.uint64(32)]
    return np.stack(words, axis=1).astype(np.uint32)


def numpy_expected(pattern, seed, step, start, count):
    """What step `step` must read: p, and ~p in the descending step 2."""
    p = numpy_pattern(pattern, seed, start, count)
    return ~p if step == 2 else p


def test_splitmix64_known_answer():
    # the first three outputs of the reference splitmix64 seeded with 0
    s = GAMMA * np.arange(1, 4, dtype=np.uint64)
    assert [int(x) for x in _mix64(s)] == [
        0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("step", [0, 1, 2, 3])
@pytest.mark.parametrize("start", [0, (1 << 32) - 3, (1 << 32) + 12345,
                                   (1 << 40) + 7])
def test_reference_is_the_numpy_pattern(probe_mod, pattern, step, start):
    count, seed = 1031, 0xC0FFEE1234
    raw = probe_mod.hbm_march_reference(pattern, seed, step, start, count)
    got = np.frombuffer(raw, dtype=np.uint32).reshape(count, 4)
    want = numpy_expected(pattern, seed, step, start, count)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:4]


def test_reference_address_is_injective_across_2_32(probe_mod):
    raw = probe_mod.hbm_march_reference("address", 0, 1, (1 << 32) - 1, 3)
    got = np.frombuffer(raw, dtype=np.uint32).reshape(3, 4)
    assert [tuple(r[:3]) for r in got] == [
        (0xFFFFFFFF, 0, 0), (0, 1, 0xFFFFFFFF), (1, 1, 0xFFFFFFFE)]
    assert len({bytes(r) for r in got}) == 3


def test_reference_random_depends_on_the_seed(probe_mod):
    a = probe_mod.hbm_march_reference("random", 1, 1, 0, 64)
    b = probe_mod.hbm_march_reference("random", 2, 1, 0, 64)
    assert a != b
    assert probe_mod.hbm_march_reference("solid", 1, 2, 0, 2) == b"\xff" * 32


@pytest.mark.parametrize("args", [
    ("stripes", 0, 1, 0, 1), ("address", 0, 4, 0, 1), ("address", 0, -1, 0, 1),
    ("address", 0, 1, 0, -1), ("address", 0, 1, 0, (1 << 24) + 1),
])
def test_reference_rejects_bad_arguments(probe_mod, args):
    with pytest.raises(ValueError):
        probe_mod.hbm_march_reference(*args)


# ---------------- argument checks: before any HIP call ----------------

_B = 16 * 4096


@pytest.mark.parametrize("kwargs", [
    {"bytes": 0},
    {"bytes": -16},
    {"bytes": 8},
    {"bytes": 24},
    {"bytes": _B, "slab_bytes": 0},
    {"bytes": _B, "slab_bytes": 8},
    {"bytes": _B, "slab_bytes": 40},
    {"bytes": _B, "slab_bytes": (64 << 30) + 16},
    {"bytes": 16 * 65537, "slab_bytes": 16},      # more than 65536 slabs
    {"bytes": _B, "guard": -1},
    {"bytes": _B, "guard": (1 << 20) + 1},
    {"bytes": _B, "patterns": []},
    {"bytes": _B, "patterns": ["stripes"]},
    {"bytes": _B, "patterns": ["solid", "solid"]},
    {"bytes": _B, "patterns": ["address", "solid", "address"]},
    {"bytes": _B, "max_records": 0},
    {"bytes": _B, "max_records": 4097},
    {"bytes": 16 * ((1 << 21) + 1), "return_data": True},
    {"bytes": _B, "corrupt": ()},
    {"bytes": _B, "corrupt": ("solid", 0, "flip", 0, 0)},
    {"bytes": _B, "corrupt": ("solid", 0, "flip", 0, 0, 0, 0)},
    {"bytes": _B, "corrupt": ("solid", 0, "swap", 0, 0)},
    {"bytes": _B, "corrupt": ("stripes", 0, "flip", 0, 0, 0)},
    {"bytes": _B, "corrupt": ("solid", 0, "flip", 0, 0, 0),
     "patterns": ["checker"]},                    # that pattern is not run
    {"bytes": _B, "corrupt": ("solid", -1, "flip", 0, 0, 0)},
    {"bytes": _B, "corrupt": ("solid", 3, "flip", 0, 0, 0)},
    {"bytes": _B, "corrupt": ("solid", 0, "flip", 4096, 0, 0)},
    {"bytes": _B, "corrupt": ("solid", 0, "flip", -1, 0, 0)},
    {"bytes": _B, "corrupt": ("solid", 0, "flip", 0, 4, 0)},
    {"bytes": _B, "corrupt": ("solid", 0, "flip", 0, -1, 0)},
    {"bytes": _B, "corrupt": ("solid", 0, "flip", 0, 0, 32)},
    {"bytes": _B, "corrupt": ("solid", 0, "flip", 0, 0, -1)},
    {"bytes": _B, "corrupt": ("solid", 0, "alias", 0, 0)},
    {"bytes": _B, "corrupt": ("solid", 0, "alias", 4095, 1)},
    {"bytes": _B, "corrupt": ("solid", 0, "alias", 0, -1)},
    {"bytes": _B, "corrupt": ("solid", 0, "alias", 4096, -1)},
    {"bytes": _B, "corrupt": ("solid", 3, "alias", 0, 1)},
    {"bytes": _B, "corrupt": ("solid", 0, "alias", 0, 1, 2)},
    {"bytes": _B, "corrupt": (0, 0, "flip", 0, 0, 0)},
])
def test_hbm_scrub_rejects_bad_arguments(probe_mod, kwargs):
    with pytest.raises(ValueError):
        probe_mod.hbm_scrub(device=0, **kwargs)


# ---------------- policy (stubbed probe module) ----------------

BDF = "0000:05:00.0"
VRAM = 288 << 30


def _clean_result(bytes_tested, **over):
    res = {"bytes_requested": bytes_tested, "bytes_tested": bytes_tested,
           "slabs": 1, "vram_bytes": VRAM, "vram_free_before": VRAM - (1 << 30),
           "mismatches": 0, "first_bad": -1, "bad_bits": (0, 0, 0, 0),
           "records": [], "bad_ranges": [], "guard_ok": True,
           "beyond_cache": bytes_tested >= 512 << 20, "scrub_ms": 12.5,
           "steps": {}, "ok": True}
    res.update(over)
    return res


class _ScrubStub:
    """The extension as hbm_scrub (the policy) and the console script see it."""

    def __init__(self, over=None, free=VRAM - (1 << 30), tested=None,
                 during=None, devices=1):
        self.over = over or {}
        self.free = free
        self.tested = tested      # None: all that was asked for
        self.during = during      # called while the scrub "runs"
        self.devices = devices
        self.calls = []

    def device_count(self):
        return self.devices

    def pci_bus_ids(self):
        return [BDF.upper()] * self.devices

    def mem_info(self, device=0):
        return (self.free, VRAM)

    def hbm_scrub(self, device=0, bytes=0, **kwargs):
        self.calls.append(dict(device=device, bytes=bytes, **kwargs))
        if self.during:
            self.during()
        tested = bytes if self.tested is None else self.tested
        return _clean_result(tested, bytes_requested=bytes, **self.over)

    def run_probe(self, device=0, hbm_bytes=0):
        return {"wave_ok": True, "mfma_ok": True, "lds_ok": True,
                "hbm_copy_ok": True, "hbm_mismatches": 0, "hbm_first_bad": -1,
                "mfma_tflops": 2000.0, "hbm_gbps": 6200.0, "healthy": True}


def _write_ecc(sysroot, ue, ce, extra=""):
    d = sysroot / "sys" / "bus" / "pci" / "devices" / BDF / "ras"
    d.mkdir(parents=True, exist_ok=True)
    (d / "umc_err_count").write_text(f"{extra}ue: {ue}\nce: {ce}\n")


def test_clean_scrub_is_healthy(tmp_path):
    stub = _ScrubStub()
    res = native.hbm_scrub(device=0, bytes=1 << 30, sysroot=str(tmp_path),
                           mod=stub)
    assert stub.calls == [{"device": 0, "bytes": 1 << 30}]
    assert res["healthy"] is True
    assert res["violations"] == [] and res["warnings"] == []
    assert res["ecc"] is None  # no counter file under this sysroot


def test_bad_ranges_give_one_violation_line_each(tmp_path):
    first = {"pattern": "checker", "step": 1, "index": 0x420000 + 5, "word": 2,
             "got": 0x55555155, "expected": 0x55555555}
    ranges = [
        {"start": 0x4200000, "end": 0x43FFFFF, "mismatches": 3, "slab": 0,
         "device_address": 0x7F0004200000, "first": first},
        {"start": 0x10000000, "end": 0x103FFFFF, "mismatches": 70000, "slab": 1,
         "device_address": 0x7F0110000000, "first": None},
    ]
    stub = _ScrubStub(over={"bad_ranges": ranges, "mismatches": 70003,
                            "ok": False})
    res = native.hbm_scrub(bytes=1 << 30, sysroot=str(tmp_path), mod=stub)
    assert res["healthy"] is False
    assert res["violations"] == [
        "hbm_scrub: 3 bad elements in bytes 0x4200000-0x43fffff "
        "(pattern checker step 1, bits 0x00000400 in word 2)",
        "hbm_scrub: 70000 bad elements in bytes 0x10000000-0x103fffff",
    ]


def test_overwritten_guard_is_a_violation(tmp_path):
    stub = _ScrubStub(over={"guard_ok": False, "ok": False})
    res = native.hbm_scrub(bytes=1 << 30, sysroot=str(tmp_path), mod=stub)
    assert res["healthy"] is False
    assert res["violations"] == ["hbm_scrub: guard band overwritten"]


@pytest.mark.parametrize("bytes_arg", [None, "all"])
def test_all_takes_free_vram_less_the_reserve(tmp_path, bytes_arg):
    free = VRAM - (3 << 30) + 8   # not a multiple of 16
    stub = _ScrubStub(free=free)
    res = native.hbm_scrub(bytes=bytes_arg, reserve_bytes=1 << 30,
                           sysroot=str(tmp_path), mod=stub)
    want = (free - (1 << 30)) // 16 * 16
    assert stub.calls[0]["bytes"] == want
    assert want >= 0.9 * VRAM and res["warnings"] == [] and res["healthy"]


def test_all_with_nothing_left_raises(tmp_path):
    with pytest.raises(ValueError):
        native.hbm_scrub(bytes="all", sysroot=str(tmp_path),
                         mod=_ScrubStub(free=1 << 30))


def test_partial_scrub_of_all_only_warns(tmp_path):
    # a busy node: little free; and a slab that was refused
    for stub in (_ScrubStub(free=100 << 30),
                 _ScrubStub(tested=200 << 30)):
        res = native.hbm_scrub(bytes="all", sysroot=str(tmp_path), mod=stub)
        tested = res["bytes_tested"]
        assert tested < 0.9 * VRAM
        assert res["warnings"] == [
            f"hbm_scrub_partial: tested {tested} of {VRAM} bytes"]
        assert res["violations"] == [] and res["healthy"] is True


def test_explicit_byte_count_never_warns_partial(tmp_path):
    res = native.hbm_scrub(bytes=1 << 20, sysroot=str(tmp_path),
                           mod=_ScrubStub())
    assert res["warnings"] == []


def test_ecc_unchanged_is_reported_and_clean(tmp_path):
    _write_ecc(tmp_path, 0, 7, extra="junk line\nother: 5\n")
    res = native.hbm_scrub(bytes=1 << 20, sysroot=str(tmp_path),
                           mod=_ScrubStub())
    assert res["ecc"] == {"before": {"ue": 0, "ce": 7},
                          "after": {"ue": 0, "ce": 7}}
    assert res["healthy"] and not res["warnings"] and not res["violations"]


def test_ce_rise_warns_with_the_count(tmp_path):
    _write_ecc(tmp_path, 0, 7)
    stub = _ScrubStub(during=lambda: _write_ecc(tmp_path, 0, 12))
    res = native.hbm_scrub(bytes=1 << 20, sysroot=str(tmp_path), mod=stub)
    assert res["ecc"]["after"] == {"ue": 0, "ce": 12}
    assert res["warnings"] == [
        "hbm_scrub_ecc: 5 corrected ECC errors during the scrub"]
    assert res["violations"] == [] and res["healthy"] is True


def test_ue_rise_is_a_violation(tmp_path):
    _write_ecc(tmp_path, 1, 7)
    stub = _ScrubStub(during=lambda: _write_ecc(tmp_path, 3, 7))
    res = native.hbm_scrub(bytes=1 << 20, sysroot=str(tmp_path), mod=stub)
    assert res["violations"] == [
        "hbm_scrub: 2 uncorrectable ECC errors during the scrub"]
    assert res["healthy"] is False and res["warnings"] == []


@pytest.mark.parametrize("text", ["", "ue: x\nce: 1\n", "ce: 1\n", "garbage"])
def test_unparseable_ecc_file_is_none(tmp_path, text):
    _write_ecc(tmp_path, 0, 0)
    path = tmp_path / "sys/bus/pci/devices" / BDF / "ras" / "umc_err_count"
    path.write_text(text)
    assert native.read_ecc_counts(BDF, str(tmp_path)) is None
    res = native.hbm_scrub(bytes=1 << 20, sysroot=str(tmp_path),
                           mod=_ScrubStub())
    assert res["ecc"] is None and res["healthy"] is True


def test_missing_ecc_file_is_none(tmp_path):
    assert native.read_ecc_counts(BDF, str(tmp_path)) is None


# ---------------- env switch and deep_health_probe ----------------


@pytest.mark.parametrize("value,want", [
    (None, None), ("", None), ("0", None), (" 0 ", None), ("all", "all"),
    ("ALL", "all"), ("1073741824", 1 << 30), ("0x40000000", 1 << 30),
])
def test_env_parsing(monkeypatch, value, want):
    if value is None:
        monkeypatch.delenv(native.HBM_SCRUB_ENV, raising=False)
    else:
        monkeypatch.setenv(native.HBM_SCRUB_ENV, value)
    assert native.hbm_scrub_bytes_from_env() == want
    # an explicit argument wins over the environment
    assert native.hbm_scrub_bytes_from_env(4096) == 4096
    assert native.hbm_scrub_bytes_from_env(0) is None
    assert native.hbm_scrub_bytes_from_env("all") == "all"


@pytest.mark.parametrize("value", ["lots", "-16", "1e9"])
def test_env_garbage_raises(monkeypatch, value):
    monkeypatch.setenv(native.HBM_SCRUB_ENV, value)
    with pytest.raises(ValueError):
        native.hbm_scrub_bytes_from_env()


def _probe_with(monkeypatch, stub, **kwargs):
    monkeypatch.delenv(native.CU_SWEEP_ENV, raising=False)
    monkeypatch.setattr(native, "load_healthprobe",
                        lambda required=None: stub)
    return native.deep_health_probe(mfma_floor_tflops=0, hbm_floor_gbps=0,
                                    **kwargs)


def test_deep_probe_without_the_option_is_key_for_key_as_before(monkeypatch):
    monkeypatch.delenv(native.HBM_SCRUB_ENV, raising=False)
    stub = _ScrubStub()
    res = _probe_with(monkeypatch, stub)
    assert stub.calls == []
    assert set(res) == set(stub.run_probe()) | {"floors", "floor_violations"}
    assert res["healthy"] is True and res["floor_violations"] == []


def test_deep_probe_with_the_option_carries_the_scrub(monkeypatch):
    monkeypatch.delenv(native.HBM_SCRUB_ENV, raising=False)
    stub = _ScrubStub()
    res = _probe_with(monkeypatch, stub, hbm_scrub_bytes=1 << 26)
    assert stub.calls == [{"device": 0, "bytes": 1 << 26}]
    assert set(res) == (set(stub.run_probe()) |
                        {"floors", "floor_violations", "hbm_scrub"})
    assert res["hbm_scrub"]["healthy"] and res["healthy"] is True


def test_deep_probe_reads_the_env(monkeypatch):
    monkeypatch.setenv(native.HBM_SCRUB_ENV, str(1 << 24))
    stub = _ScrubStub()
    res = _probe_with(monkeypatch, stub)
    assert stub.calls[0]["bytes"] == 1 << 24 and "hbm_scrub" in res
    # and an explicit 0 turns it off again
    stub2 = _ScrubStub()
    assert "hbm_scrub" not in _probe_with(monkeypatch, stub2, hbm_scrub_bytes=0)
    assert stub2.calls == []


def test_deep_probe_joins_violations_and_warnings(monkeypatch):
    monkeypatch.delenv(native.HBM_SCRUB_ENV, raising=False)
    stub = _ScrubStub(over={"guard_ok": False, "ok": False}, free=100 << 30)
    res = _probe_with(monkeypatch, stub, hbm_scrub_bytes="all")
    assert res["healthy"] is False
    assert res["floor_violations"] == ["hbm_scrub: guard band overwritten"]
    assert len(res["warnings"]) == 1
    assert res["warnings"][0].startswith("hbm_scrub_partial: tested ")


# ---------------- the plugin never scrubs ----------------


class _PluginStub(_ScrubStub):
    """What the plugin's deep probe may touch, with every call recorded."""

    def __init__(self):
        super().__init__()
        self.probes = []
        self.sweeps = []

    def pci_bus_ids(self):
        return []  # the plugin falls back to the rank of the device id

    def run_probe(self, device=0, hbm_bytes=0):
        self.probes.append(device)
        return super().run_probe(device, hbm_bytes)

    def cu_sweep(self, device=0, reps=0, inject=None):
        self.sweeps.append(device)
        return {"bad": [], "ok": True, "coverage_complete": True,
                "cu_count": 256, "cus_covered": 256, "simds_covered": 1024}


@pytest.mark.parametrize("cu_sweep", [False, True])
@pytest.mark.parametrize("value", ["all", str(1 << 30)])
def test_plugin_ignores_the_env(monkeypatch, tmp_path, cu_sweep, value):
    """Heartbeat and PreStart probe a live node, where the pods own the VRAM:
    with AMDXDP_HBM_SCRUB_BYTES set on the DaemonSet they still never scrub."""
    from k8s_device_plugin_amd.plugin import AMDGPUPlugin
    from k8s_device_plugin_amd.protos import deviceplugin as dp
    from k8s_device_plugin_amd.testing.fakesysfs import build_mi355x_node

    monkeypatch.setenv(native.HBM_SCRUB_ENV, value)
    monkeypatch.delenv(native.CU_SWEEP_ENV, raising=False)
    monkeypatch.delenv(native.CU_SWEEP_INJECT_ENV, raising=False)
    stub = _PluginStub()
    monkeypatch.setattr(native, "load_healthprobe", lambda required=None: stub)
    # the same env does turn the scrub on for a direct call
    assert "hbm_scrub" in native.deep_health_probe()
    assert len(stub.calls) == 1
    stub.calls.clear()
    stub.probes.clear()

    fs = build_mi355x_node(str(tmp_path / "n"), n_gpus=1)
    dev_root = os.path.join(fs.paths.root, "dev")
    os.makedirs(os.path.join(dev_root, "dri"), exist_ok=True)
    open(os.path.join(dev_root, "kfd"), "w").close()
    plugin = AMDGPUPlugin(resource="gpu", paths=fs.paths, dev_root=dev_root,
                          deep_probe_every=1, prestart_probe=True,
                          prestart_deep=True, deep_cu_sweep=cu_sweep)
    plugin.start()
    try:
        plugin.heartbeat()
        assert stub.probes == [0] and stub.calls == []
        assert not plugin._deep_failed

        dev = next(iter(plugin.devices.values()))
        open(os.path.join(dev_root, "dri", f"renderD{dev.render_d}"),
             "w").close()

        class _Ctx:
            def abort(self, code, msg):
                raise AssertionError(f"aborted: {msg}")

        plugin.PreStartContainer(
            dp.PreStartContainerRequest(devices_ids=[dev.id]), _Ctx())
        assert stub.probes == [0, 0] and stub.calls == []
        assert bool(stub.sweeps) == cu_sweep
    finally:
        plugin.stop()


# ---------------- the console script ----------------


def _run_cli(monkeypatch, stub, argv, capsys):
    def load(required=None):
        if stub is None:
            raise native.NativeExtensionMissing("not built")
        return stub
    monkeypatch.setattr(native, "load_healthprobe", load)
    code = cli.scrub_main(argv)
    return code, capsys.readouterr()


def test_cli_exit_0_when_healthy(monkeypatch, capsys, tmp_path):
    stub = _ScrubStub()
    code, out = _run_cli(monkeypatch, stub,
                         ["--bytes", "0x100000", "--sysroot", str(tmp_path)],
                         capsys)
    assert code == 0 and "healthy" in out.out
    assert stub.calls == [{"device": 0, "bytes": 1 << 20}]


def test_cli_exit_1_when_unhealthy(monkeypatch, capsys, tmp_path):
    stub = _ScrubStub(over={"guard_ok": False, "ok": False})
    code, out = _run_cli(monkeypatch, stub,
                         ["--bytes", "1048576", "--sysroot", str(tmp_path)],
                         capsys)
    assert code == 1
    assert "UNHEALTHY" in out.out and "guard band overwritten" in out.out


def test_cli_exit_2_without_extension_or_gpu(monkeypatch, capsys):
    assert _run_cli(monkeypatch, None, [], capsys)[0] == 2
    assert _run_cli(monkeypatch, _ScrubStub(devices=0), [], capsys)[0] == 2
    assert _run_cli(monkeypatch, _ScrubStub(), ["--device", "3"], capsys)[0] == 2


class _FailingStub(_ScrubStub):
    """Device 1 cannot be scrubbed, device 2 is unhealthy when told to be."""

    def __init__(self, error, sick=False):
        super().__init__(devices=3)
        self.error = error
        self.sick = sick

    def hbm_scrub(self, device=0, bytes=0, **kwargs):
        if device == 1:
            raise self.error
        res = super().hbm_scrub(device=device, bytes=bytes, **kwargs)
        if device == 2 and self.sick:
            res.update(guard_ok=False, ok=False)
        return res


@pytest.mark.parametrize("error", [
    ValueError("bytes must be a positive multiple of 16"),
    RuntimeError("hbm_scrub: no slab could be allocated"),
])
def test_cli_a_scrub_that_could_not_run_is_exit_2_not_1(monkeypatch, capsys,
                                                       tmp_path, error):
    """Could not look is not a sick GPU: the other devices still run, the
    JSON keeps what was collected, and the exit code is 2."""
    stub = _FailingStub(error)
    code, out = _run_cli(
        monkeypatch, stub,
        ["--device", "all", "--bytes", "1048576", "--json", "--sysroot",
         str(tmp_path)], capsys)
    assert code == 2
    assert [c["device"] for c in stub.calls] == [0, 2]
    doc = json.loads(out.out)
    assert doc["0"]["healthy"] is True and doc["2"]["healthy"] is True
    assert doc["1"] == {"error": str(error), "healthy": None}
    assert f"device 1: {error}" in out.err
    # an unhealthy GPU among them still wins
    code, _ = _run_cli(
        monkeypatch, _FailingStub(error, sick=True),
        ["--device", "all", "--bytes", "1048576", "--sysroot", str(tmp_path)],
        capsys)
    assert code == 1


def test_cli_all_with_nothing_free_is_exit_2(monkeypatch, capsys, tmp_path):
    code, out = _run_cli(monkeypatch, _ScrubStub(free=1 << 30),
                         ["--sysroot", str(tmp_path)], capsys)
    assert code == 2 and "leaves nothing to test" in out.err


def test_cli_all_devices_json_patterns_and_reserve(monkeypatch, capsys,
                                                   tmp_path):
    stub = _ScrubStub(devices=8)
    code, out = _run_cli(
        monkeypatch, stub,
        ["--device", "all", "--reserve-bytes", str(4 << 30), "--patterns",
         "address,random", "--json", "--sysroot", str(tmp_path)], capsys)
    assert code == 0
    assert [c["device"] for c in stub.calls] == list(range(8))
    want = (stub.free - (4 << 30)) // 16 * 16
    assert all(c["bytes"] == want and c["patterns"] == ["address", "random"]
               for c in stub.calls)
    doc = json.loads(out.out)
    assert sorted(doc) == [str(d) for d in range(8)]
    assert all(r["healthy"] for r in doc.values())


def test_console_script_is_declared():
    with open(os.path.join(REPO, "setup.py")) as f:
        assert ("amd-hbm-scrub=k8s_device_plugin_amd.cli:scrub_main"
                in f.read())
    # the static metadata wins over setup.py where both exist
    with open(os.path.join(REPO, "pyproject.toml")) as f:
        assert ('amd-hbm-scrub = "k8s_device_plugin_amd.cli:scrub_main"'
                in f.read())

"""The default deep-probe checks (HBM copy, LDS, peak MFMA), CPU side: the
fill pattern under the host sanitizers, the argument checks of the three
test-facing entries (they reject before any HIP call) and the health policy
for a copy that differs from the pattern.

The kernels themselves run on the GPU: tests/test_probe_kernels_gpu.py.
"""

import os
import shutil
import subprocess

import pytest

import k8s_device_plugin_amd.native as native
from k8s_device_plugin_amd.native import build as nb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_DIR = os.path.join(REPO, "k8s_device_plugin_amd", "native")


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


def test_hbm_pattern_is_a_build_input():
    assert os.path.join(nb.PKG_DIR, "hbm_pattern.h") in nb._HIP_HEADERS


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_hbm_pattern_under_sanitizers(tmp_path):
    """A stand-alone program (its own main) checks that the pattern is exact
    in fp32 at the field boundaries and that no power-of-two or 65536*m
    displacement maps an element onto an equal one, under ASan + UBSan."""
    exe = str(tmp_path / "hbm_pattern_check")
    # static runtimes, as for sweep_table_check (tests/test_cu_sweep.py)
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-static-libasan",
         "-static-libubsan", f"-I{NATIVE_DIR}",
         os.path.join(REPO, "tests", "native", "hbm_pattern_check.cpp"),
         "-o", exe],
        check=True, capture_output=True, text=True,
    )
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ok" in run.stdout


# ---------------- argument checks: before any HIP call ----------------

_N = 4 * 262144


@pytest.mark.parametrize("kwargs", [
    {"n": 0},
    {"n": -1},
    {"n": (1 << 32) + 1},
    {"n": 1, "threads": 0},
    {"n": 1, "threads": 32},
    {"n": 1, "threads": 100},
    {"n": 1, "threads": 1088},
    {"n": 1, "blocks": -1},
    {"n": 1025, "blocks": 1},                # 4 * 1 * 256 < n
    {"n": 769, "blocks": 3, "threads": 64},  # 4 * 3 * 64 < n
    {"n": 1, "guard": -1},
    {"n": 1, "guard": (1 << 20) + 1},
    {"n": (1 << 21) + 1, "return_data": True},
    {"n": _N, "corrupt": ("flip", _N, 0, 0)},
    {"n": _N, "corrupt": ("flip", -1, 0, 0)},
    {"n": _N, "corrupt": ("flip", 0, 4, 0)},
    {"n": _N, "corrupt": ("flip", 0, -1, 0)},
    {"n": _N, "corrupt": ("flip", 0, 0, 32)},
    {"n": _N, "corrupt": ("flip", 0, 0)},
    {"n": _N, "corrupt": ("alias", 0, 0)},
    {"n": _N, "corrupt": ("alias", _N - 1, 1)},
    {"n": _N, "corrupt": ("alias", 0, -1)},
    {"n": _N, "corrupt": ("alias", _N, -1)},
    {"n": _N, "corrupt": ("alias", 0, 1, 2)},
    {"n": _N, "corrupt": ("swap", 0, 1)},
    {"n": _N, "corrupt": ()},
])
def test_hbm_copy_check_rejects_bad_arguments(probe_mod, kwargs):
    with pytest.raises(ValueError):
        probe_mod.hbm_copy_check(device=0, **kwargs)


@pytest.mark.parametrize("kwargs", [
    {"lds_bytes": 0},
    {"lds_bytes": -4},
    {"lds_bytes": 6},
    {"lds_bytes": 1023},
    {"lds_bytes": 1024, "threads": 0},
    {"lds_bytes": 1024, "threads": 32},
    {"lds_bytes": 1024, "threads": 96},
    {"lds_bytes": 1024, "threads": 1088},
    {"lds_bytes": 1024, "blocks": 0},
    {"lds_bytes": 1024, "blocks": -1},
    {"lds_bytes": 1024, "corrupt": (1, 0, 1)},           # only block 0 exists
    {"lds_bytes": 1024, "blocks": 3, "corrupt": (3, 0, 1)},
    {"lds_bytes": 1024, "corrupt": (-1, 0, 1)},
    {"lds_bytes": 1024, "corrupt": (0, 256, 1)},         # words 0..255
    {"lds_bytes": 1024, "corrupt": (0, -1, 1)},
    {"lds_bytes": 1024, "corrupt": (0, 0, 0)},           # flips nothing
    {"lds_bytes": 1024, "corrupt": (0, 0, 1 << 32)},
    {"lds_bytes": 1024, "corrupt": (0, 0)},
])
def test_lds_check_rejects_bad_arguments(probe_mod, kwargs):
    with pytest.raises(ValueError):
        probe_mod.lds_check(device=0, **kwargs)


@pytest.mark.parametrize("kwargs", [
    {"iters": 0},
    {"iters": -1},
    {"iters": (1 << 20) + 1},
    {"iters": 1, "blocks": 0},
    {"iters": 1, "blocks": 4097},
])
def test_mfma_peak_check_rejects_bad_arguments(probe_mod, kwargs):
    with pytest.raises(ValueError):
        probe_mod.mfma_peak_check(device=0, **kwargs)


# ---------------- policy (stubbed probe module) ----------------


class _BadCopyStub:
    """run_probe as the module reports a copy with three wrong elements."""

    def run_probe(self, device=0, hbm_bytes=0):
        return {"wave_ok": True, "mfma_ok": True, "lds_ok": True,
                "hbm_copy_ok": False, "hbm_mismatches": 3,
                "hbm_first_bad": 65536, "mfma_tflops": 2000.0,
                "hbm_gbps": 6200.0, "healthy": False}


def test_wrong_copy_is_unhealthy_and_named(monkeypatch):
    monkeypatch.delenv(native.CU_SWEEP_ENV, raising=False)
    monkeypatch.setattr(native, "load_healthprobe",
                        lambda required=None: _BadCopyStub())
    # floors off: the copy alone decides
    res = native.deep_health_probe(mfma_floor_tflops=0, hbm_floor_gbps=0)
    assert res["healthy"] is False
    assert res["hbm_mismatches"] == 3 and res["hbm_first_bad"] == 65536
    assert res["floor_violations"] == [
        "hbm_copy: 3 elements differ from the pattern, first at 65536"
    ]

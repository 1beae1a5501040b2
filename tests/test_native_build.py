"""native/build.py staleness rule and sweep build; the probe's argument
check that needs no GPU."""

import os
import shutil

import pytest

from k8s_device_plugin_amd.native import build as nb
from k8s_device_plugin_amd.native import load_healthprobe


def test_needs_build_any_newer_input(tmp_path):
    out, a, b = (str(tmp_path / n) for n in ("out", "a", "b"))
    assert nb._needs_build(out, a, b)  # output missing
    for path in (out, a, b):
        open(path, "w").close()
    os.utime(out, (1000, 1000))
    os.utime(a, (900, 900))
    os.utime(b, (1000, 1000))
    assert not nb._needs_build(out, a, b)  # older or equal: up to date
    os.utime(b, (1001, 1001))
    assert nb._needs_build(out, a, b)  # second input newer
    os.utime(b, (900, 900))
    os.utime(a, (1001, 1001))
    assert nb._needs_build(out, a, b)  # first input newer


def test_pref_alloc_header_is_a_fastserver_build_input(monkeypatch):
    checked = []
    monkeypatch.setattr(
        nb, "_needs_build", lambda out, *inputs: checked.extend(inputs))
    nb.build_fastserver()  # _needs_build is falsy: nothing is compiled
    assert os.path.join(nb.PKG_DIR, "pref_alloc.h") in checked


@pytest.mark.skipif(shutil.which(nb.HIPCC) is None, reason="no hipcc")
def test_build_sweeps_produces_both_binaries():
    outs = nb.build_sweeps()
    assert [os.path.basename(o) for o in outs] == ["mfma_bench", "hbm_bench"]
    for out in outs:
        assert os.access(out, os.X_OK), out


@pytest.mark.parametrize("hbm_bytes", [0, 15])
def test_run_probe_rejects_less_than_one_float4(hbm_bytes):
    """Rejected before any HIP call, so it holds without a GPU."""
    try:  # torch's HIP runtime must load first (see __graft_entry__.build)
        import torch  # noqa: F401
    except ImportError:
        pass
    mod = load_healthprobe(required=False)
    if mod is None:
        pytest.skip("_healthprobe.so not built (no hipcc)")
    with pytest.raises(ValueError):
        mod.run_probe(hbm_bytes=hbm_bytes)

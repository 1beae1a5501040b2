"""CU sweep on a real MI355X (pytest -m gpu): exact known-answer products
of every matrix dtype path on every SIMD of every CU, the place of each
wave read from the hardware id registers.

The sweep has no problem size to shrink: one launch of cu_count blocks is
its smallest case, a few milliseconds of GPU time.
"""

import pytest

pytestmark = pytest.mark.gpu

PIPES = ["bf16_16", "bf16_32", "f16_16", "fp8_16", "i8_16", "mxfp8_16"]


@pytest.fixture(scope="module")
def probe_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from k8s_device_plugin_amd.native import load_healthprobe

    return load_healthprobe(required=True)


@pytest.fixture(scope="module")
def plain_probe(probe_mod):
    """The deep probe as it is without the sweep: no argument, no env."""
    import os

    from k8s_device_plugin_amd.native import (
        CU_SWEEP_ENV,
        CU_SWEEP_INJECT_ENV,
        deep_health_probe,
    )

    assert CU_SWEEP_ENV not in os.environ
    assert CU_SWEEP_INJECT_ENV not in os.environ
    return deep_health_probe(device=0, hbm_bytes=1 << 28)


def test_healthy_sweep_covers_every_simd(probe_mod, plain_probe):
    cu_count = plain_probe["cu_count"]
    res = probe_mod.cu_sweep(device=0)
    print({k: v for k, v in res.items() if k != "records"})
    assert res["ok"] and res["bad"] == [], res["bad"]
    assert res["coverage_complete"], (
        res["cus_covered"], res["simds_covered"], res["uncovered"])
    assert res["uncovered"] == []
    assert res["cu_count"] == cu_count
    assert res["cus_covered"] == cu_count
    assert res["simds_covered"] == 4 * cu_count
    assert 1 <= res["launches"] <= 4
    assert res["waves_checked"] == 4 * cu_count * res["launches"]
    assert len(res["records"]) == res["waves_checked"]
    # every dtype path ran and matched bit for bit, which is also the proof
    # that each dtype's lane map is right on hardware
    assert res["pipes"] == PIPES
    assert all(r[2] == 0 for r in res["records"])
    assert res["sweep_ms"] > 0
    # every CU shows exactly SIMDs 0-3
    simds = {}
    for hw_id, xcc_id, *_ in res["records"]:
        *cu, simd = probe_mod.decode_hw_id(hw_id, xcc_id)
        simds.setdefault(tuple(cu), set()).add(simd)
    assert len(simds) == cu_count
    assert all(s == {0, 1, 2, 3} for s in simds.values())


@pytest.mark.parametrize("where,wave,pipe", [
    ("first", 0, 0),   # first pipe
    ("middle", 2, 3),  # a middle pipe
    ("last", 3, 5),    # last pipe, block cu_count - 1, last wave
])
def test_injected_bad_pipe_is_found_and_named(probe_mod, plain_probe,
                                              where, wave, pipe):
    cu_count = plain_probe["cu_count"]
    block = {"first": 0, "middle": cu_count // 2, "last": cu_count - 1}[where]
    res = probe_mod.cu_sweep(device=0, inject=(block, wave, pipe))
    assert not res["ok"]
    assert len(res["bad"]) == 1, res["bad"]
    bad = res["bad"][0]
    assert bad["pipes"] == [PIPES[pipe]]
    rec = res["records"][block * 4 + wave]
    assert rec[2] == 1 << pipe
    assert (bad["xcc"], bad["se"], bad["sh"], bad["cu"], bad["simd"]) == \
        probe_mod.decode_hw_id(rec[0], rec[1])
    first = bad["first"]
    assert first["pipe"] == PIPES[pipe]
    assert first["got"] != first["expected"]
    # the hook flips one bit of one register in one lane, nothing else
    assert bin(first["got"] ^ first["expected"]).count("1") == 1
    assert bad["bad_lanes"] == 1 << first["lane"]
    assert sum(1 for r in res["records"] if r[2]) == res["launches"]
    # the injection does not disturb the coverage
    assert res["coverage_complete"]


def test_deep_health_probe_with_sweep(probe_mod, plain_probe):
    from k8s_device_plugin_amd.native import deep_health_probe

    assert plain_probe["healthy"], plain_probe
    assert "cu_sweep" not in plain_probe
    res = deep_health_probe(device=0, hbm_bytes=1 << 28, cu_sweep=True)
    assert res["healthy"], res["floor_violations"]
    assert res["cu_sweep"]["ok"] and res["cu_sweep"]["coverage_complete"]
    assert "warnings" not in res
    assert set(plain_probe) <= set(res)  # every pre-existing key is there


def test_deep_health_probe_inject_env(probe_mod, plain_probe, monkeypatch):
    from k8s_device_plugin_amd.native import (
        CU_SWEEP_ENV,
        CU_SWEEP_INJECT_ENV,
        deep_health_probe,
    )

    monkeypatch.setenv(CU_SWEEP_ENV, "1")
    monkeypatch.setenv(CU_SWEEP_INJECT_ENV, "1:1:4")
    res = deep_health_probe(device=0, hbm_bytes=1 << 28)
    assert not res["healthy"]
    lines = [v for v in res["floor_violations"] if v.startswith("cu_sweep:")]
    assert len(lines) == 1 and lines[0].endswith("failed i8_16"), lines

"""bench.py command line: the lean plain run, --full and --dump-outputs."""

import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*argv):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    return subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), *argv],
        capture_output=True, text=True, timeout=300, env=env, cwd=REPO,
    )


def _run(*argv):
    out = _bench(*argv)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_reproducible_outputs(tmp_path):
    args = ("--gpus", "2", "--steps", "7", "--warmup", "2", "--sysfs", "fake")
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    rec = _run(*args, "--dump-outputs", a)
    _run(*args, "--dump-outputs", b)

    assert rec["steps"] == 7 and rec["ms_per_step"] > 0
    # seven Allocate round trips were recorded inside the timed window
    assert rec["config"]["timed_allocates"] == 7
    assert rec["value"] == pytest.approx(
        2 * 1e3 / rec["ms_per_step"], rel=1e-2
    )
    # the extras did not run
    assert rec["config"]["native_client_allocate_p50_us"] is None
    assert rec["config"]["curve"] is None
    assert rec["config"]["deep_probe"] is None

    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert "allocate_response_bytes.npy" in names
    assert "granted_device_indices.npy" in names
    total = 0
    for name in names:
        x, y = np.load(os.path.join(a, name)), np.load(os.path.join(b, name))
        assert x.dtype in (np.float32, np.float64)
        assert x.size > 0 and np.array_equal(x, y), name
        total += x.nbytes
    assert total <= 64 << 20

    # the stored bytes are the response the last step received
    from k8s_device_plugin_amd.protos import deviceplugin as dp

    raw = np.load(os.path.join(a, "allocate_response_bytes.npy"))
    resp = dp.AllocateResponse.FromString(bytes(raw.astype(np.uint8)))
    assert len(resp.container_responses[0].devices) == 1 + 2 * 2
    assert len(np.load(os.path.join(a, "granted_device_indices.npy"))) == 2
    # and the decoded view agrees with them
    nodes = np.load(os.path.join(a, "allocate_device_nodes.npy"))
    assert nodes.shape == (5, 3)
    assert sorted(nodes[:, 0]) == [0, 1, 1, 2, 2]
    counts = np.load(os.path.join(a, "allocate_counts.npy"))
    cr = resp.container_responses[0]
    assert list(counts) == [5, len(cr.mounts), len(cr.envs),
                            len(cr.annotations), len(cr.cdi_devices)]


def test_extras_need_full():
    out = _bench("--curve", "1,2")
    assert out.returncode == 2
    assert "--full" in out.stderr


def test_full_runs_the_extras():
    rec = _run(
        "--full", "--sysfs", "fake", "--curve", "1,2",
        "--steps", "5", "--warmup", "1",
    )
    assert [c["n"] for c in rec["config"]["curve"]] == [1, 2]
    for entry in rec["config"]["curve"]:
        assert entry["ms_per_step"] > 0 and entry["allocate_p50_us"] > 0
    # the compiled client is built with g++ and loads the libnghttp2 that
    # the native server uses too: where both are there it must have run
    p50 = rec["config"]["native_client_allocate_p50_us"]
    if rec["config"]["server"] == "native" and shutil.which("g++"):
        assert p50 is not None and p50 > 0
        assert rec["config"]["native_client_preferred_p50_us"] > 0
    else:
        assert p50 is None

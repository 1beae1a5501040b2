"""native/pref_alloc.h as a stand-alone program under ASan + UBSan.

The Python policy writes the case file (its exported state and its own
answers); tests/native/pref_alloc_check.cpp loads each state, searches
with both scorers and must give the same id lists.
"""

import glob
import os
import random
import shutil
import subprocess

import pytest

from k8s_device_plugin_amd.allocator import AllocationError, BestEffortPolicy
from k8s_device_plugin_amd.testing.fakesysfs import build_mi355x_node
from k8s_device_plugin_amd.topology import KFDTopology, discover_gpus

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_DIR = os.path.join(REPO, "k8s_device_plugin_amd", "native")

SEVERED = {(2, 7), (2, 8), (3, 9)}  # test_non_uniform_topology_uses_generic_path

# name -> (n_gpus, partitions per GPU, GPU-GPU links to remove, uniform)
TOPOLOGIES = {
    "2x1": (2, 1, (), True),               # single-node groups, new_size == 1 seeds
    "4x4": (4, 4, (), True),               # seed completes in a group; spill-over
    "8x8": (8, 8, (), True),               # 64 partitions: 30-of-64, 63-of-64
    "4x4-severed": (4, 4, SEVERED, False),  # per-node scorer as loaded
    "4x1-nolinks": (4, 1, "all", True),    # empty weight table, still ready
}


def _remove_links(fs, which):
    """Remove both directions of the given GPU-GPU links ("all": every one)."""
    removed = 0
    for props in glob.glob(os.path.join(fs.paths.kfd_topology_nodes, "*",
                                        "io_links", "*", "properties")):
        p = dict(line.split()[:2] for line in open(props) if line.strip())
        pair = tuple(sorted((int(p["node_from"]), int(p["node_to"]))))
        gpu_gpu = min(pair) >= 2  # nodes 0 and 1 are the CPUs
        if (gpu_gpu if which == "all" else pair in which):
            shutil.rmtree(os.path.dirname(props))
            removed += 1
    return removed


def _requests(ids, rng):
    """(name, available, required, size, must_fail) for one topology."""
    for size in range(1, len(ids) + 1):
        yield f"full-{size}", ids, [], size, False
    for i in range(40):  # drawn as in test_fastserver_fuzz.py
        available = rng.sample(ids, rng.randint(2, len(ids)))
        size = rng.randint(1, len(available))
        required = rng.sample(available, rng.randint(0, min(2, size)))
        yield f"random-{i}", available, required, size, False
    yield "size-0", ids, [], 0, True
    yield "size-gt-available", ids[:2], [], 3, True
    yield "required-gt-size", ids, ids[:2], 1, True
    yield ("required-not-available", ids[1:] + ["unknown-a", "unknown-b"],
           ids[:1], 2, True)
    yield "unknown-id-available", ids + ["not-a-dev"], [], 2, False


def _write_cases(path, root):
    rng = random.Random(0x9FA11)
    n_cases = 0
    with open(path, "w") as f:
        def put(*tokens):
            tokens = [str(t) for t in tokens]
            assert all(t and not any(c.isspace() for c in t) for t in tokens)
            f.write(" ".join(tokens) + "\n")

        for name, (n_gpus, parts, cut, uniform) in TOPOLOGIES.items():
            fs = build_mi355x_node(
                os.path.join(root, name), n_gpus=n_gpus,
                partitions_per_gpu=parts,
                compute_partition="CPX" if parts > 1 else "SPX")
            if cut:
                assert _remove_links(fs, cut) == (
                    n_gpus * (n_gpus - 1) if cut == "all" else 2 * len(cut))
            topo = KFDTopology.load(fs.paths)
            devices = discover_gpus(fs.paths, topology=topo)
            policy = BestEffortPolicy()
            policy.init(devices.values(), topology=topo)
            assert policy._uniform == uniform, name
            groups, node_of_id, weights = policy.export_state()
            assert bool(weights) == (cut != "all"), name

            put("topology", name, int(uniform), len(groups))
            for parent, nodes in groups:
                put(parent or "-", len(nodes), *nodes)
            put(len(node_of_id))
            for dev, node in node_of_id.items():
                put(dev, node)
            put(len(weights))
            for a, b, w in weights:
                put(a, b, w)

            ids = sorted(devices)
            assert len(ids) == n_gpus * parts
            for case, available, required, size, must_fail in _requests(ids, rng):
                head = ["case", case, size, len(available), *available,
                        len(required), *required]
                try:
                    out = policy.allocate(available, required, size)
                except AllocationError:
                    put(*head, "err")
                else:
                    assert not must_fail, (name, case)
                    put(*head, "ok", len(out), *out)
                n_cases += 1
    return n_cases


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_pref_alloc_under_sanitizers(tmp_path):
    case_file = str(tmp_path / "cases.txt")
    n_cases = _write_cases(case_file, str(tmp_path))
    assert n_cases == sum(g * p + 45 for g, p, _, _ in TOPOLOGIES.values())

    exe = str(tmp_path / "pref_alloc_check")
    # the runtimes are linked statically: the dynamic ASan runtime refuses
    # to start wherever the environment preloads any other library
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-static-libasan",
         "-static-libubsan", f"-I{NATIVE_DIR}",
         os.path.join(REPO, "tests", "native", "pref_alloc_check.cpp"),
         "-o", exe],
        check=True, capture_output=True, text=True,
    )
    run = subprocess.run([exe, case_file], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, \
        run.stderr
    assert run.stdout.split() == ["pref_alloc_check:", str(n_cases), "cases", "ok"]

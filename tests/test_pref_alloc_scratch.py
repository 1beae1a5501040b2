"""native/pref_alloc.h with ONE scratch object across topologies and cases,
as a stand-alone program under ASan + UBSan.

The server keeps a single prefalloc::Scratch for every request it will ever
serve, and the allocator state under it can be replaced.  Here the Python
policy writes a case file (its exported state and its own answers) whose
ORDER is chosen to expose anything stale in that scratch: a large topology
first, then the smallest, then mid-sized ones, the large one again, a
topology with more than 20 groups (the hash-set dedup), and the smallest
once more.  tests/native/pref_alloc_scratch_check.cpp runs every case with
both scorers through one scratch and must give the policy's id lists.
"""

import os
import random
import shutil
import subprocess
import time

import pytest

from k8s_device_plugin_amd.allocator import AllocationError, BestEffortPolicy
from k8s_device_plugin_amd.testing.fakesysfs import build_mi355x_node
from k8s_device_plugin_amd.topology import KFDTopology, discover_gpus

from test_pref_alloc_native import NATIVE_DIR, REPO, SEVERED, _remove_links

# 22 single-node groups: kfd nodes 2..23 are the GPUs.  The removed links
# make some pairs cheaper than the rest, so the winner is not simply the
# first candidate generated.
SEVERED_22 = {(9, 14), (9, 20), (14, 20), (5, 17)}

# (name, n_gpus, partitions per GPU, GPU-GPU links to remove, uniform), in
# the order the one scratch meets them
SEQUENCE = [
    ("8x8", 8, 8, (), True),
    ("2x1", 2, 1, (), True),
    ("4x1-nolinks", 4, 1, "all", True),
    ("4x4", 4, 4, (), True),
    ("4x4-severed", 4, 4, SEVERED, False),
    ("8x8-again", 8, 8, (), True),
    ("22x1-severed", 22, 1, SEVERED_22, True),
    ("2x1-again", 2, 1, (), True),
]


def _requests(name, ids, parts, rng):
    """(case name, available, required, size, must_fail) for one topology."""
    n = len(ids)
    # with 22 single-node groups a large request walks up to 2^22 parent
    # sets, in the policy too: those stay small, or draw on five devices
    many_groups = name.startswith("22x1")
    pool = ids[3:8] if many_groups else ids
    yield "size-1", ids, [], 1, False
    yield "all-but-one", pool, [], len(pool) - 1, False
    if name.startswith("8x8"):
        yield "30-of-64", ids, [], 30, False
        yield "63-of-64", ids, [], 63, False
    if many_groups:
        # more than 20 groups: dedup by hash set, queue left incomplete;
        # 2 clears the set entry by entry, 3 wholesale, 4 grows it first
        for size in (2, 3, 4):
            yield f"hash-{size}", ids, [], size, False
        yield "hash-3-required", ids[1:], [ids[12], ids[7]], 3, False
    if n >= 4:
        yield "required", ids, [ids[1], ids[-1]], 3, False
        yield "required-all-but-one", pool, [pool[2]], len(pool) - 1, False
    if parts > 1:
        # one GPU with a single partition taken, and a size that ends
        # inside a group: the last group added is a prefix
        partial = ids[:1] + ids[2:]
        yield "partial-group", partial, [], parts + 2, False
        yield "partial-group-required", partial, [ids[parts]], parts + 1, False
        yield "half-of-each", ids[::2], [], parts, False
    yield "duplicate-id", pool + [pool[0]], [], len(pool) - 1, False
    yield "unknown-id", pool + ["not-a-dev"], [], len(pool) - 1, False
    yield ("duplicate-and-unknown", [ids[-1], "not-a-dev"] + ids + [ids[0]],
           ids[:1], min(2, n), False)
    yield ("unknown-in-both", pool + ["not-a-dev"], ["not-a-dev"], len(pool),
           False)
    for i in range(12):  # drawn as in test_fastserver_fuzz.py
        available = rng.sample(ids, rng.randint(2, n))
        size = rng.randint(1, min(len(available), 4 if many_groups else n))
        required = rng.sample(available, rng.randint(0, min(2, size)))
        yield f"random-{i}", available, required, size, False
    yield "size-0", ids, [], 0, True
    yield "size-gt-available", ids[:2], [], 3, True
    yield "required-gt-size", ids, ids[:2], 1, True
    yield ("required-not-available", ids[1:] + ["unknown-a", "unknown-b"],
           ids[:1], 2, True)


def _write_cases(path, root):
    rng = random.Random(0x5C7A7C4)
    n_cases = 0
    answers = {}
    with open(path, "w") as f:
        def put(*tokens):
            tokens = [str(t) for t in tokens]
            assert all(t and not any(c.isspace() for c in t) for t in tokens)
            f.write(" ".join(tokens) + "\n")

        for name, n_gpus, parts, cut, uniform in SEQUENCE:
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
            assert len(groups) == n_gpus

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
            for case, available, required, size, must_fail in _requests(
                    name, ids, parts, rng):
                head = ["case", case, size, len(available), *available,
                        len(required), *required]
                t0 = time.perf_counter()
                try:
                    out = policy.allocate(available, required, size)
                except AllocationError:
                    assert must_fail, (name, case)
                    put(*head, "err")
                else:
                    assert not must_fail, (name, case)
                    put(*head, "ok", len(out), *out)
                    answers[name, case] = out
                # a request the policy itself takes long over has no place
                # in a quick test
                assert time.perf_counter() - t0 < 2.0, (name, case)
                n_cases += 1
    return n_cases, answers


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_one_scratch_across_topologies_under_sanitizers(tmp_path):
    case_file = str(tmp_path / "cases.txt")
    n_cases, answers = _write_cases(case_file, str(tmp_path))
    assert n_cases > 20 * len(SEQUENCE)
    # the 22-group winner is decided by weight, not by generation order:
    # a dedup that lost or repeated parent sets would change it
    seed = answers["22x1-severed", "hash-2"]
    assert answers["22x1-severed", "hash-3"][:2] != seed
    # the scratch meets the same requests before and after the others
    for first, again in (("8x8", "8x8-again"), ("2x1", "2x1-again")):
        for case in ("size-1", "all-but-one", "required", "30-of-64"):
            assert answers.get((first, case)) == answers.get((again, case))

    exe = str(tmp_path / "pref_alloc_scratch_check")
    # the runtimes are linked statically: the dynamic ASan runtime refuses
    # to start wherever the environment preloads any other library
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-static-libasan",
         "-static-libubsan", f"-I{NATIVE_DIR}",
         os.path.join(REPO, "tests", "native", "pref_alloc_scratch_check.cpp"),
         "-o", exe],
        check=True, capture_output=True, text=True,
    )
    run = subprocess.run([exe, case_file], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, \
        run.stderr
    assert run.stdout.split() == ["pref_alloc_scratch_check:", str(n_cases),
                                  "cases", "ok"]

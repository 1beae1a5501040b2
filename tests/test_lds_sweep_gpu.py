"""LDS sweep on a real MI355X (pytest -m gpu): the march of
native/lds_march.h over the whole LDS of every CU, through the 128-, 64- and
32-bit loads and stores, the LDS-DMA and the transposed read, with the place
of each block read from the hardware id registers.

One launch at the card's full LDS is a few hundred microseconds; the small
shapes are one element, one transposed-read round, a round plus a tail, each
side of 64 KiB and the whole LDS.
"""

import os

import pytest

pytestmark = pytest.mark.gpu

PATHS = ["b128", "b64", "b32", "dma", "tr16"]
ACCESS_BYTES = {"b128": 16, "b64": 8, "b32": 4, "dma": 16, "tr16": 8}
# the pattern a corruption names, and a step of the path a reading step follows
PATTERN = {"b128": "address", "b64": "address", "b32": "address",
           "dma": "random", "tr16": "address"}
AFTER = {"b128": 0, "b64": 1, "b32": 2, "dma": 1, "tr16": 0}
SEED = 0x5EED


@pytest.fixture(scope="module")
def probe_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from k8s_device_plugin_amd.native import load_healthprobe

    return load_healthprobe(required=True)


@pytest.fixture(scope="module")
def limit(probe_mod):
    return probe_mod.shared_mem_per_block(0)


@pytest.fixture(scope="module")
def plain_probe(probe_mod):
    """The deep probe as it is without the sweep: no argument, no env."""
    from k8s_device_plugin_amd.native import (
        LDS_SWEEP_ENV,
        LDS_SWEEP_INJECT_ENV,
        deep_health_probe,
    )

    assert LDS_SWEEP_ENV not in os.environ
    assert LDS_SWEEP_INJECT_ENV not in os.environ
    return deep_health_probe(device=0, hbm_bytes=1 << 28)


def _covered(probe_mod, lds_bytes):
    return {p["name"]: p["bytes"]
            for p in probe_mod.lds_sweep_reference(lds_bytes)["paths"]}


def _brief(res):
    return {k: v for k, v in res.items() if k != "records"}


def test_healthy_sweep_owns_every_cus_lds(probe_mod, limit):
    res = probe_mod.lds_sweep(device=0)
    print(_brief(res))
    assert res["ok"] and res["bad"] == [] and res["mismatches"] == 0
    assert res["coverage_complete"], (res["cus_covered"], res["uncovered"])
    assert res["cus_covered"] == res["cu_count"] and res["uncovered"] == 0
    assert res["placement_consistent"]
    assert 1 <= res["launches"] <= 4
    assert res["lds_bytes"] == limit == res["lds_bytes_per_cu"]
    # all five paths, each over what the schedule says it covers: the LDS-DMA
    # reaches every whole KiB, the upper 96 KiB included
    assert list(res["paths"]) == PATHS
    assert res["paths"] == _covered(probe_mod, limit)
    assert res["paths"]["dma"] == limit // 1024 * 1024
    assert res["reps"] == probe_mod.lds_sweep_reference(16)["default_reps"] * \
        2 ** (res["launches"] - 1)
    assert len(res["records"]) == res["cu_count"] * res["launches"]
    assert res["sweep_ms"] > 0
    # one block per CU, its four waves on that CU's four SIMDs
    cus = set()
    for hw_ids, xcc_ids, *_ in res["records"][:res["cu_count"]]:
        where = [probe_mod.decode_hw_id(h, x) for h, x in zip(hw_ids, xcc_ids)]
        assert len({w[:4] for w in where}) == 1
        assert sorted(w[4] for w in where) == [0, 1, 2, 3]
        cus.add(where[0][:4])
    if res["launches"] == 1:
        assert len(cus) == res["cu_count"]


@pytest.mark.parametrize("blocks", [1, 3])
def test_small_shapes_are_clean(probe_mod, limit, blocks):
    for lds_bytes in (16, 2048, 2064, 65536, 67584, limit):
        res = probe_mod.lds_sweep(device=0, lds_bytes=lds_bytes, blocks=blocks,
                                  reps=1)
        assert res["mismatches"] == 0 and res["ok"], (lds_bytes, res["bad"])
        assert res["paths"] == _covered(probe_mod, lds_bytes)
        assert res["lds_bytes"] == lds_bytes and res["launches"] == 1
        assert len(res["records"]) == blocks
        assert res["placement_consistent"]
        # fewer blocks than CUs, or less than a CU's LDS: never complete
        assert not res["coverage_complete"]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("whole", [True, False], ids=["limit", "2064"])
def test_one_flipped_bit_is_one_mismatch(probe_mod, limit, whole, path):
    lds_bytes = limit if whole else 2064
    blocks = 3
    last = _covered(probe_mod, lds_bytes)[path] // 16 - 1
    elements = [0, last] + ([65536 // 16] if whole else [])
    for element in elements:
        for word in (0, 3):
            for bit in (0, 31):
                for block in (0, blocks - 1):
                    corrupt = (block, path, PATTERN[path], AFTER[path], "flip",
                               element, word, bit)
                    res = probe_mod.lds_sweep(
                        device=0, lds_bytes=lds_bytes, blocks=blocks, reps=1,
                        paths=[path], corrupt=corrupt)
                    where = (corrupt, _brief(res))
                    assert not res["ok"], where
                    assert res["mismatches"] == res["launches"] == 1, where
                    assert len(res["bad"]) == 1, where
                    bad = res["bad"][0]
                    want_bits = [0, 0, 0, 0]
                    want_bits[word] = 1 << bit
                    assert list(bad["bad_bits"]) == want_bits, where
                    assert bad["mismatches"] == 1
                    first = bad["first"]
                    assert (first["path"], first["pattern"], first["step"],
                            first["element"], first["word"]) == (
                        path, PATTERN[path], AFTER[path] + 1, element, word), where
                    assert first["got"] ^ first["expected"] == 1 << bit, where
                    rec = res["records"][block]
                    assert rec[2] == 1 and list(rec[3]) == want_bits
                    assert all(r[2] == 0 for i, r in enumerate(res["records"])
                               if i != block)
                    assert (bad["xcc"], bad["se"], bad["sh"], bad["cu"]) == \
                        probe_mod.decode_hw_id(rec[0][0], rec[1][0])[:4]


def test_flip_in_a_full_sweep_is_counted_once_per_launch(probe_mod, limit):
    """Default blocks, paths and reps: the damage is done in the first round
    of each launch only, and a step writes what it expected, not what it
    read, so nothing echoes."""
    last_block = probe_mod.lds_sweep(device=0, lds_bytes=16, blocks=1,
                                     reps=1)["cu_count"] - 1
    res = probe_mod.lds_sweep(
        device=0, corrupt=(last_block, "b128", "checker", 2, "flip",
                           limit // 16 - 1, 1, 17))
    assert res["mismatches"] == res["launches"]
    assert 1 <= len(res["bad"]) <= res["launches"]
    first = res["bad"][0]["first"]
    assert (first["path"], first["pattern"], first["step"], first["element"],
            first["word"]) == ("b128", "checker", 3, limit // 16 - 1, 1)
    assert first["got"] ^ first["expected"] == 1 << 17
    assert res["coverage_complete"]  # the damage does not disturb the coverage


@pytest.mark.parametrize("path", ["b128", "b64", "b32"])
def test_alias_is_counted_per_access(probe_mod, limit, path):
    """Element e := element e + distance after a step: the next step finds it
    in every access in which the two elements' reference bytes differ."""
    blocks, block = 3, 1
    elems = limit // 16
    width = ACCESS_BYTES[path]
    for after, element, distance in ((0, 0, 1), (1, 5, 16), (2, 4096, 4096),
                                     (0, elems - 1, -4096)):
        step = after + 1
        want = probe_mod.hbm_march_reference(
            "address", SEED, step, block * elems + element, 1)
        there = probe_mod.hbm_march_reference(
            "address", SEED, step, block * elems + element + distance, 1)
        count = sum(want[i:i + width] != there[i:i + width]
                    for i in range(0, 16, width))
        assert count >= 1  # address is injective
        res = probe_mod.lds_sweep(
            device=0, blocks=blocks, reps=1, paths=[path], patterns=["address"],
            corrupt=(block, path, "address", after, "alias", element, distance))
        where = (path, after, element, distance, _brief(res))
        assert res["mismatches"] == count and res["launches"] == 1, where
        assert len(res["bad"]) == 1 and res["bad"][0]["first"]["element"] == element, where
        assert res["bad"][0]["first"]["step"] == step, where
        # the documented blind spot: solid holds the same value everywhere
        res = probe_mod.lds_sweep(
            device=0, blocks=blocks, reps=1, paths=[path], patterns=["solid"],
            corrupt=(block, path, "solid", after, "alias", element, distance))
        assert res["mismatches"] == 0 and res["ok"], where


def test_deep_health_probe_with_the_sweep(probe_mod, plain_probe):
    from k8s_device_plugin_amd.native import deep_health_probe

    assert plain_probe["healthy"], plain_probe
    assert "lds_sweep" not in plain_probe
    res = deep_health_probe(device=0, hbm_bytes=1 << 28, lds_sweep=True)
    assert res["healthy"], res["floor_violations"]
    assert res["lds_sweep"]["ok"] and res["lds_sweep"]["coverage_complete"]
    assert res["lds_sweep"]["violations"] == []
    assert "warnings" not in res
    assert set(plain_probe) <= set(res)  # every pre-existing key is there


def test_deep_health_probe_inject_env(probe_mod, plain_probe, monkeypatch):
    from k8s_device_plugin_amd.native import (
        LDS_SWEEP_ENV,
        LDS_SWEEP_INJECT_ENV,
        deep_health_probe,
    )

    monkeypatch.setenv(LDS_SWEEP_ENV, "1")
    monkeypatch.setenv(LDS_SWEEP_INJECT_ENV, "1:7:2:10")
    res = deep_health_probe(device=0, hbm_bytes=1 << 28)
    assert not res["healthy"]
    lines = [v for v in res["floor_violations"] if v.startswith("lds_sweep:")]
    assert len(lines) == 1, lines
    assert "1 bad accesses (path b128 pattern address step 1, element 7, " \
        "bits 0x00000400 in word 2)" in lines[0], lines

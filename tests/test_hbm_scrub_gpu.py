"""The HBM scrub on a real MI355X (pytest -m gpu): the march kernels against
a numpy statement of each pattern, and shown to go red: one flipped bit
after any step of any pattern, in the first element, the last and on a slab
boundary, is counted exactly once and named exactly.

S = 1024 * 256 is the stride of a march launch on its minimum grid.  N_BIG =
4 S + 5 takes 1025 blocks (stride 262400): most threads go four-wide, the
last take the tail.  Split at SLAB_BIG it gives a slab on the minimum grid
with both paths mixed and a shorter last slab on the tail alone.  The
largest fast case moves about 400 MB; the one beyond-cache run 18 GiB.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S = 1024 * 256
POISON = 0xA5
GUARD = 4096
SEED = 0xC0FFEE1234
PATTERNS = ["address", "solid", "checker", "random"]
N_BIG = 4 * S + 5
SLAB_BIG = 800000       # elements: 3 S < SLAB_BIG < 4 S, and N_BIG = 1.3 slabs
GAMMA = np.uint64(0x9E3779B97F4A7C15)


@pytest.fixture(scope="module")
def probe_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from k8s_device_plugin_amd.native import load_healthprobe

    return load_healthprobe(required=True)


def _mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def numpy_pattern(pattern, seed, start, count):
    """[count][4] uint32, stated here and not taken from the module:
    address {lo32(i), hi32(i), ~lo32(i), mix32(i)}, solid 0, checker
    0x55555555, random outputs 2i and 2i + 1 of splitmix64 from seed."""
    i = np.uint64(start) + np.arange(count, dtype=np.uint64)
    lo32 = np.uint64(0xFFFFFFFF)
    if pattern == "address":
        lo = i & lo32
        words = [lo, i >> np.uint64(32), ~lo & lo32,
                 _mix64(i + GAMMA) >> np.uint64(32)]
    elif pattern == "solid":
        words = [np.zeros(count, dtype=np.uint64)] * 4
    elif pattern == "checker":
        words = [np.full(count, 0x55555555, dtype=np.uint64)] * 4
    else:
        s = np.uint64(seed) + (np.uint64(2) * i + np.uint64(1)) * GAMMA
        a, b = _mix64(s), _mix64(s + GAMMA)
        words = [a & lo32, a >> np.uint64(32), b & lo32, b >> np.uint64(32)]
    return np.stack(words, axis=1).astype(np.uint32)


@pytest.fixture(scope="module")
def final_words():
    """Per pattern the [N_BIG][4] state that a clean march leaves: p.
    Read-only."""
    out = {}
    for p in PATTERNS:
        w = numpy_pattern(p, SEED, 0, N_BIG)
        w.setflags(write=False)
        out[p] = w
    return out


def _slab_sizes(n, slab_elems):
    sizes = [slab_elems] * (n // slab_elems)
    if n % slab_elems:
        sizes.append(n % slab_elems)
    return sizes


def _elements(res, n, slab_elems):
    """The n elements as [n][4] uint32, after checking every guard band."""
    sizes = _slab_sizes(n, slab_elems)
    assert res["slabs"] == len(sizes) == len(res["data"])
    parts = []
    for raw, size in zip(res["data"], sizes):
        raw = np.frombuffer(raw, dtype=np.uint8)
        assert raw.size == (GUARD + size + GUARD) * 16
        lo, mid, hi = np.split(raw, [GUARD * 16, (GUARD + size) * 16])
        assert (lo == POISON).all() and (hi == POISON).all()
        parts.append(mid.view(np.uint32).reshape(size, 4))
    return np.concatenate(parts)


def _assert_clean(res, n):
    assert res["mismatches"] == 0 and res["first_bad"] == -1
    assert res["guard_ok"] and res["ok"]
    assert res["records"] == [] and res["bad_ranges"] == []
    assert tuple(res["bad_bits"]) == (0, 0, 0, 0)
    assert res["bytes_tested"] == res["bytes_requested"] == 16 * n


# ---------------- clean ----------------


@pytest.mark.parametrize("n,slab_elems", [
    (1, 1 << 28),
    (1023, 1 << 28), (1023, 400),
    (1024, 1 << 28), (1024, 1000),
    (1025, 1 << 28), (1025, 1024),       # a last slab of one element
    (N_BIG, 1 << 28), (N_BIG, SLAB_BIG),
])
@pytest.mark.parametrize("last", ["random", "address"])
def test_clean_scrub_leaves_the_last_pattern(probe_mod, final_words, n,
                                             slab_elems, last):
    patterns = [p for p in PATTERNS if p != last] + [last]
    res = probe_mod.hbm_scrub(device=0, bytes=16 * n, slab_bytes=16 * slab_elems,
                              guard=GUARD, patterns=patterns, seed=SEED,
                              return_data=True)
    _assert_clean(res, n)
    assert res["patterns"] == patterns and res["poison_byte"] == POISON
    assert not res["beyond_cache"]
    got = _elements(res, n, slab_elems)
    want = final_words[last][:n]
    assert np.array_equal(got, want), (
        "first wrong element %d" % np.flatnonzero((got != want).any(axis=1))[0])
    # 6 n elements moved per pattern: 1 written, 2 * 2 read and written, 1 read
    steps = res["steps"]
    assert steps["march_write"]["bytes"] == 4 * 16 * n
    assert steps["march_rw"]["bytes"] == 4 * 4 * 16 * n
    assert steps["march_read"]["bytes"] == 4 * 16 * n


@pytest.mark.parametrize("pattern", PATTERNS)
def test_one_pattern_alone_is_clean_and_left_behind(probe_mod, final_words,
                                                    pattern):
    res = probe_mod.hbm_scrub(device=0, bytes=16 * N_BIG,
                              slab_bytes=16 * SLAB_BIG, guard=GUARD,
                              patterns=[pattern], seed=SEED, return_data=True)
    _assert_clean(res, N_BIG)
    assert np.array_equal(_elements(res, N_BIG, SLAB_BIG), final_words[pattern])


# ---------------- flip ----------------

# the first element; the last (tail path, last slab); both sides of the slab
# boundary
FLIP_ELEMENTS = [0, N_BIG - 1, SLAB_BIG - 1, SLAB_BIG]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("after_step", [0, 1, 2])
def test_one_flipped_bit_is_counted_once_and_named(probe_mod, final_words,
                                                   pattern, after_step):
    for k, element in enumerate(FLIP_ELEMENTS):
        word = (k + after_step) % 4
        bit = (7 * k + 11 * after_step + 31 * PATTERNS.index(pattern)) % 32
        res = probe_mod.hbm_scrub(
            device=0, bytes=16 * N_BIG, slab_bytes=16 * SLAB_BIG, guard=GUARD,
            seed=SEED, corrupt=(pattern, after_step, "flip", element, word, bit),
            return_data=True)
        where = (pattern, after_step, element, word, bit)
        assert res["mismatches"] == 1 and res["first_bad"] == element, where
        assert not res["ok"] and res["guard_ok"], where
        # every other step and pattern is clean: this is the only record
        assert len(res["records"]) == 1, where
        r = res["records"][0]
        assert (r["pattern"], r["step"], r["index"], r["word"]) == (
            pattern, after_step + 1, element, word), where
        assert r["got"] ^ r["expected"] == 1 << bit, where
        p_word = int(final_words[pattern][element, word])
        want = p_word ^ 0xFFFFFFFF if after_step == 1 else p_word
        assert r["expected"] == want, where
        bits = [0, 0, 0, 0]
        bits[word] = 1 << bit
        assert list(res["bad_bits"]) == bits, where
        # the 2 MiB range of that element, in its slab
        assert len(res["bad_ranges"]) == 1, where
        rng = res["bad_ranges"][0]
        start = 16 * element // (2 << 20) * (2 << 20)
        assert rng["start"] == start, where
        assert rng["end"] == min(start + (2 << 20), 16 * N_BIG) - 1, where
        assert rng["mismatches"] == 1 and rng["first"] == r, where
        assert rng["slab"] == start // 16 // SLAB_BIG, where
        # the step that saw it wrote the complement of what it EXPECTED: the
        # march ends on the last pattern as if nothing had happened.  Only
        # step 3 writes nothing: what it sees in the last pattern stays.
        final = final_words[PATTERNS[-1]]
        if pattern == PATTERNS[-1] and after_step == 2:
            final = final.copy()
            final[element, word] ^= np.uint32(1 << bit)
        assert np.array_equal(_elements(res, N_BIG, SLAB_BIG), final), where


# ---------------- alias ----------------


@pytest.mark.parametrize("distance", [1, S, 262400, -4097])
@pytest.mark.parametrize("after_step", [0, 2])
def test_alias_is_what_the_address_dependent_patterns_are_for(
        probe_mod, distance, after_step):
    """Element j overwritten with element j + distance, by one 16-byte
    hipMemcpy: at the launch's own stride, at one element, across the slab
    boundary.  address and random see exactly that element; solid and
    checker hold the same value everywhere and cannot."""
    j = SLAB_BIG + 1000 if distance < 0 else 12345
    for pattern in PATTERNS:
        res = probe_mod.hbm_scrub(
            device=0, bytes=16 * N_BIG, slab_bytes=16 * SLAB_BIG, guard=GUARD,
            patterns=[pattern], seed=SEED,
            corrupt=(pattern, after_step, "alias", j, distance))
        if pattern in ("address", "random"):
            assert res["mismatches"] == 1 and res["first_bad"] == j, pattern
            assert [(r["pattern"], r["step"], r["index"])
                    for r in res["records"]] == [(pattern, after_step + 1, j)]
        else:
            _assert_clean(res, N_BIG)


# ---------------- the record bound ----------------


def test_mismatches_count_beyond_the_record_bound(probe_mod):
    flips = [("solid", 0, "flip", 5, 0, 3), ("solid", 0, "flip", S + 9, 3, 30),
             ("random", 2, "flip", N_BIG - 2, 1, 0)]
    res = probe_mod.hbm_scrub(device=0, bytes=16 * N_BIG,
                              slab_bytes=16 * SLAB_BIG, guard=GUARD, seed=SEED,
                              corrupt=flips, max_records=1)
    assert res["mismatches"] == 3 and res["first_bad"] == 5
    assert len(res["records"]) == 1
    assert res["records"][0]["index"] in (5, S + 9)   # solid runs before random
    assert list(res["bad_bits"]) == [1 << 3, 1 << 0, 0, 1 << 30]
    assert [r["mismatches"] for r in res["bad_ranges"]] == [1, 1, 1]
    # the same with room for all of them
    res = probe_mod.hbm_scrub(device=0, bytes=16 * N_BIG,
                              slab_bytes=16 * SLAB_BIG, guard=GUARD, seed=SEED,
                              corrupt=flips, max_records=2)
    assert res["mismatches"] == 3 and len(res["records"]) == 2


# ---------------- beyond the cache ----------------


def test_scrub_beyond_the_infinity_cache(probe_mod):
    res = probe_mod.hbm_scrub(device=0, bytes=768 << 20, slab_bytes=256 << 20)
    for step in ("march_write", "march_rw", "march_read"):
        print(step, "%.0f GB/s" % res["steps"][step]["gbps"])
    print("scrub_ms %.2f wall_ms %.2f" % (res["scrub_ms"], res["wall_ms"]))
    assert res["beyond_cache"] is True and res["slabs"] == 3
    assert res["ok"] and res["mismatches"] == 0 and res["guard_ok"]
    assert res["bytes_tested"] == 768 << 20
    assert res["scrub_ms"] > 0


# ---------------- through the policy ----------------


def test_deep_health_probe_with_the_scrub(probe_mod, monkeypatch):
    from k8s_device_plugin_amd import native

    monkeypatch.delenv(native.HBM_SCRUB_ENV, raising=False)
    monkeypatch.delenv(native.CU_SWEEP_ENV, raising=False)
    plain = native.deep_health_probe(hbm_bytes=1 << 28)
    assert "hbm_scrub" not in plain
    res = native.deep_health_probe(hbm_bytes=1 << 28, hbm_scrub_bytes=1 << 26)
    assert res["healthy"], res["floor_violations"]
    assert set(res) == set(plain) | {"hbm_scrub"}
    scrub = res["hbm_scrub"]
    assert scrub["healthy"] and scrub["violations"] == []
    assert scrub["bytes_tested"] == 1 << 26 and scrub["mismatches"] == 0


def test_policy_names_a_flipped_bit(probe_mod, tmp_path):
    """The violation line of the policy from a real, corrupted scrub."""
    from k8s_device_plugin_amd import native

    class Corrupting:
        mem_info = staticmethod(probe_mod.mem_info)
        pci_bus_ids = staticmethod(probe_mod.pci_bus_ids)

        @staticmethod
        def hbm_scrub(device=0, bytes=0):
            return probe_mod.hbm_scrub(
                device=device, bytes=bytes,
                corrupt=("checker", 0, "flip", (0x4200000 >> 4) + 3, 2, 10))

    res = native.hbm_scrub(bytes=1 << 27, sysroot=str(tmp_path),
                           mod=Corrupting)
    assert res["healthy"] is False
    assert res["violations"] == [
        "hbm_scrub: 1 bad elements in bytes 0x4200000-0x43fffff "
        "(pattern checker step 1, bits 0x00000400 in word 2)"]

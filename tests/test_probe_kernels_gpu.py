"""The deep probe's default HBM, LDS and peak-MFMA kernels on a real MI355X
(pytest -m gpu), each against a reference stated here in numpy and each
shown to go red: a wrong element, a wrong LDS word and a wrong accumulator
are all visible.

S = 1024 * 256 is the stride of the one-shot copy on its minimum grid; the
sizes sit on both sides of every point where hbm_copy_kernel changes path.
The largest case moves about 25 MB.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S = 1024 * 256
POISON = 0xA5
GUARD = 4096  # float4s on each side of dst


@pytest.fixture(scope="module")
def probe_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from k8s_device_plugin_amd.native import load_healthprobe

    return load_healthprobe(required=True)


# ---------------- HBM copy ----------------

N_MAX = 4 * 256 * 1500


@pytest.fixture(scope="module")
def pattern_words():
    """[N_MAX][4] uint32: the encodings of the fill pattern, stated here and
    not taken from the module.  Element i is (i & 0xFFFF, (i >> 16) & 0xFFFF,
    (i >> 32) & 0xFFFF, (i & 0xFFFF) + 0.5) as float32.  Read-only."""
    i = np.arange(N_MAX, dtype=np.uint64)
    x = (i & 0xFFFF).astype(np.float32)
    y = ((i >> 16) & 0xFFFF).astype(np.float32)
    z = ((i >> 32) & 0xFFFF).astype(np.float32)
    w = x + np.float32(0.5)
    words = np.stack([x, y, z, w], axis=1).view(np.uint32)
    words.setflags(write=False)
    return words


def _split(res, n):
    """(guard before, the n elements as [n][4] uint32, guard after)."""
    raw = np.frombuffer(res["data"], dtype=np.uint8)
    assert raw.size == (GUARD + n + GUARD) * 16
    lo, mid, hi = np.split(raw, [GUARD * 16, (GUARD + n) * 16])
    return lo, mid.view(np.uint32).reshape(n, 4), hi


def _check_clean_copy(probe_mod, pattern_words, n, blocks, threads=256):
    res = probe_mod.hbm_copy_check(device=0, n=n, blocks=blocks,
                                   threads=threads, guard=GUARD,
                                   return_data=True)
    grid_blocks = blocks or max(1024, -(-n // (threads * 4)))
    stride = grid_blocks * threads
    assert res["blocks"] == grid_blocks and res["stride"] == stride
    # the kernel's own condition, thread by thread
    wide = int(np.count_nonzero(np.arange(stride) + 3 * stride < n))
    assert res["wide_threads"] == wide
    assert res["tail_threads"] == stride - wide
    assert res["poison_byte"] == POISON

    lo, got, hi = _split(res, n)
    assert np.array_equal(got, pattern_words[:n]), (
        "first wrong element %d" %
        np.flatnonzero((got != pattern_words[:n]).any(axis=1))[0])
    assert (lo == POISON).all() and (hi == POISON).all()
    assert res["guard_ok"]
    assert res["mismatches"] == 0 and res["first_bad"] == -1
    return res


@pytest.mark.parametrize("n,wide", [
    (1, 0),                     # one element, tail path
    (255, 0), (256, 0), (257, 0),   # block boundary
    (S - 1, 0), (S, 0), (S + 1, 0),  # tail loop of one against two trips
    (3 * S, 0),                 # no thread 4-wide
    (3 * S + 1, 1),             # exactly thread 0 4-wide
    (3 * S + 5, 5),             # a few threads 4-wide
    (4 * S - 1, S - 1),         # all but the last thread 4-wide
    (4 * S, S),                 # exact fit
    (4 * S + 1, 261377),        # 1025 blocks, stride 262400, both paths mixed
    (4 * 256 * 1500, 256 * 1500),   # exact fit on a non-minimum grid
])
def test_copy_default_grid_is_the_pattern_bit_for_bit(probe_mod, pattern_words,
                                                      n, wide):
    res = _check_clean_copy(probe_mod, pattern_words, n, blocks=0)
    assert res["wide_threads"] == wide
    if n == 4 * S + 1:
        assert res["blocks"] == 1025 and res["stride"] == 262400


@pytest.mark.parametrize("n,wide", [
    (767, 0), (768, 0), (769, 1), (1023, 255), (1024, 256),
])
def test_copy_one_block_is_the_pattern_bit_for_bit(probe_mod, pattern_words,
                                                   n, wide):
    res = _check_clean_copy(probe_mod, pattern_words, n, blocks=1)
    assert res["stride"] == 256 and res["wide_threads"] == wide


def _numpy_mismatches(res, pattern_words, n):
    lo, got, hi = _split(res, n)
    assert (lo == POISON).all() and (hi == POISON).all() and res["guard_ok"]
    return np.flatnonzero((got != pattern_words[:n]).any(axis=1))


N_SEEN = 4 * S
# not in the head, middle or end windows of 16 that the probe used to sample
J_UNSAMPLED = 12345


@pytest.mark.parametrize("distance", [65536, S])
def test_verifier_sees_an_aliased_element(probe_mod, pattern_words, distance):
    """Element j overwritten with element j + distance: one period of the
    old pattern, and the copy's own stride.  A pattern of period 65536
    makes both invisible."""
    n, j = N_SEEN, J_UNSAMPLED
    assert 16 <= j < n // 2 - 16
    res = probe_mod.hbm_copy_check(device=0, n=n, guard=GUARD,
                                   corrupt=("alias", j, distance),
                                   return_data=True)
    bad = _numpy_mismatches(res, pattern_words, n)
    assert list(bad) == [j]
    assert res["mismatches"] == 1 and res["first_bad"] == j
    assert res["mismatches"] == bad.size


@pytest.mark.parametrize("j,component,bit", [
    (0, 0, 31),               # the sign of a zero: -0.0 == 0.0 as floats
    (0, 3, 0),
    (16, 1, 0),               # first element past the old head window
    (16, 2, 30),
    (N_SEEN // 2 - 17, 2, 1),
    (N_SEEN // 2 - 17, 0, 23),
    (N_SEEN - 17, 3, 22),     # last element before the old end window
    (N_SEEN - 17, 1, 31),
    (N_SEEN - 1, 0, 0),
    (N_SEEN - 1, 3, 31),
])
def test_verifier_sees_one_flipped_bit(probe_mod, pattern_words, j, component,
                                       bit):
    n = N_SEEN
    res = probe_mod.hbm_copy_check(device=0, n=n, guard=GUARD,
                                   corrupt=("flip", j, component, bit),
                                   return_data=True)
    lo, got, hi = _split(res, n)
    assert got[j, component] == pattern_words[j, component] ^ np.uint32(1 << bit)
    bad = _numpy_mismatches(res, pattern_words, n)
    assert list(bad) == [j]
    assert res["mismatches"] == 1 and res["first_bad"] == j
    assert res["mismatches"] == bad.size


def test_deep_health_probe_verifies_the_whole_copy(probe_mod):
    from k8s_device_plugin_amd.native import deep_health_probe

    hbm_bytes = 16 * (4 * S + 7)
    res = deep_health_probe(device=0, hbm_bytes=hbm_bytes)
    assert res["hbm_copy_ok"] and res["healthy"], res
    assert res["hbm_mismatches"] == 0 and res["hbm_first_bad"] == -1
    assert res["hbm_bytes_tested"] == hbm_bytes


# ---------------- LDS ----------------


@pytest.fixture(scope="module")
def lds_limit(probe_mod):
    limit = probe_mod.shared_mem_per_block(0)
    assert limit >= 160 * 1024 and limit % 4 == 0  # gfx950: all of a CU's LDS
    return limit


def _lds_sizes(limit):
    return [4, 4 * 255, 4 * 256, 4 * 257, 65536, 65540, 131072, limit]


@pytest.mark.parametrize("size_index", range(8))
def test_lds_counts_exactly_the_corrupted_word(probe_mod, lds_limit, size_index):
    """Clean: 0.  One wrong word in one block: every thread of that block
    reads it once, so exactly `threads` errors, whichever word, bit or
    block; the other blocks (their pattern includes blockIdx) add none."""
    lds_bytes = _lds_sizes(lds_limit)[size_index]
    words = lds_bytes // 4
    targets = sorted({0, words - 1, words // 2} |
                     {w for w in (16383, 16384) if w < words})
    for threads in (64, 256):
        for blocks in (1, 3):
            where = f"lds_bytes={lds_bytes} threads={threads} blocks={blocks}"
            assert probe_mod.lds_check(device=0, lds_bytes=lds_bytes,
                                       blocks=blocks, threads=threads) == 0, where
            for block in sorted({0, blocks - 1}):
                for word in targets:
                    for mask in (1, 1 << 31):
                        got = probe_mod.lds_check(
                            device=0, lds_bytes=lds_bytes, blocks=blocks,
                            threads=threads, corrupt=(block, word, mask))
                        assert got == threads, (where, block, word, mask)


def test_lds_check_rejects_more_than_the_gpu_has(probe_mod, lds_limit):
    with pytest.raises(ValueError, match="sharedMemPerBlock"):
        probe_mod.lds_check(device=0, lds_bytes=lds_limit + 4)


# ---------------- peak MFMA ----------------


@pytest.fixture(scope="module")
def peak_product():
    """[16 regs][64 lanes] of A @ B for mfma_peak_kernel's operands, through
    the lane maps of v_mfma_f32_32x32x16_bf16: lane l holds A[l & 31][8 (l >>
    5) + r] and B[8 (l >> 5) + r][l & 31], r = 0..7, and result register reg
    of lane l is D[(reg & 3) + 8 (reg >> 2) + 4 (l >> 5)][l & 31] (the map of
    tests/test_cu_sweep.py::_result_row)."""
    a = np.zeros((32, 16), dtype=np.int64)
    b = np.zeros((16, 32), dtype=np.int64)
    for lane in range(64):
        for r in range(8):
            a[lane & 31, 8 * (lane >> 5) + r] = ((lane + r) % 5) - 2
            b[8 * (lane >> 5) + r, lane & 31] = ((3 * lane + r) % 7) - 3
    d = a @ b
    assert np.abs(d).max() == 18 and 8192 * 18 < 1 << 24  # exact in fp32
    frag = np.empty((16, 64), dtype=np.int64)
    for reg in range(16):
        for lane in range(64):
            frag[reg, lane] = d[(reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5),
                                lane & 31]
    frag.setflags(write=False)
    return frag


@pytest.mark.parametrize("iters", [1, 64, 8192])
def test_peak_kernel_accumulates_iters_products(probe_mod, peak_product, iters):
    """The kernel that mfma_tflops times, with its accumulators stored:
    every wave's acc[0] and acc[1] equal iters * (A @ B) bit for bit, so the
    iters * 2 accumulating MFMAs per wave of the TF/s formula did run."""
    blocks = 2
    raw = probe_mod.mfma_peak_check(device=0, iters=iters, blocks=blocks)
    got = np.frombuffer(raw, dtype=np.uint32)
    assert got.size == blocks * 8 * 2 * 16 * 64
    got = got.reshape(blocks, 8, 2, 16, 64)
    want = (iters * peak_product).astype(np.float32).view(np.uint32)
    bad = np.argwhere(got != want[None, None, None])
    assert bad.size == 0, (
        f"{len(bad)} accumulator values differ; first (block, wave, acc, "
        f"reg, lane) = {tuple(bad[0])}: got "
        f"{got[tuple(bad[0])]:#x}, expected {want[bad[0][3], bad[0][4]]:#x}")

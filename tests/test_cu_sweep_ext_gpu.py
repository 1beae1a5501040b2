"""The CU sweep's extra pipe sets on a real MI355X (pytest -m gpu): the
block-scaled fp4 / fp6 pipes with live scales (mx) and bf8, the 32x32
shapes, f64 and f32-input (wide).

mfma_raw runs one wave once on fragments built HERE, with encoders written
from the format definitions: one-hot operands establish the operand and
result maps, a single odd scale establishes which lane's scale applies to
which block, and a decoy byte shows that the byte select is live.  The
sweeps themselves have no shape to shrink: one launch of cu_count blocks.
"""

import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BASE = ["bf16_16", "bf16_32", "f16_16", "fp8_16", "i8_16", "mxfp8_16"]
MX = ["mxfp4_16", "mxfp4_32", "mxfp6_16", "mxbf6_16", "mxfp8xfp4_16"]
WIDE = ["bf8_16", "f16_32", "fp8_32", "i8_32", "f64_16", "f32_16"]
SETS = {"mx": MX, "wide": WIDE}

# format -> (bits, exponent bits, mantissa bits, bias); i8 apart
FORMATS = {
    "fp4": (4, 2, 1, 1), "fp6": (6, 2, 3, 1), "bf6": (6, 3, 2, 3),
    "fp8": (8, 4, 3, 7), "bf8": (8, 5, 2, 15), "bf16": (16, 8, 7, 127),
    "f16": (16, 5, 10, 15), "f32": (32, 8, 23, 127), "f64": (64, 11, 52, 1023),
}
# pipe -> (M, N, K, A format, B format, result)
PIPES = {
    "bf16_16": (16, 16, 32, "bf16", "bf16", "f32"),
    "bf16_32": (32, 32, 16, "bf16", "bf16", "f32"),
    "f16_16": (16, 16, 32, "f16", "f16", "f32"),
    "fp8_16": (16, 16, 32, "fp8", "fp8", "f32"),
    "i8_16": (16, 16, 64, "i8", "i8", "i32"),
    "mxfp8_16": (16, 16, 128, "fp8", "fp8", "f32"),
    "mxfp4_16": (16, 16, 128, "fp4", "fp4", "f32"),
    "mxfp4_32": (32, 32, 64, "fp4", "fp4", "f32"),
    "mxfp6_16": (16, 16, 128, "fp6", "fp6", "f32"),
    "mxbf6_16": (16, 16, 128, "bf6", "bf6", "f32"),
    "mxfp8xfp4_16": (16, 16, 128, "fp8", "fp4", "f32"),
    "bf8_16": (16, 16, 32, "bf8", "bf8", "f32"),
    "f16_32": (32, 32, 16, "f16", "f16", "f32"),
    "fp8_32": (32, 32, 16, "fp8", "fp8", "f32"),
    "i8_32": (32, 32, 32, "i8", "i8", "i32"),
    "f64_16": (16, 16, 4, "f64", "f64", "f64"),
    "f32_16": (16, 16, 4, "f32", "f32", "f32"),
}
SCALED = set(MX)  # mfma_raw takes scales for these; mxfp8_16 has its 127s


def encode(fmt, x):
    """The element code of x, which the format represents exactly."""
    if fmt == "i8":
        assert x == int(x) and -128 <= x <= 127
        return int(x) & 0xFF
    bits, e_bits, m_bits, bias = FORMATS[fmt]
    if x == 0:
        return 0
    sign = 1 if x < 0 else 0
    frac, exp = math.frexp(abs(x))  # abs(x) = frac * 2**exp, 0.5 <= frac < 1
    e = exp - 1 + bias
    if e >= 1:
        mant = (frac * 2 - 1) * (1 << m_bits)
    else:  # subnormal
        mant = abs(x) / 2.0 ** (1 - bias - m_bits)
        e = 0
    assert mant == int(mant) and e < (1 << e_bits), (fmt, x)
    return sign << (bits - 1) | e << m_bits | int(mant)


def pack(fmt, values):
    """values [64][J] -> the lanes' fragments: element j is bits
    [j * bits, (j + 1) * bits) of the lane's little-endian bit string."""
    bits = 8 if fmt == "i8" else FORMATS[fmt][0]
    out = bytearray()
    for lane in values:
        word = 0
        for j, x in enumerate(lane):
            word |= encode(fmt, x) << (j * bits)
        out += word.to_bytes(len(lane) * bits // 8, "little")
    return bytes(out)


def k_of(pipe, fmt, group, j):
    """The slot rule: element j of lane group `group` is slot group * J + j.
    One exception: the 8-bit side of the scaled fp8 x fp4 pipe holds
    k = 16 group + j (j < 16) and 64 + 16 group + (j - 16), its 4-bit side
    k = 32 group + j, and they meet by k."""
    m, _, k, fa, fb, _ = PIPES[pipe]
    if pipe in SCALED and fa != fb and FORMATS[fmt][0] == 8:
        return 16 * group + j if j < 16 else 64 + 16 * group + (j - 16)
    return group * (k // (64 // m)) + j


def fragments(pipe, a, b):
    """Lane l holds row / column l % M and the slots k_of(l // M, j) of
    A [M][K] and B [K][N]."""
    m, n, k, fa, fb, _ = PIPES[pipe]
    j_per_lane = k // (64 // m)
    a_vals = [[a[lane % m][k_of(pipe, fa, lane // m, j)] for j in range(j_per_lane)]
              for lane in range(64)]
    b_vals = [[b[k_of(pipe, fb, lane // m, j)][lane % n] for j in range(j_per_lane)]
              for lane in range(64)]
    return pack(fa, a_vals), pack(fb, b_vals)


def result_matrix(pipe, raw):
    """The raw result registers -> D [M][N] through the C/D lane maps."""
    m, n, _, _, _, result = PIPES[pipe]
    dtype = {"f32": np.float32, "i32": np.int32, "f64": np.float64}[result]
    per_lane = np.frombuffer(raw, dtype=np.uint32).reshape(64, -1).copy().view(dtype)
    assert per_lane.shape == (64, m * n // 64)
    d = np.full((m, n), np.nan)
    for lane in range(64):
        for r in range(per_lane.shape[1]):
            if result == "f64":
                row = (lane >> 4) + 4 * r
            elif m == 16:
                row = 4 * (lane >> 4) + r
            else:
                row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
            assert np.isnan(d[row, lane % n])  # the map covers D once
            d[row, lane % n] = per_lane[lane, r]
    return d


def scale_words(true, others=127, byte=0):
    """64 scale words: `true` [64] in byte `byte`, `others` elsewhere."""
    words = np.empty(64, dtype=np.uint32)
    for lane in range(64):
        w = 0
        for k in range(4):
            w |= int(true[lane] if k == byte else others) << (8 * k)
        words[lane] = w
    return words.tobytes()


@pytest.fixture(scope="module")
def probe_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from k8s_device_plugin_amd.native import load_healthprobe

    return load_healthprobe(required=True)


@pytest.fixture(scope="module")
def plain_probe(probe_mod):
    import os

    from k8s_device_plugin_amd import native

    for env in (native.CU_SWEEP_ENV, native.CU_SWEEP_INJECT_ENV,
                native.CU_SWEEP_EXTRA_ENV):
        assert env not in os.environ
    return native.deep_health_probe(device=0, hbm_bytes=1 << 28)


def distinct_rows_b(k, n):
    """B [K][N] of small integers that every format holds, rows pairwise
    distinct and columns pairwise distinct."""
    rng = np.random.RandomState(20240607)
    b = rng.choice([-4, -3, -2, -1, 1, 2, 3, 4], size=(k, n))
    assert len({tuple(r) for r in b}) == k and len({tuple(c) for c in b.T}) == n
    return b


# ---------------- mfma_raw: maps, scale ownership, byte select ----------------


@pytest.mark.parametrize("corner", ["first", "last", "middle"])
@pytest.mark.parametrize("pipe", BASE + MX + WIDE)
def test_one_hot_a_selects_one_row_of_b(probe_mod, pipe, corner):
    """A lone A element at (row, slot) against a B with distinct rows gives
    a * B[slot] in row `row` of D and zero elsewhere, times the scales of
    the two blocks that hold the slot (mx): those of lane group slot // 32.
    The middle slot is one where the halves of an 8-bit scaled operand and
    its blocks part ways (k = 71: lane group 0, block 2)."""
    m, n, k, _, _, _ = PIPES[pipe]
    row, slot = {"first": (0, 0), "last": (m - 1, k - 1),
                 "middle": (m // 2 + 1, k * 5 // 9)}[corner]
    a = np.zeros((m, k))
    a[row, slot] = 2.0
    b = distinct_rows_b(k, n)
    a_frag, b_frag = fragments(pipe, a, b)
    kwargs, factor = {}, np.ones(n)
    if pipe in SCALED:
        # every lane its own scale, 1/2 .. 4 on A and 1/4 .. 2 on B
        sa = np.array([126 + lane % 4 for lane in range(64)])
        sb = np.array([125 + (lane * 7 + lane // 16) % 4 for lane in range(64)])
        kwargs = {"scale_a": scale_words(sa), "scale_b": scale_words(sb)}
        group = slot // 32  # the block's scales sit in this lane group
        factor = np.array([2.0 ** (int(sa[group * m + row]) - 127 +
                                   int(sb[group * m + col]) - 127)
                           for col in range(n)])
    d = result_matrix(pipe, probe_mod.mfma_raw(0, pipe, a_frag, b_frag, **kwargs))
    want = np.zeros((m, n))
    want[row] = 2.0 * b[slot] * factor
    assert np.array_equal(d, want), (pipe, corner, d)


@pytest.mark.parametrize("pipe", MX)
def test_scale_belongs_to_the_lane_that_holds_the_block(probe_mod, pipe):
    """All ones, all scales 1 except one lane's on each side: only the 32
    elements of that lane's block are scaled (with all ones the test cannot
    tell which lane holds them; the middle one-hot case does)."""
    m, n, k, _, _, _ = PIPES[pipe]
    a_frag, b_frag = fragments(pipe, np.ones((m, k)), np.ones((k, n)))
    sa = np.full(64, 127)
    sb = np.full(64, 127)
    lane_a, lane_b = 37, 22
    sa[lane_a] = 130  # x 8
    sb[lane_b] = 125  # / 4
    raw = probe_mod.mfma_raw(0, pipe, a_frag, b_frag, scale_a=scale_words(sa),
                             scale_b=scale_words(sb))
    want = np.zeros((m, n))
    for i in range(m):
        for j in range(n):
            for g in range(64 // m):
                want[i, j] += 32 * 2.0 ** (int(sa[g * m + i]) + int(sb[g * m + j]) - 254)
    d = result_matrix(pipe, raw)
    assert np.array_equal(d, want), (pipe, d)
    assert len(np.unique(want)) == 4  # plain, A's, B's, both


@pytest.mark.parametrize("pipe", MX)
def test_byte_select_is_live(probe_mod, pipe):
    """The same operands with the decoy byte selected on purpose: off by the
    decoy's factor, on each side."""
    m, n, k, _, _, _ = PIPES[pipe]
    a = np.zeros((m, k))
    a[3, 40] = 1.0
    a_frag, b_frag = fragments(pipe, a, distinct_rows_b(k, n))
    truth = np.full(64, 127)
    # byte 0 true; byte 2 of A holds 127 + 8, byte 3 of B 127 - 9
    sa = np.frombuffer(scale_words(truth), dtype=np.uint32) + (8 << 16)
    sb = np.frombuffer(scale_words(truth), dtype=np.uint32) - (9 << 24)
    run = lambda sel: result_matrix(pipe, probe_mod.mfma_raw(
        0, pipe, a_frag, b_frag, scale_a=sa.tobytes(), scale_b=sb.tobytes(),
        sel=sel))
    plain = run((0, 0))
    assert np.count_nonzero(plain) == n
    assert np.array_equal(run((2, 0)), plain * 2.0 ** 8)
    assert np.array_equal(run((0, 3)), plain * 2.0 ** -9)
    assert np.array_equal(run((2, 3)), plain * 2.0 ** -1)
    assert np.array_equal(run((1, 1)), plain)


# ---------------- the sweeps ----------------


@pytest.mark.parametrize("pipe_set", ["mx", "wide"])
def test_healthy_sweep_covers_every_simd(probe_mod, plain_probe, pipe_set):
    cu_count = plain_probe["cu_count"]
    res = probe_mod.cu_sweep(device=0, pipe_set=pipe_set)
    print({k: v for k, v in res.items() if k not in ("records", "bad")})
    assert res["ok"] and res["bad"] == [], (len(res["bad"]), res["bad"][:2])
    assert res["coverage_complete"], (
        res["cus_covered"], res["simds_covered"], res["uncovered"])
    assert res["cu_count"] == cu_count
    assert res["cus_covered"] == cu_count
    assert res["simds_covered"] == 4 * cu_count
    assert res["pipe_set"] == pipe_set
    assert res["pipes"] == SETS[pipe_set]
    assert len(res["records"]) == res["waves_checked"]
    assert all(r[2] == 0 for r in res["records"])
    assert res["sweep_ms"] > 0


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("pipe_set", ["mx", "wide"])
def test_injected_bad_pipe_is_found_and_named(probe_mod, plain_probe,
                                              pipe_set, where):
    cu_count = plain_probe["cu_count"]
    names = SETS[pipe_set]
    block, wave, pipe = ((0, 0, 0) if where == "first"
                         else (cu_count - 1, 3, len(names) - 1))
    res = probe_mod.cu_sweep(device=0, inject=(block, wave, pipe),
                             pipe_set=pipe_set)
    assert not res["ok"]
    assert len(res["bad"]) == 1, res["bad"]
    bad = res["bad"][0]
    assert bad["pipes"] == [names[pipe]]
    rec = res["records"][block * 4 + wave]
    assert rec[2] == 1 << pipe
    assert (bad["xcc"], bad["se"], bad["sh"], bad["cu"], bad["simd"]) == \
        probe_mod.decode_hw_id(rec[0], rec[1])
    first = bad["first"]
    assert first["pipe"] == names[pipe]
    # one lane, one flipped bit
    assert bin(first["got"] ^ first["expected"]).count("1") == 1
    assert bad["bad_lanes"] == 1 << first["lane"]
    assert sum(1 for r in res["records"] if r[2]) == res["launches"]
    assert res["coverage_complete"]


def test_base_sweep_is_still_the_six(probe_mod):
    res = probe_mod.cu_sweep(device=0)
    assert res["pipes"] == BASE and res["ok"]


# ---------------- probe level ----------------


def test_deep_health_probe_with_the_extra_sets(probe_mod, plain_probe):
    from k8s_device_plugin_amd.native import deep_health_probe

    assert plain_probe["healthy"], plain_probe
    assert "cu_sweep_extra" not in plain_probe
    base_only = deep_health_probe(device=0, hbm_bytes=1 << 28, cu_sweep=True)
    assert "cu_sweep_extra" not in base_only
    res = deep_health_probe(device=0, hbm_bytes=1 << 28, cu_sweep=True,
                            cu_sweep_extra="all")
    assert res["healthy"], res["floor_violations"]
    assert "warnings" not in res
    assert set(plain_probe) <= set(res)
    assert res["cu_sweep"]["pipes"] == BASE
    assert list(res["cu_sweep_extra"]) == ["mx", "wide"]
    for pipe_set, sweep in res["cu_sweep_extra"].items():
        assert sweep["ok"] and sweep["coverage_complete"]
        assert sweep["pipes"] == SETS[pipe_set]


def test_deep_health_probe_inject_by_name(probe_mod, plain_probe, monkeypatch):
    from k8s_device_plugin_amd import native

    monkeypatch.setenv(native.CU_SWEEP_INJECT_ENV, "1:1:mxfp4_16")
    res = native.deep_health_probe(device=0, hbm_bytes=1 << 28, cu_sweep=True,
                                   cu_sweep_extra="all")
    assert not res["healthy"]
    lines = [v for v in res["floor_violations"] if v.startswith("cu_sweep:")]
    assert len(lines) == 1 and lines[0].endswith("failed mxfp4_16"), lines
    assert res["cu_sweep"]["ok"] and res["cu_sweep_extra"]["wide"]["ok"]

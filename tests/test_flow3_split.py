"""GPU parity of option f3split: one pair on flow3's staged two-column linear-gap
kernel cut at a column, the left half scored forward and the right half on both sequences mirrored in the
same launch, joined by sw_flow3_combine_kernel.  Bit-exact against the oracle.

Covered with f3split = 1 (cut whenever each half gets two strips, n >= 379): widths on both sides of that
bound and of a strip (253, 378 stay whole; 379, 504, 505, 1000, 2521 are cut, with lead pads of 125, 0,
125, 8 and 125 columns), rows 1 (no crossing term), 2, 17 and around a wave and a chunk (63, 64, 65, 300;
row counts off a multiple of 4 take the byte-wise mirrored staging, the others the 16-byte one); random
pairs, 5 %-mutated copies (the crossing term decides), pairs whose best alignment lies wholly in one half;
three linear-gap constant sets; grids of 1, 2 and 3 workgroups; a seven-letter pair; launches back to back
on the same buffers; and the automatic plan's choice (variant bit 17 of sw_last_stats)."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PARAMS = [(1, -1, 1, 1), (2, -3, 2, 2), (3, -1, 4, 4)]
NS = [253, 378, 379, 504, 505, 1000, 2521]
MS = [1, 2, 17, 63, 64, 65, 300]
ACGT = np.frombuffer(b"ACGT", np.uint8)
CUT = 1 << 17
AUTO_N = 4096   # the automatic plan cuts pairs this wide or wider (sw_engine.hip F3_SPLIT_AUTO_N)


@pytest.fixture(autouse=True)
def _defaults(engine, request):
    def reset():
        engine.set_option("f3split", -1)
        engine.set_option("blocks", 0)
        engine.set_option("orient", 0)
        engine.set_option("linear", -1)
        engine.set_option("trace", 0)
    request.addfinalizer(reset)
    engine.set_option("orient", 1)   # seq1 across the lanes: n is its length


def _mutated(rng, alpha, a, m, lo):
    """m symbols of a from lo on (wrapped), 5 % replaced and one short insertion"""
    b = np.resize(a[lo:], m).copy() if lo + m > len(a) else a[lo:lo + m].copy()
    mut = rng.random(m) < 0.05
    b[mut] = alpha[rng.integers(0, len(alpha), int(mut.sum()))]
    if m > 20:
        k = int(rng.integers(5, m - 5))
        b = np.concatenate([b[:k], alpha[rng.integers(0, len(alpha), 2)], b[k:]])[:m]
    return np.ascontiguousarray(b)


def _cut_of(engine, n):
    plan = engine.split_bounds(n)
    return None if plan is None else plan[0]


def _check(engine, oracle_mod, a, b, prm_t, tag):
    exp = oracle_mod.score_linear(a, b, oracle_mod.Params(*prm_t))
    got = engine.score(a, b, engine.Params(*prm_t))
    st = engine.last_stats()
    assert got == exp, (tag, got, exp, st)
    return st


@pytest.mark.parametrize("prm_t", PARAMS)
def test_shapes_against_oracle(engine, oracle_mod, prm_t):
    """Every (n, m) of the grid, a random pair and a mutated copy laid across the cut: the oracle's score,
    on the cut path exactly when each half has two strips."""
    engine.set_option("f3split", 1)
    rng = np.random.default_rng(zlib.crc32(repr(prm_t).encode()))
    crossing = 0
    for n in NS:
        c = _cut_of(engine, n)
        assert (c is not None) == (n >= 379), (n, c)
        for m in MS:
            a = ACGT[rng.integers(0, 4, n)]
            pairs = [("random", a, ACGT[rng.integers(0, 4, m)])]
            # the copied window straddles the cut (or the middle of an uncut pair)
            lo = max(0, min(n - m, (c if c is not None else n // 2) - m // 2))
            pairs.append(("mutated", a, _mutated(rng, ACGT, a, m, lo)))
            for kind, x, y in pairs:
                st = _check(engine, oracle_mod, x, y, prm_t, (kind, n, m))
                assert bool(st["variant"] & CUT) == (n >= 379), (kind, n, m, st)
                assert st["variant"] & 64, st   # the flow3 kernel
            if c is not None and m >= 17:
                # the mutated copy's best path crosses the cut: neither half alone reaches the score
                op = oracle_mod.Params(*prm_t)
                y = pairs[1][2]
                whole = oracle_mod.score_linear(a, y, op)
                crossing += whole > max(oracle_mod.score_linear(a[:c], y, op), oracle_mod.score_linear(a[c:], y, op))
    assert crossing >= 15, crossing


def test_one_sided_alignments(engine, oracle_mod):
    """The best alignment wholly left or wholly right of the cut: the halves' own maxima carry the score."""
    engine.set_option("f3split", 1)
    rng = np.random.default_rng(11)
    n, m = 1000, 120
    c = _cut_of(engine, n)
    op = oracle_mod.Params(1, -1, 1, 1)
    for lo in (20, c - m - 30, c + 30, n - m - 5):
        a = ACGT[rng.integers(0, 4, n)]
        b = _mutated(rng, ACGT, a, m, lo)
        st = _check(engine, oracle_mod, a, b, (1, -1, 1, 1), ("one-sided", lo))
        assert st["variant"] & CUT, st
        side = a[:c] if lo < c else a[c:]
        assert oracle_mod.score_linear(side, b, op) == oracle_mod.score_linear(a, b, op), lo


@pytest.mark.parametrize("blocks", [1, 2, 3])
def test_small_grids(engine, oracle_mod, blocks):
    """Fewer workgroups than strip groups (2521 columns: 3 + 3 groups): items are claimed in order, the
    left chain first, so every group's producer has been claimed before it."""
    engine.set_option("f3split", 1)
    engine.set_option("blocks", blocks)
    rng = np.random.default_rng(100 + blocks)
    a = ACGT[rng.integers(0, 4, 2521)]
    for prm_t in PARAMS:
        b = _mutated(rng, ACGT, a, 300, 1100)
        st = _check(engine, oracle_mod, a, b, prm_t, ("grid", blocks, prm_t))
        assert st["variant"] & CUT and st["blocks"] == blocks and st["items"] == 6, st


def test_seven_letter_pair(engine, oracle_mod):
    """A pair over seven byte values on sw_flow3h_kernel, cut (mirrored column words and row symbols)."""
    engine.set_option("f3split", 1)
    alpha = np.frombuffer(b"ACGTNRY", np.uint8)
    rng = np.random.default_rng(7)
    for n, m in ((1000, 300), (505, 65)):
        a = alpha[rng.integers(0, 7, n)]
        b = _mutated(rng, alpha, a, m, _cut_of(engine, n) - m // 2)
        for prm_t in PARAMS:
            st = _check(engine, oracle_mod, a, b, prm_t, ("hep", n, m, prm_t))
            assert st["variant"] & CUT and st["dna"] == 2, st


def test_back_to_back_launches(engine, oracle_mod):
    """Launches of one shape reuse the boundary buffers: the epoch-keyed granules of the last launch
    must not serve the next one (the combine kernel checks every key)."""
    engine.set_option("f3split", 1)
    rng = np.random.default_rng(23)
    n, m = 2521, 300
    a1 = ACGT[rng.integers(0, 4, n)]
    a2 = ACGT[rng.integers(0, 4, n)]
    pairs = [(a1, _mutated(rng, ACGT, a1, m, 1150)), (a2, ACGT[rng.integers(0, 4, m)]),
             (a2, _mutated(rng, ACGT, a2, m, 1200))]
    exp = [oracle_mod.score_linear(x, y) for x, y in pairs]
    assert len(set(exp)) == 3
    for _ in range(2):
        for (x, y), e in zip(pairs, exp):
            assert engine.score(x, y) == e
            assert engine.last_stats()["variant"] & CUT


def test_automatic_choice(engine, oracle_mod):
    """f3split = -1: cut from AUTO_N columns on the staged linear-gap kernel; whole below it, with the
    affine step (other constants, or option linear = 0), and for a traced launch."""
    import torch
    rng = np.random.default_rng(5)
    m = 300
    wide = ACGT[rng.integers(0, 4, AUTO_N)]
    b = _mutated(rng, ACGT, wide, m, AUTO_N // 2 - 100)
    assert engine.get_option("f3split") == -1
    st = _check(engine, oracle_mod, wide, b, (1, -1, 1, 1), "auto wide")
    assert st["variant"] & CUT and st["variant"] & 64, st
    uncut_items = (((AUTO_N - 2 + 125) // 126) + 3) // 4
    assert st["items"] in (uncut_items, uncut_items + 1), st   # both halves' groups
    st = _check(engine, oracle_mod, wide[:AUTO_N - 1], b, (1, -1, 1, 1), "auto below")
    assert not st["variant"] & CUT, st
    st = _check(engine, oracle_mod, wide, b, (2, -3, 5, 2), "auto affine constants")
    assert not st["variant"] & CUT, st
    engine.set_option("linear", 0)
    st = _check(engine, oracle_mod, wide, b, (1, -1, 1, 1), "auto linear = 0")
    assert not st["variant"] & CUT, st
    engine.set_option("linear", -1)
    strips = (AUTO_N - 2 + 125) // 126
    trace = torch.zeros(16 * strips, dtype=torch.int64, device="cuda")
    engine.set_option("trace", trace.data_ptr())
    st = _check(engine, oracle_mod, wide, b, (1, -1, 1, 1), "auto traced")
    engine.set_option("trace", 0)
    torch.cuda.synchronize()
    assert not st["variant"] & CUT and st["items"] == uncut_items, st
    assert int((trace.view(strips, 16)[:, 2] != 0).sum()) == strips   # one chain of all the strips
    engine.set_option("f3split", 0)
    st = _check(engine, oracle_mod, wide, b, (1, -1, 1, 1), "off")
    assert not st["variant"] & CUT, st
    for bad in (-2, 2):
        with pytest.raises(engine.SwError):
            engine.set_option("f3split", bad)

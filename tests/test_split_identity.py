"""CPU check of the identity behind option f3split (one pair cut at a column c and
scored from both ends).  With the linear-gap step (G_INIT == G_EXT) the DP has one value per grid node, so

    score = max( max H over columns [0, c),
                 max H over columns [c, n) taken mirrored against the mirrored rows,
                 max over i of H_L[i][c] + H_R[m - i][n - c] )

where H_L is the forward DP of the left half and H_R the DP of the mirrored right half.  Checked against
oracle.score_full with both halves from oracle.slab (whose edge is H of the slab's last column, rows
1..m): random and similar pairs, a cut in every residue class of n mod 126, three linear-gap constant
sets.  And the engine's planner (sw_split_bounds, no device): the cut it picks for every n in 252..5000.
"""
import zlib

import numpy as np
import pytest

PARAMS = [(1, -1, 1, 1), (2, -3, 2, 2), (3, -1, 4, 4)]
ACGT = np.frombuffer(b"ACGT", np.uint8)


def split_score(oracle_mod, a, b, c, op):
    """The right-hand side of the identity and whether the crossing term decided it."""
    m = len(b)
    best_l, (hl, _) = oracle_mod.slab(a[:c], b, op)
    best_r, (hr, _) = oracle_mod.slab(a[c:][::-1].copy(), b[::-1].copy(), op)
    # node rows i = 1 .. m - 1: H_L[i][c] = hl[i - 1], H_R[m - i][n - c] = hr[m - i - 1]; rows 0 and m
    # add a border zero to a value the other half's maximum already covers
    cross = int((hl[:m - 1].astype(np.int64) + hr[:m - 1][::-1]).max()) if m > 1 else 0
    return max(best_l, best_r, cross), cross > max(best_l, best_r)


def _pairs(rng, n, m):
    a = ACGT[rng.integers(0, 4, n)]
    yield a, ACGT[rng.integers(0, 4, m)]
    # a mutated copy of a window of a: long alignments that cross any cut inside the window
    lo = int(rng.integers(0, max(1, n - m + 1)))
    b = np.resize(a[lo:lo + m], m).copy()
    mut = rng.random(m) < 0.05
    b[mut] = ACGT[rng.integers(0, 4, int(mut.sum()))]
    if m > 20:
        k = int(rng.integers(5, m - 5))
        b = np.concatenate([b[:k], ACGT[rng.integers(0, 4, 3)], b[k:]])[:m]
    yield a, np.ascontiguousarray(b)


@pytest.mark.parametrize("prm_t", PARAMS)
def test_identity_every_residue_class(oracle_mod, prm_t):
    op = oracle_mod.Params(*prm_t)
    rng = np.random.default_rng(zlib.crc32(repr(prm_t).encode()))
    decided = 0
    for res in range(126):
        n = 260 + res + 126 * int(rng.integers(0, 2))   # n mod 126 takes every value
        m = int(rng.choice([1, 2, 17, 64, 150, 300]))
        for a, b in _pairs(rng, n, m):
            exp = oracle_mod.score_full(a, b, op)
            for c in (126, int(rng.integers(1, n)), n - 1):
                got, by_cross = split_score(oracle_mod, a, b, c, op)
                assert got == exp, (prm_t, n, m, c)
                decided += by_cross
    assert decided > 50, decided   # the crossing term is exercised, not only the halves' maxima


def test_identity_similar_pairs(oracle_mod):
    for seed, n in ((1, 700), (2, 1500), (3, 2521)):
        a, b = oracle_mod.similar_pair(seed, n)
        for prm_t in PARAMS:
            op = oracle_mod.Params(*prm_t)
            exp = oracle_mod.score_full(a, b, op)
            for c in (126, 126 * (n // 252), n - 127):
                assert split_score(oracle_mod, a, b, c, op)[0] == exp, (seed, n, prm_t, c)


def test_planner_bounds():
    """sw_split_bounds: cut and padded right half are multiples of 126, the pad is under one strip, each
    half has two strips or more, the strips add up, and exactly the pairs too narrow for that stay uncut."""
    import concurrentproject_amd as sw
    for n in range(252, 5001):
        plan = sw.split_bounds(n)
        if n < 379:   # 252 columns on the left and 127 on the right is the narrowest cut
            assert plan is None, (n, plan)
            continue
        assert plan is not None, n
        c, lead, strips = plan
        assert c % 126 == 0 and (n - c + lead) % 126 == 0 and 0 <= lead < 126, (n, plan)
        left, right = c // 126, (n - c + lead) // 126
        assert left >= 2 and right >= 2 and left + right == strips, (n, plan)
        assert 0 <= right - left <= 1 or left == 2, (n, plan)   # balanced chains
        assert 0 < c < n, (n, plan)
    assert sw.split_bounds(65536) == (32760, 110, 521)   # C2: 260 + 261 strips

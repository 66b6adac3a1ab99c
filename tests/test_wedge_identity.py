"""CPU model of the wedge plan (one long pair scored as two wedges cut along an
anti-diagonal staircase), at the staged linear-gap kernel's lane geometry, against oracle.score_full.

Forward chain F over the padded columns [0, W), W = 126 S + 2: strip s holds columns [126 s, 126 s + 128),
lane l the columns 126 s + 2 l (A) and + 1 (B); at step t lane l is at row t - l; strip s runs
end_s = E0 - 64 s steps and then one step more, so lane l knows H of both its columns at rows
b = end_s - 1 - l and b + 1 (lane 0 of a strip s > 0 at row b only: its inflow of row b + 1 is never
published; lane 63 of strip s - 1 holds the same columns at rows b + 1 and b + 2).  Backward chain B: the same construction on both sequences mirrored, with
lead = W - n dead columns and rlead dead rows in front, so that its strip S - 1 - s lies on F's strip s
(lane 63 - l on lane l, columns A and B swapped) and E0' = m + rlead - 2 - E0 + 64 S, both multiples of 64
(the chunk loop's body is two 32-row chunks).

Node form (tests/test_split_identity.py): node (i, j) is the corner below-right of cell (i - 1, j - 1);
H_F(node) is F's H of that cell, H_B(node) is B's H of the mirrored image of cell (i, j).  Then

    score = max( max H of F's region, max H of B's region, max over shared nodes of H_F + H_B ).

The model runs each chain with every cell outside its region poisoned, so a region that is not closed under
(up, left, up-left) shows as a wrong score, and it asserts the covering condition on the shared nodes: per
column j their rows are one interval [lo_j, hi_j] with hi_{j+1} >= lo_j, so a path that lies in neither
region passes through one of them (assert_covering).
"""
import zlib

import numpy as np
import pytest

PARAMS = [(1, -1, 1, 1), (2, -3, 2, 2), (3, -1, 4, 4)]
ACGT = np.frombuffer(b"ACGT", np.uint8)
POISON = 1 << 20
DEAD = -(1 << 10)


def wedge_plan(n, m):
    """(S, lead, rlead, E0, E0b), or None where a strip would keep less than one 64-row body: the
    arithmetic of the engine's plan_wedge."""
    S = max(2, -(-(n - 2) // 126))
    lead = 126 * S + 2 - n
    if m < 64 * S + 64:
        return None
    rlead = (2 - m) % 64
    T = m + rlead - 2 + 64 * S
    E0 = 64 * (T // 128)
    return S, lead, rlead, E0, T - E0


def region_dp(cols, rows, hi, prm):
    """Linear-gap H of `rows` x `cols` (byte 0: a dead row / column) where column c is computed for rows
    <= hi[c] only; every other cell reads POISON.  Returns H as int64 [len(rows), len(cols)]."""
    ma, mi, G, _ = prm
    W = len(cols)
    H = np.empty((len(rows), W), np.int64)
    prev = np.zeros(W + 1, np.int64)
    ramp = G * np.arange(W + 1, dtype=np.int64)
    for i, ch in enumerate(rows):
        s = np.where((cols == ch) & (ch != 0), ma, mi).astype(np.int64)
        s[(cols == 0) | (ch == 0)] = DEAD
        d = np.maximum(np.maximum(prev[:-1] + s, prev[1:] - G), 0)
        # H[j] = max over k <= j of d[k] - G (j - k): a running maximum of d[k] + G k
        cur = np.maximum.accumulate(np.concatenate(([0], d)) + ramp) - ramp
        cur[1:][i > hi] = POISON
        H[i] = cur[1:]
        prev = cur
    return H


def wedge_model(a, b, prm):
    """(score, whether the crossing term decided it); asserts the covering condition on the way."""
    n, m = len(a), len(b)
    S, lead, rlead, E0, E0b = wedge_plan(n, m)
    W = 126 * S + 2

    def chain(cols, rows, e0):
        hi = np.full(W, -1)
        lanes = []
        for s in range(S):
            for l in range(64):
                last = e0 - 64 * s - 1 - l
                assert 0 <= last and last + 1 < len(rows), (n, m, s, l)
                c = 126 * s + 2 * l
                hi[c:c + 2] = np.maximum(hi[c:c + 2], last + 1)
                lanes.append((s, l, c, last))
        H = region_dp(cols, rows, hi, prm)
        best = int(H[H < POISON // 2].max())
        # lane 0 of a strip with inflow has no second row: the strip on its left ends 64 steps later and its
        # exit flush stops one row short of it (lane 63 of that strip holds the same columns a row further down)
        return best, {(s, l): (c, last, H[last, c], H[last, c + 1]) +
                      ((H[last + 1, c], H[last + 1, c + 1]) if s == 0 or l else (None, None))
                      for s, l, c, last in lanes}

    best_f, f = chain(np.concatenate([a, np.zeros(W - n, np.uint8)]), b, E0)
    best_b, g = chain(np.concatenate([np.zeros(lead, np.uint8), a[::-1]]),
                      np.concatenate([np.zeros(rlead, np.uint8), b[::-1]]), E0b)
    nf, nb = {}, {}
    for (s, l), (c, last, a0, b0, a1, b1) in f.items():
        for node, v in (((last + 1, c + 1), a0), ((last + 1, c + 2), b0), ((last + 2, c + 1), a1),
                        ((last + 2, c + 2), b1)):
            assert v is None or nf.setdefault(node, v) == v   # the duplicated boundary lanes agree
    for (s, l), (p, last, a0, b0, a1, b1) in g.items():
        # mirrored cell (r', p) is the original cell (m - 1 - (r' - rlead), W - 1 - p)
        r, c = m - 1 + rlead - last, W - 1 - p
        for node, v in (((r, c), a0), ((r, c - 1), b0), ((r - 1, c), a1), ((r - 1, c - 1), b1)):
            assert v is None or nb.setdefault(node, v) == v
    shared = set(nf) & set(nb)
    cross = max(int(nf[k] + nb[k]) for k in shared)
    assert max(nf[k] for k in shared) < POISON // 2 and max(nb[k] for k in shared) < POISON // 2
    assert_covering(set(nf), set(nb), n, m)
    return max(best_f, best_b, cross), cross > max(best_f, best_b)


def assert_covering(nf, nb, n, m):
    """A path found by neither chain starts above B's region and ends below F's.  Call a node above
    (below) when its row is less (more) than every shared row of its column; the start is above and the
    end below, since the shared nodes lie in both regions.  The shared rows of column j must be one
    interval [lo_j, hi_j] with hi_{j+1} >= lo_j: then no right or diagonal move leads from above straight
    to below, and a down move cannot, so the first node that is not above is shared.  Node column 0 is F's
    border (H_F = 0): from B's first row there down, B's own maximum covers the path; with no lead pad
    node column n is B's border in the same way."""
    rows = {}
    for i, j in nf & nb:
        rows.setdefault(j, []).append(i)
    lo = {j: min(r) for j, r in rows.items()}
    hi = {j: max(r) for j, r in rows.items()}
    for j, r in rows.items():
        assert sorted(r) == list(range(lo[j], hi[j] + 1)), (n, m, j)
    lo[0] = min(i for i, j in nb if j == 0)
    hi[0] = m
    if n not in rows:
        lo[n], hi[n] = 0, max(i for i, j in nf if j == n)
    for j in range(1, n + 1):
        assert 0 <= lo[j] <= hi[j] <= m and hi[j] >= lo[j - 1], (n, m, j, lo[j - 1], lo[j], hi[j])


def _pairs(rng, n, m):
    a = ACGT[rng.integers(0, 4, n)]
    yield a, ACGT[rng.integers(0, 4, m)]
    # a mutated copy of a, stretched over the rows: its best alignment runs corner to corner, across the staircase
    b = a[np.minimum((np.arange(m) * n) // m, n - 1)].copy()
    mut = rng.random(m) < 0.05
    b[mut] = ACGT[rng.integers(0, 4, int(mut.sum()))]
    k = int(rng.integers(5, m - 5))
    b = np.concatenate([b[:k], ACGT[rng.integers(0, 4, 3)], b[k:]])[:m]
    yield a, np.ascontiguousarray(b)


def _m_choices(S, n):
    lo = 64 * S + 64
    return [lo, lo + 1, lo + 32, lo + 61, max(lo, n), max(lo, n + 37), max(lo, 2 * n - 5)]


@pytest.mark.parametrize("prm_t", PARAMS)
def test_wedge_every_residue_class(oracle_mod, prm_t):
    op = oracle_mod.Params(*prm_t)
    rng = np.random.default_rng(zlib.crc32(repr(prm_t).encode()))
    decided = 0
    for res in range(126):
        n = 253 + res + 126 * int(rng.integers(0, 2))   # n mod 126 takes every value; 2 to 4 strips
        S = wedge_plan(n, 1 << 20)[0]
        ms = _m_choices(S, n)
        m = ms[(res + PARAMS.index(prm_t)) % len(ms)]
        for a, b in _pairs(rng, n, m):
            got, by_cross = wedge_model(a, b, prm_t)
            assert got == oracle_mod.score_full(a, b, op), (prm_t, n, m)
            decided += by_cross
    # of the 252 pairs of a constant set the crossing term decides 247, 227 and 252 (the oracle's scores of these
    # seeded inputs: half the pairs are random, where a short best path straddles the staircase's band often)
    assert decided >= 200, decided


def test_wedge_admission_and_heights(oracle_mod):
    """m from the smallest admissible to 2n, every residue of m mod 64 (every rlead), 2 to 6 strips."""
    prm_t = PARAMS[0]
    op = oracle_mod.Params(*prm_t)
    rng = np.random.default_rng(7)
    for n, ms in ((253, range(192, 192 + 66)), (255, (256, 300)), (379, (320, 321, 383, 500, 758)), (380, (384, 385, 760)),
                  (633, (448, 449, 640, 1266)), (700, (448, 449, 511, 1400))):
        S = wedge_plan(n, 1 << 20)[0]
        for m in ms:
            if m < 64 * S + 64:
                assert wedge_plan(n, m) is None
                continue
            S_, lead, rlead, E0, E0b = wedge_plan(n, m)
            assert 0 <= lead < 126 and 0 <= rlead < 64 and (126 * S + 2) % 126 == 2
            assert E0 % 64 == 0 and E0b % 64 == 0 and min(E0, E0b) >= 64 * S and 0 <= E0b - E0 <= 64
            assert E0 <= m - 1 and E0b <= m + rlead - 1
            for a, b in _pairs(rng, n, m):
                got, _ = wedge_model(a, b, prm_t)
                assert got == oracle_mod.score_full(a, b, op), (n, m)


def test_wedge_similar_pairs(oracle_mod):
    for seed, n in ((1, 700), (2, 1500)):
        a, b = oracle_mod.similar_pair(seed, n)
        for prm_t in PARAMS:
            got, _ = wedge_model(a, b, prm_t)
            assert got == oracle_mod.score_full(a, b, oracle_mod.Params(*prm_t)), (seed, n, prm_t)

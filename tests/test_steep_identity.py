"""CPU model of the steep wedge plan: the two-wedge plan of tests/test_wedge_identity.py
with a staircase that drops more than 64 rows behind some strips, at the staged linear-gap kernel's lane geometry,
against oracle.score_full.

Both chains run S strips, S a multiple of 4, over W = 126 S + 2 padded columns.  The drop behind strip j (how many
steps strip j + 1 ends before strip j) is d[j % 4], a multiple of 64 with d[0] == d[2]; cum[s] is the sum of the
drops behind strips 0 .. s - 1 and D = cum[S - 1].  Forward chain F: strip s runs end_s = e0_F - cum[s] steps and
one more, lane l of it holds H of columns 126 s + 2 l (A) and + 1 (B) at rows end_s - 1 - l and one below (lane 0
of a strip s > 0 the first of them only).  Mirrored chain B: the same on both sequences mirrored, W - 2 - n dead
columns and rlead = (3 - m) mod 64 dead rows in front, e0_F + e0_B = m + rlead + 61 + D; its cell (r', q) is the
node (m - 1 + rlead - r', W - 3 - q) of F's grid (node (i, j): the corner below-right of cell (i - 1, j - 1)).
The mirrored chain's drops are F's read from the far end, the same pattern again.

What strip s hands to strip s + 1 is the column left of the two that lane 63 and the next strip's lane 0 share:
lane 62's column B, 126 s + 125, node column 126 s + 126.  The two dead columns less than the uniform plan's put
B's hand-off column of strip S - 2 - s onto the same node column, and the staircase runs down it from the node of
the right strip's lane 0 to those of the left strip's lane 62.  A chain has H along it from the rows the strip
published (rows <= end_s - 65; the last drop - 63 of them are used), the row after them (end_s - 64: lane 63 of
the I/O register after the last step, which the kernel stores on its own) and lane 62's own two rows.  Every
boundary is joined this way, those with a 64-row drop too: without the hand-off columns the covering fails.

As in test_wedge_identity, each chain runs with every cell outside its region poisoned, the covering condition
is asserted on the shared nodes, and

    score = max( max H of F's region, max H of B's region, max over shared nodes of H_F + H_B ).
"""
import numpy as np
import pytest

from test_wedge_identity import PARAMS, POISON, _pairs, region_dp

PATTERNS = [(64, 64, 64, 128), (64, 128, 64, 128), (128, 128, 128, 128), (64, 64, 64, 192)]


def steep_plan(n, m, d):
    """(S, lead_b, rlead, e0_f, e0_b, cum), or None where the steep plan refuses: the arithmetic of
    sw_internal.h steep_bounds."""
    assert len(d) == 4 and all(x >= 64 and x % 64 == 0 for x in d) and d[0] == d[2]
    if n < 253:
        return None
    S = (n - 2 + 125) // 126
    S = 4 * ((S + 3) // 4)
    W = 126 * S + 2
    if n + 2 > W:
        return None
    cum = np.concatenate(([0], np.cumsum([d[j % 4] for j in range(S - 1)]))).astype(np.int64)
    D = int(cum[-1])
    rlead = (3 - m) % 64
    T = m + rlead + 61 + D
    e0f = 64 * (T // 128)
    e0b = T - e0f
    if min(e0f, e0b) - D < 64 or e0f > m - 1 or e0b > m + rlead - 1:
        return None
    return S, W - 2 - n, rlead, e0f, e0b, cum


def steep_min_m(n, d):
    """The smallest m the steep plan admits at n columns."""
    m = 1
    while steep_plan(n, m, d) is None:
        m += 1
    return m


def steep_model(a, b, prm, d, segments=True):
    """(score, the best node: 'chain', 'diag', 'seg-wg' (a hand-off column behind a workgroup's last strip) or
    'seg-lds'); asserts the covering condition on the way.  segments = False leaves the hand-off columns out
    of the join (and asserts nothing about covering)."""
    n, m = len(a), len(b)
    S, lead_b, rlead, e0f, e0b, cum = steep_plan(n, m, d)
    W = 126 * S + 2

    def chain(cols, rows, e0):
        assert len(cols) == W
        hi = np.full(W, -1)
        lanes = []
        for s in range(S):
            end = e0 - int(cum[s])
            for l in range(64):
                last = end - 1 - l
                assert 0 <= last and last + 1 < len(rows), (n, m, s, l)
                c = 126 * s + 2 * l
                hi[c:c + 2] = np.maximum(hi[c:c + 2], last + 1)
                lanes.append((s, l, c, last))
        assert np.all(hi[1:] <= hi[:-1])      # closed under (up, left, up-left)
        H = region_dp(cols, rows, hi, prm)
        best = int(H[H < POISON // 2].max())
        cells = {}                            # (row, padded column) -> (H, kind) of everything the chain exports
        for s, l, c, last in lanes:
            for r in (last, last + 1) if s == 0 or l else (last,):
                for cc in (c, c + 1):
                    assert cells.setdefault((r, cc), (int(H[r, cc]), "diag"))[0] == H[r, cc]
        for s in range(S - 1):
            drop = int(cum[s + 1] - cum[s])
            end = e0 - int(cum[s])
            # the hand-off column of strip s, lane 62's column B: the last drop - 63 rows its exit flush
            # publishes (rows <= end - 65) and the row in lane 63 of its I/O register after the last step
            for r in range(end - drop - 1, end - 63) if segments else ():
                assert (r, 126 * s + 125) not in cells and r >= 0
                cells[(r, 126 * s + 125)] = (int(H[r, 126 * s + 125]), "seg-wg" if s % 4 == 3 else "seg-lds")
        return best, cells

    best_f, cf = chain(np.concatenate([a, np.zeros(W - n, np.uint8)]), b, e0f)
    best_b, cb = chain(np.concatenate([np.zeros(lead_b, np.uint8), a[::-1], np.zeros(2, np.uint8)]),
                       np.concatenate([np.zeros(rlead, np.uint8), b[::-1]]), e0b)
    nf = {(r + 1, c + 1): v for (r, c), v in cf.items()}
    nb = {(m - 1 + rlead - r, W - 3 - q): v for (r, q), v in cb.items()}
    shared = set(nf) & set(nb)
    assert max(nf[k][0] for k in shared) < POISON // 2 and max(nb[k][0] for k in shared) < POISON // 2
    for i, j in shared:   # the hand-off columns of the two chains lie on each other, and on nothing else
        assert (nf[i, j][1] == "diag" and nb[i, j][1] == "diag") or j % 126 == 0, (i, j, nf[i, j], nb[i, j])
    if segments:
        assert_covering(shared, set(nf), set(nb), n, m)
    cross, kind = max((nf[k][0] + nb[k][0], max(nf[k][1], nb[k][1])) for k in shared)
    diag = max(nf[k][0] + nb[k][0] for k in shared if nf[k][1] == "diag" and nb[k][1] == "diag")
    if cross <= max(best_f, best_b):
        kind = "chain"
    elif cross <= diag:
        kind = "diag"
    return max(best_f, best_b, cross), kind


def assert_covering(shared, nf, nb, n, m):
    """A path that neither chain finds starts above B's region and ends below F's; it passes through a shared
    node when the shared rows of every node column j are one interval [lo_j, hi_j] with hi_{j+1} >= lo_j (no
    right or diagonal move leads from above every shared row straight to below them) and no column of
    1 .. n - 1 is without one.  Node column 0 is F's border, covered from B's first row there down by B's own
    maximum; node column n is B's border in the same way."""
    rows = {}
    for i, j in shared:
        rows.setdefault(j, []).append(i)
    lo = {j: min(r) for j, r in rows.items()}
    hi = {j: max(r) for j, r in rows.items()}
    for j, r in rows.items():
        assert sorted(r) == list(range(lo[j], hi[j] + 1)), (n, m, j, sorted(r))
    lo[0] = min(i for i, j in nb if j == 0)
    hi[0] = m
    if n not in rows:
        lo[n], hi[n] = 0, max(i for i, j in nf if j == n)
    for j in range(1, n + 1):
        assert j in lo, (n, m, j)
        assert 0 <= lo[j] <= hi[j] <= m and hi[j] >= lo[j - 1], (n, m, j, lo[j - 1], lo[j], hi[j])


def _shapes(rng, d, count):
    """`count` shapes (n, m): n over S = 4, 8, 12, m from the steep admission edge to 2 n + 401."""
    for k in range(count):
        n = int(rng.integers(380, 1391))
        if steep_plan(n, 1 << 20, d) is None:     # 126 roundup4(S) < n: the steep plan refuses this width
            n -= 4
        lo = steep_min_m(n, d)
        m = [lo, lo + 1 + k % 63, lo + int(rng.integers(0, 200)), max(lo, n + 300), 2 * n + 401][k % 5]
        yield n, m


@pytest.mark.parametrize("d", PATTERNS)
def test_steep_scores_and_segments(oracle_mod, d):
    prm_t = PARAMS[PATTERNS.index(d) % 3]
    op = oracle_mod.Params(*prm_t)
    rng = np.random.default_rng(100 + PATTERNS.index(d))
    kinds = {"chain": 0, "diag": 0, "seg-wg": 0, "seg-lds": 0}
    wrong_without = 0
    for n, m in _shapes(rng, d, 20):
        for a, b in _pairs(rng, n, m):
            want = oracle_mod.score_full(a, b, op)
            got, kind = steep_model(a, b, prm_t, d)
            assert got == want, (d, n, m)
            kinds[kind] += 1
            if kind.startswith("seg"):
                wrong_without += steep_model(a, b, prm_t, d, segments=False)[0] != want
    # conditions on these seeded inputs: a segment node decides pairs of every pattern (strictly: above both
    # chains' maxima and the best non-segment shared node), an in-workgroup one where the pattern has any, and
    # the join without the segments gets pairs wrong
    assert kinds["seg-wg"] + kinds["seg-lds"] >= 1, kinds
    assert kinds["seg-lds"] >= 1 or max(d[:3]) == 64, kinds
    assert wrong_without >= 1, kinds


def test_steep_every_residue(oracle_mod):
    """Every residue of m mod 64 (every rlead) and of n mod 126 that S = 4, 8, 12 admit, two patterns."""
    prm_t = PARAMS[0]
    op = oracle_mod.Params(*prm_t)
    rng = np.random.default_rng(11)
    for res in range(126):
        d = PATTERNS[res % 2]
        S = (4, 8, 12)[res % 3]
        n = 126 * (S - 1) + 1 + res              # 126 (S - 1) < n <= 126 S, every residue mod 126
        assert steep_plan(n, 1 << 20, d)[0] == S
        m = steep_min_m(n, d) + res % 64 + 64 * int(rng.integers(0, 3))
        a, b = list(_pairs(rng, n, m))[res % 2]
        assert steep_model(a, b, prm_t, d)[0] == oracle_mod.score_full(a, b, op), (d, n, m)


def test_steep_admission():
    for d in PATTERNS:
        # 126 roundup4(S) + 2 < n + 2: no room for the forward chain's two dead columns
        assert steep_plan(505, 1 << 20, d) is None and steep_plan(1009, 1 << 20, d) is None
        assert steep_plan(504, 1 << 20, d)[0] == 4 and steep_plan(507, 1 << 20, d)[0] == 8
        for n in (380, 504, 760, 1000, 1006, 1390):
            S = steep_plan(n, 1 << 20, d)[0]
            D = (S // 4) * sum(d) - d[3]
            lo = steep_min_m(n, d)
            assert lo == D + 65, (d, n, lo)          # the issue's example: n = 1390, (64,128,64,128): 1089
            assert steep_plan(n, lo - 1, d) is None
            for m in range(lo, lo + 130):
                S_, lead_b, rlead, e0f, e0b, cum = steep_plan(n, m, d)
                assert S_ == S and cum[-1] == D and 0 <= lead_b == 126 * S - n
                assert e0f % 64 == 0 and e0b % 64 == 0 and 0 <= e0b - e0f <= 64
                assert e0f + e0b == m + rlead + 61 + D and min(e0f, e0b) - D >= 64
                assert e0f <= m - 1 and e0b <= m + rlead - 1
    assert steep_min_m(1390, (64, 128, 64, 128)) == 1089

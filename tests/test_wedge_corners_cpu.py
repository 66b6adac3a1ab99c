"""CPU: the wedge identity at the corners of the scoring-constant domain, and the inputs of
tests/test_wedge_corners.py (built here, once, for both files).

The two-wedge plans get one long pair's score from two chains and a crossing term
max H_F + H_B over the nodes the chains share: the staircase's diagonal nodes and, on a steep staircase, the
strips' hand-off columns.  wedge_model (tests/test_wedge_identity.py) and steep_model
(tests/test_steep_identity.py) restate that at the staged kernel's lane geometry; their own tests run three
constant sets with small MATCH, MISMATCH < 0 and G > 0.  Here they run at every set of
test_param_corners.CORNERS that the staged linear-gap kernel admits (flow_ok and G_INIT == G_EXT): free gaps,
G = 100, MISMATCH = 0, MATCH = 127 and MATCH <= 0 among them.  Per set and input the model must equal
oracle.score_linear, with its covering assertion holding.

The inputs earn their place, which the models decide and no kernel: under every admitted set with MATCH > 0
each plan has an input whose score the crossing term alone gives, and each steep pattern one that a
hand-off-column node alone gives ('seg-wg' / 'seg-lds': above both chains' maxima and every diagonal node)."""
import zlib

import numpy as np
import pytest

from test_param_corners import ACGT, ACGTN, CORNERS, flow_ok, linear
from test_steep_identity import steep_min_m, steep_model, steep_plan
from test_wedge_identity import wedge_model, wedge_plan

UNIFORM = (64, 64, 64, 64)
STEEP_PATTERNS = [(64, 128, 64, 128), (128, 64, 128, 128)]
PATTERNS = [UNIFORM] + STEEP_PATTERNS
# 8 and 12 strips a chain: the smallest widths whose chains have a cross-workgroup hop and a workgroup-boundary
# hand-off column
NS = [1000, 1390]
IDENT = 1000
SEED = 1

# the sets the staged two-column linear-gap kernel admits, and so the wedge plans: 10 of the 29, counted by
# hand in test_param_corners (N_FLOW_LIN)
ADMITTED = [t for t in CORNERS if flow_ok(t) and linear(t)]
POSITIVE = [t for t in ADMITTED if t[0] > 0]
ZERO = [t for t in ADMITTED if t[0] <= 0]


def stretched(rng, alpha, a, m):
    """a stretched (or squeezed) over m rows, 5 % replaced and one short insertion: corner to corner
    (as tests/test_flow3_steep.py)"""
    n = len(a)
    b = a[np.minimum((np.arange(m) * n) // m, n - 1)].copy()
    mut = rng.random(m) < 0.05
    b[mut] = alpha[rng.integers(0, len(alpha), int(mut.sum()))]
    k = int(rng.integers(5, m - 5))
    return np.ascontiguousarray(np.concatenate([b[:k], alpha[rng.integers(0, len(alpha), 2)], b[k:]])[:m])


def rows(n, d):
    """17 rows above the pattern's admission edge (the uniform plan's own: 64 S + 64), and n + 300"""
    edge = 64 * wedge_plan(n, 1 << 20)[0] + 64 if d == UNIFORM else steep_min_m(n, d)
    return [edge + 17, n + 300]


_INPUTS = {}


def inputs(d):
    """[(tag, columns, rows)] of pattern d: per width and height a random pair and a stretched copy, at 1000
    columns the same over ACGTN (the seven-letter kernel), and the identical pair of 1000, whose whole
    diagonal crosses the staircase."""
    if d not in _INPUTS:
        rng = np.random.default_rng(zlib.crc32(repr(("wedge corners", SEED, d)).encode()))
        out = []
        for alpha, name, ns in ((ACGT, "acgt", NS), (ACGTN, "acgtn", NS[:1])):
            for n in ns:
                for m in rows(n, d):
                    assert d == UNIFORM or steep_plan(n, m, d) is not None, (d, n, m)
                    assert d != UNIFORM or wedge_plan(n, m) is not None, (d, n, m)
                    a = alpha[rng.integers(0, len(alpha), n)]
                    out.append(((name, "random", n, m), a, alpha[rng.integers(0, len(alpha), m)]))
                    out.append(((name, "stretched", n, m), a, stretched(rng, alpha, a, m)))
        s = ACGT[rng.integers(0, 4, IDENT)]
        assert d == UNIFORM or steep_plan(IDENT, IDENT, d) is not None
        out.append((("acgt", "identical", IDENT, IDENT), s, s.copy()))
        _INPUTS[d] = out
    return _INPUTS[d]


_EXP = {}


def expected(oracle_mod, d, t, which=None):
    """oracle.score_linear of inputs(d) (of those at the indices `which`) under the constants t, each computed
    once."""
    ins = inputs(d)
    have = _EXP.setdefault((d, t), {})
    op = oracle_mod.Params(*t)
    for i in range(len(ins)) if which is None else which:
        if i not in have:
            have[i] = oracle_mod.score_linear(ins[i][1], ins[i][2], op)
    return [have[i] for i in (range(len(ins)) if which is None else which)]


def model(a, b, t, d):
    """(score, what decided it: 'chain', 'diag', 'seg-wg' or 'seg-lds') of the plan with the drops d"""
    if d == UNIFORM:
        score, crossed = wedge_model(a, b, t)
        return score, "diag" if crossed else "chain"
    return steep_model(a, b, t, d)


def test_admitted_sets_counted_by_hand():
    assert len(CORNERS) == 29 and len(ADMITTED) == 10 and len(POSITIVE) == 7 and len(ZERO) == 3
    assert (27, -127, 100, 100) in ADMITTED and (28, -127, 100, 100) not in ADMITTED
    assert {t[2] for t in POSITIVE} == {0, 1, 3, 27, 100}


@pytest.mark.parametrize("d", PATTERNS)
def test_identity_at_the_corners(oracle_mod, d):
    ins = inputs(d)
    assert len(ins) == 13
    crossed = {t: 0 for t in ADMITTED}
    on_segment = {t: 0 for t in ADMITTED}
    for t in ADMITTED:
        exp = expected(oracle_mod, d, t)
        for (tag, a, b), e in zip(ins, exp):
            got, kind = model(a, b, t, d)     # (asserts the covering condition)
            assert got == e, (d, t, tag, got, e)
            crossed[t] += kind != "chain"
            on_segment[t] += kind.startswith("seg")
        assert exp[-1] == max(t[0], 0) * IDENT, (d, t, exp[-1])
    print("\npattern %s: %d sets admitted, %d inputs; decided by the crossing term %s, strictly by a hand-off-column "
          "node %s" % (d, len(ADMITTED), len(ins), [crossed[t] for t in ADMITTED], [on_segment[t] for t in ADMITTED]))
    for t in ZERO:
        assert expected(oracle_mod, d, t) == [0] * len(ins) and crossed[t] == 0
    for t in POSITIVE:
        assert crossed[t] >= 1, (d, t, crossed)
        assert d == UNIFORM or on_segment[t] >= 1, (d, t, on_segment)

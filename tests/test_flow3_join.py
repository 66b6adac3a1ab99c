"""GPU parity of the wedge launch that joins its chains inside the staged kernel ("the join in
the kernel"; sw_flow3.hip f3_join_strip): no descriptor copies, no memset of the claim counter or of the score and
no combine kernel.  Every strip counts itself into the join units that read it, the wave that completes a unit runs
it, the last strip to finish writes the score.  Bit-exact against oracle.score_linear with SWMI_F3WEDGE = 1.

Covered: n = 760, 1000, 1006, 1390 (and 505, uniform only: the steep frame holds 504 columns at S = 4) with rows at
the steep admission edge, 17 above it and n + 300; the uniform pattern, (64,128,64,128) and (128,64,128,128);
random pairs and stretched copies laid corner to corner (one of whose best paths the CPU model finds on a segment
node); grids of 1, 2, 3 workgroups and the default; three pairs launched twice each, then launches alternating
patterns and SWMI_F3JOIN = 0 / 1, then an affine launch (which resets the claim counter) between two of them; a
seven-letter pair; and sw_last_stats unchanged from SWMI_F3JOIN = 0.
The corners of the scoring-constant domain over these launches: tests/test_wedge_corners.py."""
import os
import zlib

import numpy as np
import pytest

from test_steep_identity import steep_min_m, steep_model, steep_plan

pytestmark = pytest.mark.gpu

PARAMS = [(1, -1, 1, 1), (2, -3, 2, 2), (3, -1, 4, 4)]
ACGT = np.frombuffer(b"ACGT", np.uint8)
WEDGE = 1 << 18
STEEP = 1 << 19
ENV = "SWMI_F3WEDGE"
ENV_DROPS = "SWMI_F3WEDGE_DROPS"
ENV_JOIN = "SWMI_F3JOIN"
UNIFORM = (64, 64, 64, 64)
STEEP_PATTERNS = [(64, 128, 64, 128), (128, 64, 128, 128)]
NS = [760, 1000, 1006, 1390]


@pytest.fixture(autouse=True)
def _defaults(engine, request):
    def reset():
        for k in (ENV, ENV_DROPS, ENV_JOIN):
            os.environ.pop(k, None)
        engine.set_option("blocks", 0)
        engine.set_option("orient", 0)
    request.addfinalizer(reset)
    engine.set_option("orient", 1)   # seq1 across the lanes: n is its length
    os.environ[ENV] = "1"
    os.environ.pop(ENV_JOIN, None)


def _drops(d):
    os.environ[ENV_DROPS] = ",".join(str(x) for x in d)


def _join(on):
    if on:
        os.environ.pop(ENV_JOIN, None)
    else:
        os.environ[ENV_JOIN] = "0"


def _stretched(rng, alpha, a, m):
    """a stretched (or squeezed) over m rows, 5 % replaced and one short insertion: corner to corner
    (as tests/test_flow3_steep.py)"""
    n = len(a)
    b = a[np.minimum((np.arange(m) * n) // m, n - 1)].copy()
    mut = rng.random(m) < 0.05
    b[mut] = alpha[rng.integers(0, len(alpha), int(mut.sum()))]
    k = int(rng.integers(5, m - 5))
    return np.ascontiguousarray(np.concatenate([b[:k], alpha[rng.integers(0, len(alpha), 2)], b[k:]])[:m])


def _rows(n, d):
    """the steep admission edge of the pattern (the uniform plan: of (64,128,64,128); 505 columns, which no steep
    frame of four strips holds: the uniform plan's own edge 64 S + 64), 17 rows above it, and n + 300"""
    if n == 505:
        lo = 64 * ((n - 2 + 125) // 126) + 64
    else:
        lo = steep_min_m(n, STEEP_PATTERNS[0] if d == UNIFORM else d)
    return [lo, lo + 17, n + 300]


def _check(engine, oracle_mod, a, b, prm_t, tag, steep):
    exp = oracle_mod.score_linear(a, b, oracle_mod.Params(*prm_t))
    got = engine.score(a, b, engine.Params(*prm_t))
    st = engine.last_stats()
    assert got == exp, (tag, got, exp, st)
    assert st["variant"] & WEDGE and bool(st["variant"] & STEEP) == steep, (tag, st)
    return st


@pytest.mark.parametrize("d", [UNIFORM] + STEEP_PATTERNS)
def test_shapes_against_oracle(engine, oracle_mod, d):
    rng = np.random.default_rng(zlib.crc32(repr(("join", d)).encode()))
    _drops(d)
    steep = d != UNIFORM
    on_segment = 0
    for n in NS + ([] if steep else [505]):
        for m in _rows(n, d):
            assert not steep or steep_plan(n, m, d) is not None
            prm_t = PARAMS[(n + m) % 3]
            a = ACGT[rng.integers(0, 4, n)]
            for kind, y in (("random", ACGT[rng.integers(0, 4, m)]), ("stretched", _stretched(rng, ACGT, a, m))):
                _check(engine, oracle_mod, a, y, prm_t, (kind, d, n, m), steep)
            if steep and m < n + 300:
                on_segment += steep_model(a, y, prm_t, d)[1].startswith("seg")
    if d == STEEP_PATTERNS[0]:
        # stretched copies whose best path the CPU model finds on a segment node only (a property of these seeded
        # inputs, not of the kernel)
        assert on_segment >= 1, on_segment


@pytest.mark.parametrize("blocks", [1, 2, 3, 0])
def test_grids(engine, oracle_mod, blocks):
    """One workgroup running every item in order (F0, B0, F1, ...) must still complete every unit; 1390 columns are
    3 + 3 groups."""
    engine.set_option("blocks", blocks)
    rng = np.random.default_rng(300 + blocks)
    a = ACGT[rng.integers(0, 4, 1390)]
    for d, prm_t in zip([UNIFORM] + STEEP_PATTERNS, PARAMS):
        _drops(d)
        b = _stretched(rng, ACGT, a, _rows(1390, d)[1])
        st = _check(engine, oracle_mod, a, b, prm_t, ("grid", blocks, d), d != UNIFORM)
        assert st["items"] == 6 and st["blocks"] == (blocks or 6), st


def test_stats_unchanged(engine, oracle_mod):
    rng = np.random.default_rng(61)
    for d in [UNIFORM] + STEEP_PATTERNS:
        _drops(d)
        a = ACGT[rng.integers(0, 4, 1000)]
        b = _stretched(rng, ACGT, a, _rows(1000, d)[1])
        seen = []
        for on in (True, False):   # (the joining launch first: the score slot still holds the pair before)
            _join(on)
            st = _check(engine, oracle_mod, a, b, PARAMS[0], ("stats", d, on), d != UNIFORM)
            seen.append((st["items"], st["blocks"], st["variant"] & (WEDGE | STEEP), st["mode"], st["W"], st["C"]))
        assert seen[0] == seen[1], (d, seen)


def test_seven_letter_pair(engine, oracle_mod):
    alpha = np.frombuffer(b"ACGTNRY", np.uint8)
    rng = np.random.default_rng(7)
    for d in [UNIFORM] + STEEP_PATTERNS:
        _drops(d)
        n = 1000
        m = _rows(n, d)[0] + 5
        a = alpha[rng.integers(0, 7, n)]
        b = _stretched(rng, alpha, a, m)
        for prm_t in PARAMS:
            st = _check(engine, oracle_mod, a, b, prm_t, ("hep", d, prm_t), d != UNIFORM)
            assert st["dna"] == 2, st


def test_back_to_back_and_alternating(engine, oracle_mod):
    """The join counters, the claim counter's running base and the 64-bit score word live in the context from
    launch to launch: nothing of one launch may reach the next, whichever path either takes."""
    rng = np.random.default_rng(29)
    d = STEEP_PATTERNS[0]
    n, m = 1000, steep_min_m(1000, STEEP_PATTERNS[1]) + 40
    assert steep_plan(n, m, d) is not None and steep_plan(n, m, STEEP_PATTERNS[1]) is not None
    a1 = ACGT[rng.integers(0, 4, n)]
    a2 = ACGT[rng.integers(0, 4, n)]
    pairs = [(a1, _stretched(rng, ACGT, a1, m)), (a2, ACGT[rng.integers(0, 4, m)]), (a2, _stretched(rng, ACGT, a2, m))]
    exp = [oracle_mod.score_linear(x, y) for x, y in pairs]
    assert len(set(exp)) == 3
    # a high score first: a word that kept it would beat the lower ones after it
    order = sorted(range(3), key=lambda k: -exp[k])
    _drops(d)
    for k in order:
        for _ in range(2):
            assert engine.score(*pairs[k]) == exp[k], k
            assert engine.last_stats()["variant"] & STEEP
    patterns = (d, UNIFORM, STEEP_PATTERNS[1])
    for k in range(12):
        _drops(patterns[k % 3])
        _join(k % 4 in (0, 3))
        assert engine.score(*pairs[order[k % 3]]) == exp[order[k % 3]], k
        st = engine.last_stats()
        assert st["variant"] & WEDGE and bool(st["variant"] & STEEP) == (k % 3 != 1), st
    # an affine launch memsets the claim counter between two joining launches
    _join(True)
    aff = (2, -3, 5, 2)
    exp_aff = oracle_mod.score_linear(pairs[0][0], pairs[0][1], oracle_mod.Params(*aff))
    for k in range(3):
        _drops(patterns[k])
        assert engine.score(*pairs[order[0]]) == exp[order[0]], k
        assert engine.score(pairs[0][0], pairs[0][1], engine.Params(*aff)) == exp_aff
        assert not engine.last_stats()["variant"] & WEDGE
        assert engine.score(*pairs[order[2]]) == exp[order[2]], k
        assert engine.last_stats()["variant"] & WEDGE

"""GPU parity of the steep wedge plan (the model: tests/test_steep_identity.py): the two-wedge
plan with a staircase that drops more than 64 rows behind some strips, joined by sw_flow3_steep_combine_kernel
along the diagonal nodes and the strips' hand-off columns (group edges across workgroups, the chains' segment
buffers inside one).  Bit-exact against oracle.score_linear, with SWMI_F3WEDGE = 1 and the drop pattern forced by
SWMI_F3WEDGE_DROPS wherever the steep plan admits it (variant bit 19 of sw_last_stats beside bit 18).

Covered: 8 and 12 strips a chain (n = 760, 1000, 1006, 1390: S rounded up from 7, 8, 8 and 12), m at the steep
admission edge D + 65, 17 and 63 rows above it, n + 300 and 2 n + 401; random pairs and mutated copies laid
corner to corner; three linear-gap constant sets; a seven-letter pair; the patterns (64,64,64,64) (the uniform
plan), (64,64,64,128) and (64,128,64,128) and the variable unset; shapes where the steep plan refuses; grids of
1, 2 and 3 workgroups; launches back to back; a steep shape alternated with a uniform one on the same buffers;
and the automatic pattern from 4096 columns.
The corners of the scoring-constant domain over these launches: tests/test_wedge_corners.py."""
import os
import zlib

import numpy as np
import pytest

from test_steep_identity import steep_min_m, steep_model, steep_plan
from test_wedge_identity import wedge_plan

pytestmark = pytest.mark.gpu

PARAMS = [(1, -1, 1, 1), (2, -3, 2, 2), (3, -1, 4, 4)]
ACGT = np.frombuffer(b"ACGT", np.uint8)
WEDGE = 1 << 18
STEEP = 1 << 19
CUT = 1 << 17
ENV = "SWMI_F3WEDGE"
ENV_DROPS = "SWMI_F3WEDGE_DROPS"
UNIFORM = (64, 64, 64, 64)
STEEP_PATTERNS = [(64, 64, 64, 128), (64, 128, 64, 128)]
NS = [760, 1000, 1006, 1390]


@pytest.fixture(autouse=True)
def _defaults(engine, request):
    def reset():
        os.environ.pop(ENV, None)
        os.environ.pop(ENV_DROPS, None)
        engine.set_option("blocks", 0)
        engine.set_option("orient", 0)
    request.addfinalizer(reset)
    engine.set_option("orient", 1)   # seq1 across the lanes: n is its length
    os.environ[ENV] = "1"


def _drops(d):
    if d is None:
        os.environ.pop(ENV_DROPS, None)
    else:
        os.environ[ENV_DROPS] = ",".join(str(x) for x in d)


def _stretched(rng, alpha, a, m):
    """a stretched (or squeezed) over m rows, 5 % replaced and one short insertion: corner to corner"""
    n = len(a)
    b = a[np.minimum((np.arange(m) * n) // m, n - 1)].copy()
    mut = rng.random(m) < 0.05
    b[mut] = alpha[rng.integers(0, len(alpha), int(mut.sum()))]
    k = int(rng.integers(5, m - 5))
    return np.ascontiguousarray(np.concatenate([b[:k], alpha[rng.integers(0, len(alpha), 2)], b[k:]])[:m])


def _check(engine, oracle_mod, a, b, prm_t, tag, steep):
    exp = oracle_mod.score_linear(a, b, oracle_mod.Params(*prm_t))
    got = engine.score(a, b, engine.Params(*prm_t))
    st = engine.last_stats()
    assert got == exp, (tag, got, exp, st)
    assert st["variant"] & WEDGE and not st["variant"] & CUT, (tag, st)
    assert bool(st["variant"] & STEEP) == steep, (tag, st)
    S = wedge_plan(len(a), 1 << 20)[0]
    assert st["items"] == 2 * ((S + 3) // 4), (tag, st)
    return st


def _heights(n, d):
    lo = steep_min_m(n, d)
    return [lo, lo + 17, lo + 63, n + 300, 2 * n + 401]


@pytest.mark.parametrize("d", STEEP_PATTERNS)
@pytest.mark.parametrize("prm_t", PARAMS)
def test_shapes_against_oracle(engine, oracle_mod, prm_t, d):
    rng = np.random.default_rng(zlib.crc32(repr((prm_t, d)).encode()))
    _drops(d)
    on_segment = 0
    for n in NS:
        for m in _heights(n, d):
            assert steep_plan(n, m, d) is not None
            a = ACGT[rng.integers(0, 4, n)]
            for kind, y in (("random", ACGT[rng.integers(0, 4, m)]), ("stretched", _stretched(rng, ACGT, a, m))):
                _check(engine, oracle_mod, a, y, prm_t, (kind, d, n, m), True)
            if m < n + 300:
                on_segment += steep_model(a, y, prm_t, d)[1].startswith("seg")
    # stretched copies whose best path the CPU model finds on a segment node only (a property of these seeded
    # inputs, not of the kernel)
    assert on_segment >= 1, on_segment


def test_uniform_pattern_and_default(engine, oracle_mod):
    """SWMI_F3WEDGE_DROPS = 64,64,64,64 is the uniform plan; unset, the steep plan starts at
    F3_STEEP_AUTO_N columns (sw_engine.hip), far above these shapes."""
    rng = np.random.default_rng(41)
    for d in (UNIFORM, None):
        _drops(d)
        for n in NS:
            for m in _heights(n, STEEP_PATTERNS[1])[:3]:
                a = ACGT[rng.integers(0, 4, n)]
                _check(engine, oracle_mod, a, _stretched(rng, ACGT, a, m), PARAMS[0], ("uniform", d, n, m), False)


@pytest.mark.parametrize("d", STEEP_PATTERNS)
def test_refusals_keep_the_uniform_plan(engine, oracle_mod, d):
    """One row below the steep admission edge, and a width past the 126 S columns the steep plan's frame holds
    (n = 505: S = 4): bit 18 without bit 19."""
    rng = np.random.default_rng(43)
    _drops(d)
    for n, m in ((1390, steep_min_m(1390, d) - 1), (760, steep_min_m(760, d) - 1), (505, 900), (505, 2000)):
        assert steep_plan(n, m, d) is None
        a = ACGT[rng.integers(0, 4, n)]
        _check(engine, oracle_mod, a, _stretched(rng, ACGT, a, m), PARAMS[0], ("refused", d, n, m), False)
    a = ACGT[rng.integers(0, 4, 504)]        # the widest S = 4 takes
    m = steep_min_m(504, d) + 5
    _check(engine, oracle_mod, a, _stretched(rng, ACGT, a, m), PARAMS[0], ("n = 504", d, m), True)


def test_queued_pattern(engine, oracle_mod):
    """(128,64,128,128), the automatic plan's pattern for launches with more groups than CUs (sw_engine.hip
    F3_STEEP_QUEUED_DROPS): steep drops on the first and third LDS link of a workgroup."""
    rng = np.random.default_rng(53)
    d = (128, 64, 128, 128)
    _drops(d)
    for n in (760, 1390):
        for m in _heights(n, d)[:4]:
            a = ACGT[rng.integers(0, 4, n)]
            _check(engine, oracle_mod, a, _stretched(rng, ACGT, a, m), PARAMS[m % 3], ("queued", n, m), True)


def test_bad_pattern_fails_the_launch(engine):
    rng = np.random.default_rng(47)
    a = ACGT[rng.integers(0, 4, 760)]
    b = ACGT[rng.integers(0, 4, 1200)]
    for bad in ("64,64,128,64", "64,96,64,128", "64,64,64", "64,64,64,128,64", "64,64,64,320", "x"):
        os.environ[ENV_DROPS] = bad
        with pytest.raises(Exception, match="SWMI_F3WEDGE_DROPS"):
            engine.score(a, b)


@pytest.mark.parametrize("blocks", [1, 2, 3])
def test_small_grids(engine, oracle_mod, blocks):
    """Fewer workgroups than strip groups (1390 columns: 3 + 3 groups, claimed F0, B0, F1, ...)."""
    engine.set_option("blocks", blocks)
    rng = np.random.default_rng(200 + blocks)
    a = ACGT[rng.integers(0, 4, 1390)]
    for d, prm_t in zip(STEEP_PATTERNS + STEEP_PATTERNS[1:], PARAMS):
        _drops(d)
        b = _stretched(rng, ACGT, a, steep_min_m(1390, d) + 17)
        st = _check(engine, oracle_mod, a, b, prm_t, ("grid", blocks, d, prm_t), True)
        assert st["blocks"] == blocks and st["items"] == 6, st


def test_seven_letter_pair(engine, oracle_mod):
    alpha = np.frombuffer(b"ACGTNRY", np.uint8)
    rng = np.random.default_rng(7)
    d = STEEP_PATTERNS[1]
    _drops(d)
    for n, m in ((1000, steep_min_m(1000, d) + 5), (760, 1060)):
        a = alpha[rng.integers(0, 7, n)]
        b = _stretched(rng, alpha, a, m)
        for prm_t in PARAMS:
            st = _check(engine, oracle_mod, a, b, prm_t, ("hep", n, m, prm_t), True)
            assert st["dna"] == 2, st


def test_back_to_back_and_alternating(engine, oracle_mod):
    """Launches of one shape reuse the boundary and segment buffers, and a uniform launch between two steep ones
    lays its own entries over them: the epoch keys must keep every launch to its own (the combine kernels check
    every key)."""
    rng = np.random.default_rng(23)
    d = STEEP_PATTERNS[1]
    n, m = 1000, steep_min_m(1000, d) + 40
    a1 = ACGT[rng.integers(0, 4, n)]
    a2 = ACGT[rng.integers(0, 4, n)]
    pairs = [(a1, _stretched(rng, ACGT, a1, m)), (a2, ACGT[rng.integers(0, 4, m)]), (a2, _stretched(rng, ACGT, a2, m))]
    exp = [oracle_mod.score_linear(x, y) for x, y in pairs]
    assert len(set(exp)) == 3
    _drops(d)
    for _ in range(2):
        for (x, y), e in zip(pairs, exp):
            assert engine.score(x, y) == e
            assert engine.last_stats()["variant"] & STEEP
    for k in range(6):
        x, y = pairs[k % 3]
        _drops((d, UNIFORM, STEEP_PATTERNS[0])[k % 3])
        assert engine.score(x, y) == exp[k % 3]
        st = engine.last_stats()
        assert st["variant"] & WEDGE and bool(st["variant"] & STEEP) == (k % 3 != 1), st


def test_automatic_pattern(engine, oracle_mod):
    """Both variables unset: from 4096 columns (sw_engine.hip F3_STEEP_AUTO_N) the steep plan with the measured
    pattern (64,128,64,128) wherever it is admissible, the uniform wedge one row below that."""
    os.environ.pop(ENV, None)
    rng = np.random.default_rng(51)
    n, d = 4096, STEEP_PATTERNS[1]
    lo = steep_min_m(n, d)
    a = ACGT[rng.integers(0, 4, n)]
    for m, steep in ((lo, True), (n, True), (lo - 1, False)):
        _check(engine, oracle_mod, a, _stretched(rng, ACGT, a, m), PARAMS[0], ("auto", m), steep)

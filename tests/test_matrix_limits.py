"""GPU: the matrix kernels (csrc/sw_matrix.hip: score-only W = 1/2/4/8, traced, the walk, the long
path; local, global, semi-global) at the limits of the domain include/algoGPU.h declares, where no
other test runs them.  Every comparison is bit-exact, and the yardsticks are shown to hold at these
limits, without a GPU, in tests/test_matrix_limits_cpu.py, which also defines the shared inputs.

A. the alphabet: K = 32 (row and column 31 of the LDS table and the sentinel at index 32 are live),
   K = 2 and K = 1; B. entries over the whole of [-127, 127], asymmetric, on low-complexity pairs;
C. global and semi-global with gap penalties one unit inside the mode range bound, against
   `restate` (float matrices, -inf borders: nothing in it can wrap as the kernels' and the CPU
   aligner's common -2^30 could); D. local at gap penalties of 2^20; E. the claim loop and launch
   splitting in the mode instantiations; F. empty and 1-residue records and queries in a mode search.

Local scores go against check_many (tests/test_matrix.py), local alignments against the CPU aligner
and `rescore`, the modes against `restate` and `rescore_ops` (tests/test_modes_cpu.py).

What these tests were seen to notice on an MI355X, each in a build with that one defect, which the
tests of test_matrix.py, test_align.py and test_modes.py all pass: a table row stride of 32 (the
sentinel at index 32 lands in the next row: the K = 32 local tests); +127 for every -127 of the
transposed table (the local tests under FULL32 and TAB2); a MAT_NEG with 2^16 of headroom above
-2^31 instead of 2^30 (every multi-column case of C, nothing else); no host answer for an empty
record or query in a mode search (F).  The kernels as they are pass everything here."""
import numpy as np
import pytest

from test_matrix_cpu import byte_codes
from test_matrix import check_many
from test_align_cpu import end_cell, rescore
from test_modes_cpu import check_shape, rescore_ops, restate
from test_matrix_limits_cpu import (BIG_GAPS, CODE1, CODE2, CODE32, EDGE_SHAPES, FULL32, LAST, S32, SYM1, SYM2, SYM32, TAB1, TAB2,
                                    as_tuple, edge_gaps, edge_pairs, edge_u, edge_want, has_last, mutated32, pair32, rand32)

MODES = ("global", "semiglobal")
AM = {"local": 0, "global": 1, "semiglobal": 2}
RANGE_MESSAGE = "pair 0: score range exceeds the int32 engine in this mode"
_cache = {}


def cached(key, make):
    """A reference: computed once, shared among the tests, never changed."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def local_ref(key, pairs, T, gaps, code):
    return cached(("local", key, gaps), lambda: check_many(pairs, T, *gaps, code))


def restate_ref(key, pairs, T, gaps, mode, code):
    return cached(("restate", key, gaps, mode), lambda: tuple(restate(a, b, T, *gaps, mode, code) for a, b in pairs))


def cpu_ref(engine, key, pairs, sym, T, gaps, mode="local", **matrix_args):
    def make():
        with engine.Matrix(sym, T, **matrix_args) as mx:
            return tuple(engine.align_matrix_batch(pairs, mx, *gaps, cpu=True, mode=mode))
    return cached(("cpu", key, gaps, mode), make)


def force(engine, request, **options):
    """Sets engine options for this test; a finalizer restores the defaults."""
    defaults = {"W": 0, "blocks": 0, "trace_mb": 1024}
    request.addfinalizer(lambda: [engine.set_option(k, defaults[k]) for k in options])
    for k, v in options.items():
        engine.set_option(k, v)


def pair_cost(n, m, W):
    """The launch's estimate (csrc/sw_matrix.hip pair_cost): a local score-only launch puts seq2 across
    the lanes, under the transposed table, where that is cheaper."""
    return -(-n // (64 * W)) * ((m + 64 * W - 1 + 63) // 64) * 64 * (9 * W + 8)


def swapped(pairs, W):
    return sum(pair_cost(len(b), len(a), W) < pair_cost(len(a), len(b), W) for a, b in pairs)


def local_scores(engine, pairs, sym, T, gaps, want, W, **matrix_args):
    """Both orientations: (a, b) under T and (b, a) under its transpose; the launch swaps some of each."""
    flipped = [(b, a) for a, b in pairs]
    with engine.Matrix(sym, T, **matrix_args) as mx, engine.Matrix(sym, T.T, **matrix_args) as mt:
        got = engine.score_matrix_batch(pairs, mx, *gaps)
        st = engine.last_stats()
        back = engine.score_matrix_batch(flipped, mt, *gaps)
    assert st["mode"] == 6 and st["variant"] == 0 and st["items"] == len(pairs)
    assert st["W"] == W or (W == 0 and st["W"] in (1, 2, 4, 8))
    bad = [(k, len(a), len(b), g, w) for k, ((a, b), g, w) in enumerate(zip(pairs, got, want)) if g != w]
    assert not bad, (gaps, st["W"], len(bad), bad[:8])
    bad = [(k, len(a), len(b), g, w) for k, ((a, b), g, w) in enumerate(zip(flipped, back, want)) if g != w]
    assert not bad, ("transposed", gaps, len(bad), bad[:8])
    return st["W"]


def local_alignments(engine, key, pairs, sym, T, code, gaps, long=False, **matrix_args):
    """align_matrix_batch or align_matrix_long against the CPU aligner, each alignment re-scored."""
    want = cpu_ref(engine, key, pairs, sym, T, gaps, **matrix_args)
    with engine.Matrix(sym, T, **matrix_args) as mx:
        got = (engine.align_matrix_long if long else engine.align_matrix_batch)(pairs, mx, *gaps)
        st = engine.last_stats()
    assert st["mode"] == (8 if long else 7) and st["W"] == 8 and st["items"] == len(pairs) and len(got) == len(pairs)
    for k, ((a, b), g, w) in enumerate(zip(pairs, got, want)):
        assert g == w, (long, gaps, k, len(a), len(b), g, w)
        assert rescore(g, a, b, T, *gaps, code) == g.score, (gaps, k)
    return got


def mode_scores(engine, request, pairs, sym, T, gaps, mode, want, widths=(1, 2, 4, 8), **matrix_args):
    """The score-only mode kernel at every forced W against `want` (restate's tuples or plain scores)."""
    want = [w[0] if isinstance(w, tuple) else w for w in want]
    for W in widths:
        force(engine, request, W=W)
        with engine.Matrix(sym, T, **matrix_args) as mx:
            got = engine.score_matrix_batch(pairs, mx, *gaps, mode=mode)
            st = engine.last_stats()
        assert st["mode"] == 6 and st["variant"] == AM[mode] and (W == 0 or st["W"] == W)
        bad = [(k, len(a), len(b), g, w) for k, ((a, b), g, w) in enumerate(zip(pairs, got, want)) if g != w]
        assert not bad, (mode, gaps, W, len(bad), bad[:8])
    engine.set_option("W", 0)


def mode_alignments(engine, pairs, sym, T, code, gaps, mode, want, **matrix_args):
    """The traced mode kernel and the walk against `restate`: score, coordinates, operations, re-scored."""
    with engine.Matrix(sym, T, **matrix_args) as mx:
        got = engine.align_matrix_batch(pairs, mx, *gaps, mode=mode)
        st = engine.last_stats()
    assert st["mode"] == 7 and st["W"] == 8 and st["variant"] >> 28 == AM[mode] and len(got) == len(pairs)
    for k, ((a, b), g, w) in enumerate(zip(pairs, got, want)):
        assert as_tuple(g) == w, (mode, gaps, k, len(a), len(b), g, w)
        assert rescore_ops(g, a, b, T, *gaps, code) == g.score, (mode, gaps, k)
        check_shape(g, a, b, mode)
    return got


# ---- A. the alphabet: K = 32 -----------------------------------------------------------------------------

def grid32():
    """Lane, strip and chunk edges for every W, half random, half mutated copies, and four pairs whose
    orientation the launch swaps at every W; every sequence of every pair holds the last symbol."""
    def make():
        rng = np.random.default_rng(3400)
        pairs = []
        for i, n in enumerate((1, 64, 65, 512, 513, 1025)):
            for j, m in enumerate((1, 33, 64, 65, 300)):
                pairs.append(pair32(rng, n, m, (i + j) % 2 == 1, tail=True))
        return pairs + [pair32(rng, 1100, 30, False), pair32(rng, 30, 1100, True), pair32(rng, 900, 40, True),
                        pair32(rng, 40, 900, False)]
    return cached("grid32", make)


GRID_GAPS = [(12, 1), (90, 7)]


@pytest.mark.gpu
@pytest.mark.parametrize("W", [0, 1, 2, 4, 8])
def test_k32_local_scores(engine, request, W):
    pairs = grid32()
    assert has_last(pairs) and len(pairs) == 34
    force(engine, request, W=W)
    for gaps in GRID_GAPS:
        want = local_ref("grid32", pairs, FULL32, gaps, CODE32)
        used = local_scores(engine, pairs, SYM32, FULL32, gaps, want, W)
        # the launch really swaps: some pairs of each orientation are cheaper the other way round
        assert swapped(pairs, used) >= 1 and swapped([(b, a) for a, b in pairs], used) >= 1
        assert max(want) > 5000 and want != local_ref("grid32-transposed", pairs, FULL32.T, gaps, CODE32)


@pytest.mark.gpu
@pytest.mark.parametrize("gaps", GRID_GAPS)
def test_k32_local_alignments(engine, gaps):
    pairs = grid32()
    got = local_alignments(engine, "grid32", pairs, SYM32, FULL32, CODE32, gaps)
    assert [x.score for x in got] == local_ref("grid32", pairs, FULL32, gaps, CODE32)
    assert local_alignments(engine, "grid32", pairs, SYM32, FULL32, CODE32, gaps, long=True) == got
    assert sum(len(x.ops) > 2 for x in got) > 8 and any(x.beg1 < 512 < x.end1 for x in got)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_k32_modes(engine, request, mode):
    pairs, gaps = grid32(), (25, 3)
    want = restate_ref("grid32", pairs, FULL32, gaps, mode, CODE32)
    mode_scores(engine, request, pairs, SYM32, FULL32, gaps, mode, want, widths=(0, 1, 2, 4, 8))
    mode_alignments(engine, pairs, SYM32, FULL32, CODE32, gaps, mode, want)
    assert min(w[0] for w in want) < -1000 and max(w[0] for w in want) > 1000


@pytest.mark.gpu
def test_k32_strangers_go_to_the_last_row(engine, request):
    """other = 31: every byte outside the alphabet is the last symbol, the table's row and column 31."""
    rng = np.random.default_rng(3410)
    code = byte_codes(SYM32, 31)
    pairs = []
    for n, m in ((70, 90), (513, 65), (64, 300), (300, 700), (1, 1), (1030, 40)):
        a, b = rand32(rng, n), rand32(rng, m)
        a[rng.integers(0, n, 1 + n // 9)] = rng.integers(0, 256, 1 + n // 9)       # any byte
        b[rng.integers(0, m, 1 + m // 9)] = np.frombuffer(b"ac@~\x00\xff", np.uint8)[rng.integers(0, 6, 1 + m // 9)]
        pairs.append((a, b))
    assert sum(int((CODE32[a] < 0).sum() + (CODE32[b] < 0).sum()) for a, b in pairs) > 100
    gaps = (12, 1)
    want = check_many(pairs, FULL32, *gaps, code)
    for W in (0, 1, 8):
        force(engine, request, W=W)
        local_scores(engine, pairs, SYM32, FULL32, gaps, want, W, other=31)
    engine.set_option("W", 0)
    got = local_alignments(engine, "strangers", pairs, SYM32, FULL32, code, gaps, other=31)
    assert [x.score for x in got] == want
    for mode in MODES:
        ref = [restate(a, b, FULL32, *gaps, mode, code) for a, b in pairs]
        mode_scores(engine, request, pairs, SYM32, FULL32, gaps, mode, ref, widths=(1, 8), other=31)
        mode_alignments(engine, pairs, SYM32, FULL32, code, gaps, mode, ref, other=31)
    with engine.Matrix(SYM32, FULL32) as mx:                 # other = -1: the same bytes are an error
        with pytest.raises(engine.SwError, match="pair 0: seq"):
            engine.score_matrix_batch(pairs, mx, *gaps)


# ---- A. the alphabet: K = 2 and K = 1 --------------------------------------------------------------------

def small_grid(sym):
    def make():
        rng = np.random.default_rng(3420 + len(sym))
        s = np.frombuffer(sym, np.uint8)
        shapes = [(n, m) for n in (1, 65, 513, 1025) for m in (1, 65, 300)] + [(1100, 30), (30, 1100), (600, 600), (1100, 70)]
        return [(s[rng.integers(0, len(s), n)], s[rng.integers(0, len(s), m)]) for n, m in shapes]
    return cached(("small", sym), make)


SMALL = {"K2": (SYM2, TAB2, CODE2), "K1": (SYM1, TAB1, CODE1)}


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["K2", "K1"])
def test_small_alphabet_local(engine, request, which):
    sym, T, code = SMALL[which]
    pairs = small_grid(sym)
    assert [(len(a), len(b)) for a, b in pairs[-2:]] == [(600, 600), (1100, 70)] and (1, 1) == (len(pairs[0][0]), len(pairs[0][1]))
    for gaps in ((3, 1), (0, 0)):
        want = local_ref(which, pairs, T, gaps, code)
        for W in (0, 1, 2, 4, 8):
            force(engine, request, W=W)
            local_scores(engine, pairs, sym, T, gaps, want, W)
        engine.set_option("W", 0)
        got = local_alignments(engine, which, pairs, sym, T, code, gaps)
        assert local_alignments(engine, which, pairs, sym, T, code, gaps, long=True) == got
        assert [x.score for x in got] == want and max(want) >= (3000 if which == "K1" else 1000)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", ["K2", "K1"])
def test_small_alphabet_modes(engine, request, which, mode):
    sym, T, code = SMALL[which]
    pairs = small_grid(sym)
    for gaps in ((3, 1), (0, 0)):
        want = restate_ref(which, pairs, T, gaps, mode, code)
        mode_scores(engine, request, pairs, sym, T, gaps, mode, want)
        got = mode_alignments(engine, pairs, sym, T, code, gaps, mode, want)
        if which == "K1" and mode == "semiglobal" and gaps == (3, 1):   # the smallest j: poly-A's first full cover
            assert as_tuple(got[-3]) == (150, 0, 30, 0, 30, ((30, "M"),))


# ---- B. full-range entries on low-complexity pairs: ties meet steps of +-127 ---------------------------

def low_complexity32():
    def make():
        rng = np.random.default_rng(3430)
        poly = lambda n: np.full(n, LAST, np.uint8)
        two = lambda n: S32[rng.choice([0, 31], n)]
        tile = rand32(rng, 7)
        other = tile.copy()
        other[3] = LAST
        rep = np.tile(tile, 12)
        return [(poly(30), poly(30)), (poly(40), poly(7)), (poly(5), poly(33)), (two(50), two(45)), (two(20), two(64)),
                (rep, rep[:29]), (rep[3:], np.concatenate([rep[:10], rep[14:]])), (poly(70), two(70)), (two(66), poly(9)),
                (poly(1100), poly(70)), (poly(70), poly(1100)), (poly(600), poly(600)), (two(700), two(520)),
                (np.tile(tile, 90), np.tile(other, 30)), (np.tile(other, 75), np.tile(tile, 150))]
    return cached("low32", make)


LOW_GAPS = [(12, 1), (0, 0), (127, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("gaps", LOW_GAPS)
def test_full_range_ties_local(engine, gaps):
    pairs = low_complexity32()
    got = local_alignments(engine, "low32", pairs, SYM32, FULL32, CODE32, gaps)
    assert local_alignments(engine, "low32", pairs, SYM32, FULL32, CODE32, gaps, long=True) == got
    several = 0
    for (a, b), x in zip(pairs[:9], got):
        score, i, j, cand = end_cell(a, b, FULL32, *gaps, CODE32)
        assert (x.score, x.end1, x.end2) == (score, i + 1, j + 1)
        several += cand > 1
    assert several >= 1
    assert (got[9].end1, got[9].end2, got[9].score) == (70, 70, 70 * 127) and (got[11].end1, got[11].end2) == (600, 600)
    with engine.Matrix(SYM32, FULL32) as mx:
        assert engine.score_matrix_batch(pairs, mx, *gaps) == [x.score for x in got]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gaps", LOW_GAPS)
def test_full_range_ties_modes(engine, request, gaps, mode):
    pairs = low_complexity32()
    want = restate_ref("low32", pairs, FULL32, gaps, mode, CODE32)
    mode_scores(engine, request, pairs, SYM32, FULL32, gaps, mode, want, widths=(1, 8))
    got = mode_alignments(engine, pairs, SYM32, FULL32, CODE32, gaps, mode, want)
    assert list(got) == list(cpu_ref(engine, "low32", pairs, SYM32, FULL32, gaps, mode))
    if mode == "semiglobal" and gaps == (12, 1):
        assert (got[10].beg2, got[10].end2, got[10].ops) == (0, 70, ((70, "M"),))


# ---- C. gap penalties one unit inside the mode bound ------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_gaps_one_unit_inside_the_mode_bound(engine, request, shape, mode):
    n, m = shape
    u = edge_u(n, m)
    assert (n + m + 1024) * u < (1 << 28) <= (n + m + 1024) * (u + 1)
    pairs = edge_pairs(shape)                               # a batch of its own: the gaps are the batch's
    assert has_last(pairs) and [(len(a), len(b)) for a, b in pairs] == [shape, shape]
    lowest = 0
    for gaps in edge_gaps(n, m):
        want = edge_want(shape, gaps, mode)
        mode_scores(engine, request, pairs, SYM32, FULL32, gaps, mode, want)
        mode_alignments(engine, pairs, SYM32, FULL32, CODE32, gaps, mode, want)
        if gaps == (u, u):
            lowest = min(w[0] for w in want)
    assert lowest < -(1 << 24) or mode == "semiglobal"        # the scores are far from the comfortable corner
    # one unit more: refused with the range message, nothing launched
    before = engine.last_stats()
    with engine.Matrix(SYM32, FULL32) as mx:
        for gaps in ((u + 1, u + 1), (u + 1, 1), (0, u + 1)):
            with pytest.raises(engine.SwError, match=RANGE_MESSAGE):
                engine.score_matrix_batch(pairs, mx, *gaps, mode=mode)
            with pytest.raises(engine.SwError, match=RANGE_MESSAGE):
                engine.align_matrix_batch(pairs, mx, *gaps, mode=mode)
    assert engine.last_stats() == before


# ---- D. local at gap penalties of 2^20 --------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("gaps", BIG_GAPS)
def test_local_at_large_gaps(engine, request, gaps):
    pairs = grid32()[::3]
    want = local_ref("grid32/3", pairs, FULL32, gaps, CODE32)
    for W in (1, 8):
        force(engine, request, W=W)
        local_scores(engine, pairs, SYM32, FULL32, gaps, want, W)
    engine.set_option("W", 0)
    got = local_alignments(engine, "grid32/3", pairs, SYM32, FULL32, CODE32, gaps)
    assert local_alignments(engine, "grid32/3", pairs, SYM32, FULL32, CODE32, gaps, long=True) == got
    assert [x.score for x in got] == want and max(want) > 3000
    if gaps[0] <= 1:
        assert any(len(x.ops) > 1 for x in got)              # cheap openings are taken, one residue at a time
    else:
        assert all(len(x.ops) <= 1 for x in got)             # no gap is worth 2^20


# ---- E. the claim loop and launch splitting in the mode instantiations ------------------------------------

def claim_batch():
    """300 short pairs and five multi-strip pairs of different lengths: with one or two workgroups a
    wave claims many pairs, and its scratch column is reused between pairs of different m."""
    def make():
        rng = np.random.default_rng(3450)
        pairs = []
        for k in range(300):
            n, m = (int(x) for x in rng.integers(1, 49, 2))
            a = rand32(rng, n)
            pairs.append((a, mutated32(rng, a, m) if k % 2 else rand32(rng, m)))
        for n, m in ((700, 500), (640, 333), (90, 1100), (1030, 64), (513, 300)):
            pairs.append(pair32(rng, n, m, True))
        order = rng.permutation(len(pairs))                  # the long pairs anywhere in the input
        return [pairs[k] for k in order]
    return cached("claim", make)


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_claim_loop_in_the_modes(engine, request, mode, blocks):
    pairs, gaps = claim_batch(), (90, 7)
    want = cpu_ref(engine, "claim", pairs, SYM32, FULL32, gaps, mode)
    scores = [x.score for x in want]
    force(engine, request, blocks=blocks, W=0)
    with engine.Matrix(SYM32, FULL32) as mx:
        for W in (0, 1):
            engine.set_option("W", W)
            assert engine.score_matrix_batch(pairs, mx, *gaps, mode=mode) == scores
            st = engine.last_stats()
            assert st["blocks"] == blocks and st["items"] == len(pairs) and st["variant"] == AM[mode] and st["boundary_bytes"] > 0
            assert W == 0 or st["W"] == 1
            assert engine.score_matrix_batch(pairs[::-1], mx, *gaps, mode=mode) == scores[::-1]
        engine.set_option("W", 0)
        got = engine.align_matrix_batch(pairs, mx, *gaps, mode=mode)
        st = engine.last_stats()
        assert st["mode"] == 7 and st["blocks"] == blocks and st["variant"] == (AM[mode] << 28) + 1
        assert got == list(want)
        assert engine.align_matrix_batch(pairs[::-1], mx, *gaps, mode=mode) == list(want)[::-1]
    for (a, b), x in zip(pairs, got):
        assert rescore_ops(x, a, b, FULL32, *gaps, CODE32) == x.score
        check_shape(x, a, b, mode)
    assert min(scores) < 0 < max(scores)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_launch_splitting_in_the_modes(engine, request, mode):
    pairs, gaps = claim_batch(), (90, 7)
    want = list(cpu_ref(engine, "claim", pairs, SYM32, FULL32, gaps, mode))
    force(engine, request, blocks=0, trace_mb=1)
    with engine.Matrix(SYM32, FULL32) as mx:
        assert engine.align_matrix_batch(pairs, mx, *gaps, mode=mode) == want
        st = engine.last_stats()
        assert st["mode"] == 7 and st["variant"] >> 28 == AM[mode] and st["variant"] & 0xFFFFFFF > 1
        assert 0 < st["boundary_bytes"] <= (1 << 20)
        assert engine.align_matrix_batch(pairs[::-1], mx, *gaps, mode=mode) == want[::-1]


# ---- F. mode database edges ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def edge_db():
    """40 records: empty ones, 1-residue ones, the long query itself, mutated copies of it, random ones."""
    rng = np.random.default_rng(3460)
    q600 = pair32(rng, 600, 1, False)[0]
    recs = []
    for i in range(40):
        if i % 9 == 0:
            r = np.zeros(0, np.uint8)
        elif i % 9 == 1:
            r = rand32(rng, 1)
        elif i % 4 == 2:
            r = pair32(rng, 600, int(rng.integers(30, 700)), True)[1] if i % 8 == 2 else rand32(rng, int(rng.integers(2, 700)))
        else:
            r = rand32(rng, int(rng.integers(2, 300)))
        recs.append(("rec%d" % i, r))
    recs[5] = ("rec5", q600.copy())
    recs[14] = ("rec14", np.concatenate([rand32(rng, 40), q600[100:500], rand32(rng, 60)]))
    return recs, (np.zeros(0, np.uint8), q600[77:78].copy(), q600)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_mode_database_edges(engine, edge_db, mode):
    recs, queries = edge_db
    lens = [len(r) for _, r in recs]
    assert lens.count(0) == 5 and lens.count(1) >= 4
    with engine.Database.from_records(recs) as db, engine.Matrix(SYM32, FULL32) as mx:
        for go, ge in ((90, 7), (3, 7)):
            gx = min(go, ge)
            for qi, q in enumerate(queries):
                want = cpu_ref(engine, "db%d" % qi, [(q, r) for _, r in recs], SYM32, FULL32, (go, ge), mode)
                scores = db.search(q, matrix=mx, gap_init=go, gap_ext=ge, mode=mode)
                assert scores.tolist() == [x.score for x in want], (mode, qi)
                # the empty cases, as tests/test_modes_cpu.py::test_empty_sequences states them
                for i, L in enumerate(lens):
                    if len(q) == 0:
                        assert scores[i] == (-(go + (L - 1) * gx) if mode == "global" and L else 0)
                    elif L == 0:
                        assert scores[i] == -(go + (len(q) - 1) * gx)
                idx = list(range(40)) + [0, 0, 5, 1, 1, 9]
                got = db.align(q, idx, mx, go, ge, mode=mode)
                assert got == [want[i] for i in idx], (mode, qi)
                for i, x in zip(idx, got):
                    assert rescore_ops(x, q, recs[i][1], FULL32, go, ge, CODE32) == x.score
                    check_shape(x, q, recs[i][1], mode)
                order = sorted(range(40), key=lambda i: (-int(scores[i]), i))[:9]
                top = db.top(q, k=9, matrix=mx, gap_init=go, gap_ext=ge, alignments=True, mode=mode)
                assert [t[:3] for t in top] == [(int(scores[i]), i, "rec%d" % i) for i in order]
                assert [t[3] for t in top] == [want[i] for i in order]
            assert got[5].score >= int(FULL32.diagonal()[CODE32[q]].sum()) and min(scores) < 0 < max(scores)
            if mode == "semiglobal" and go == 90:             # the record that holds 400 residues of the query
                assert got[14].score > 20000 and any(op == "M" and n > 100 for n, op in got[14].ops)

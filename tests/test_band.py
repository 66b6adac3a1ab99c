"""GPU: banded alignment under a substitution matrix (include/algoGPU.h sw_*_band; the band
instantiations of the matrix kernel, the traced kernel and the band walk of csrc/sw_matrix.hip).
Every GPU alignment is compared bit for bit -- score, the four coordinates, the operations -- with
the library's CPU banded aligner (sw_align_matrix_cpu_band, itself checked against a float
restatement in tests/test_band_cpu.py), and with the score-only band kernels.

1. strip and chunk edges: every mode, every band, every forced W; 2. the band edge: a 40-residue
gap at B = 39 and B = 40; 3. stale hand-off rows: one wave, wide band then narrow bands; 4. a band
that holds the whole matrix equals no band; 5. ties and low complexity; 6. a pair refused whole and
aligned banded, and the band's own refusal; 7. penalties one unit inside the score-range bound."""
import numpy as np
import pytest

from test_matrix import SYMBOLS, mutated_copy, rand_seq, table  # noqa: F401  (fixtures)
from test_align_cpu import low_complexity_pairs
from test_modes_cpu import rescore_ops, check_shape
from test_band_cpu import columns_in_band, restate_band
from test_matrix_limits_cpu import CODE32, FULL32, SYM32, edge_u, pair32

MODES = ("local", "global", "semiglobal")
AM = {"local": 0, "global": 1, "semiglobal": 2}
_cpu_cache = {}


def cpu_ref(engine, key, pairs, T, go, ge, mode, band, symbols=SYMBOLS):
    """The CPU banded aligner's alignments of a named set of pairs: computed once, shared, never changed."""
    k = (key, go, ge, mode, band)
    if k not in _cpu_cache:
        with engine.Matrix(symbols, T) as mx:
            _cpu_cache[k] = tuple(engine.align_matrix_batch(pairs, mx, go, ge, cpu=True, mode=mode, band=band))
    return _cpu_cache[k]


def plan_cells(engine, pairs, band):
    return sum(engine.band_plan(len(a), len(b), band)["cells"] for a, b in pairs if len(a) and len(b))


def both(engine, key, pairs, T, go, ge, mode, band, symbols=SYMBOLS, code=None):
    """The GPU alignments in the band, after comparing them with the CPU banded aligner's and with the
    score-only band launch, re-scoring each and checking the launches' statistics."""
    want = cpu_ref(engine, key, pairs, T, go, ge, mode, band, symbols)
    with engine.Matrix(symbols, T) as mx:
        got = engine.align_matrix_batch(pairs, mx, go, ge, mode=mode, band=band)
        st = engine.last_stats()
        scores = engine.score_matrix_batch(pairs, mx, go, ge, mode=mode, band=band)
        ss = engine.last_stats()
    assert len(got) == len(pairs) == len(scores)
    assert st["mode"] == 10 and st["W"] == 8 and st["items"] == len(pairs) and st["variant"] >> 28 == AM[mode]
    assert ss["mode"] == 9 and ss["variant"] == AM[mode]
    assert st["cells"] == ss["cells"] == plan_cells(engine, pairs, band)
    extra = () if code is None else (code,)
    for k, ((a, b), g, w, s) in enumerate(zip(pairs, got, want, scores)):
        assert g == w, (mode, band, k, len(a), len(b), g, w)
        assert s == w.score, (mode, band, k, len(a), len(b), s, w.score)
        assert rescore_ops(g, a, b, T, go, ge, *extra) == g.score, k
        assert columns_in_band(g, len(a), len(b), band)
        check_shape(g, a, b, mode)
    return got


# ---- 1. strip and chunk edges -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def grid_pairs():
    rng = np.random.default_rng(171)
    pairs = []
    for n in (1, 63, 64, 65, 511, 512, 513, 1025, 1537):
        for m in (1, 64, 65, 300, 700, 1600):
            a = rand_seq(rng, n)
            pairs.append((a, mutated_copy(rng, a[max(0, n - m - 5):], m) if len(pairs) % 2 else rand_seq(rng, m)))
    return pairs


BANDS = (0, 1, 63, 64, 300)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("band", BANDS)
def test_traced_strip_and_chunk_edges(engine, table, grid_pairs, band, mode):
    for gaps in ((12, 1), (1, 3)):
        got = both(engine, "grid", grid_pairs, table, *gaps, mode, band)
        assert max(x.score for x in got) > 300


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W", [1, 2, 4, 8])
def test_score_kernels_every_w(engine, request, table, grid_pairs, W, mode):
    request.addfinalizer(lambda: engine.set_option("W", 0))
    engine.set_option("W", W)
    for band in BANDS:
        for gaps in ((12, 1), (0, 0)):
            want = [x.score for x in cpu_ref(engine, "grid", grid_pairs, table, *gaps, mode, band)]
            with engine.Matrix(SYMBOLS, table) as mx:
                got = engine.score_matrix_batch(grid_pairs, mx, *gaps, mode=mode, band=band)
                st = engine.last_stats()
            assert st["W"] == W and st["mode"] == 9 and st["variant"] == AM[mode]
            assert st["cells"] == plan_cells(engine, grid_pairs, band)
            bad = [(k, len(a), len(b), g, w) for k, ((a, b), g, w) in enumerate(zip(grid_pairs, got, want)) if g != w]
            assert not bad, (band, gaps, len(bad), bad[:8])


# ---- 2. the band edge -----------------------------------------------------------------------------------

def gap40_pairs(rng, at, length):
    """Two sequences of one length whose best alignments need a 40-residue gap: seq1 holds a block of
    40 at `at` that seq2 lacks, and seq2 ends in 40 residues of its own.  The path leaves the main
    diagonal by exactly 40 (test_align_long.deletion_pairs' construction: the run can slide neither way)."""
    a = rand_seq(rng, length, 20)
    if a[at - 1] == a[at + 39]:
        a[at - 1] = SYMBOLS[(SYMBOLS.index(bytes([a[at - 1]])) + 1) % 20]
    b = np.concatenate([a[:at], a[at + 40:], rand_seq(rng, 40, 20)])
    assert len(a) == len(b)
    return [(a, b), (b, a)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("at", [200, 492], ids=["inside-a-strip", "straddling-column-512"])
def test_the_band_edge(engine, table, at, mode):
    rng = np.random.default_rng(172 + at)
    pairs = gap40_pairs(rng, at, 900)
    with engine.Matrix(SYMBOLS, table) as mx:
        whole = engine.align_matrix_batch(pairs, mx, 12, 1, mode=mode)
    assert any(n >= 40 and op == "I" for n, op in whole[0].ops) and any(n >= 40 and op == "D" for n, op in whole[1].ops)
    wide = both(engine, ("gap40", at), pairs, table, 12, 1, mode, 40)
    assert list(wide) == list(whole)                        # the path touches diagonal 40 and no further
    narrow = both(engine, ("gap40", at), pairs, table, 12, 1, mode, 39)
    for x, w in zip(narrow, whole):
        assert x.score < w.score, (mode, at, x, w)


# ---- 3. stale hand-off rows -------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_stale_handoff_rows(engine, request, table, mode):
    """One launch of one workgroup (blocks=1: four waves, which claim the pairs largest first).  Four
    long pairs with a wide band (|m - n| = 1300) come first, one for every wave; the pairs with
    n = 1537 and a narrow band (|m - n| <= 63) follow, each on a wave whose scratch column still holds
    the wide pair's rows, which lie outside the rows the narrow band's strips store.  Then the other
    way round: narrow pairs first, pairs with a wide band (1537 x 300) after them."""
    request.addfinalizer(lambda: engine.set_option("blocks", 0))
    engine.set_option("blocks", 1)
    rng = np.random.default_rng(173)

    def pair(n, m):
        a = rand_seq(rng, n, 20)
        return (a, mutated_copy(rng, a[max(0, n - m - 5):], m))

    wide_first = [pair(3000, 1700) for _ in range(4)] + [pair(1537, m) for m in (1537, 1500, 1600, 1540)]
    narrow_first = [pair(1537, m) for m in (1537, 1600, 1550, 1580)] + [pair(1537, 300) for _ in range(3)]
    for batch in (wide_first, wide_first[::-1], narrow_first, narrow_first[::-1]):
        for band in (3, 1, 0):                               # 1: row i0 + dhi of a strip's inflow is one the left strip never stored
            with engine.Matrix(SYMBOLS, table) as mx:
                got = engine.align_matrix_batch(batch, mx, 12, 1, mode=mode, band=band)
                st = engine.last_stats()
                scores = engine.score_matrix_batch(batch, mx, 12, 1, mode=mode, band=band)
                assert st["blocks"] == 1 and st["mode"] == 10 and engine.last_stats()["blocks"] == 1
                for k, (p, g, s) in enumerate(zip(batch, got, scores)):
                    alone = engine.align_matrix_batch([p], mx, 12, 1, mode=mode, band=band)[0]
                    w = engine.align_matrix_batch([p], mx, 12, 1, cpu=True, mode=mode, band=band)[0]
                    assert g == alone == w and s == w.score, (mode, band, k, len(p[0]), len(p[1]), g, alone, w, s)


# ---- 4. a band that holds the whole matrix ------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_whole_matrix_band(engine, table, mode):
    rng = np.random.default_rng(72)                        # the _mode tests' traced grid
    pairs = []
    for n in (1, 511, 512, 513, 1024, 1025, 1100):
        for m in (1, 64, 65, 300, 700):
            a = rand_seq(rng, n)
            pairs += [(a, rand_seq(rng, m)), (a, mutated_copy(rng, a[max(0, n - m - 5):], m))]
    for gaps in ((12, 1), (0, 0)):
        with engine.Matrix(SYMBOLS, table) as mx:
            want = engine.align_matrix_batch(pairs, mx, *gaps, mode=mode)
            assert engine.last_stats()["mode"] == 7
            want_scores = engine.score_matrix_batch(pairs, mx, *gaps, mode=mode)
            for band in (1100, 5000):                       # max(n, m) over the batch, and beyond
                got = engine.align_matrix_batch(pairs, mx, *gaps, mode=mode, band=band)
                st = engine.last_stats()
                assert st["mode"] == 10 and st["cells"] == sum(len(a) * len(b) for a, b in pairs)
                assert got == want, (mode, gaps, band)
                assert engine.score_matrix_batch(pairs, mx, *gaps, mode=mode, band=band) == want_scores
                assert engine.last_stats()["mode"] == 9
            for (a, b), w in list(zip(pairs, want))[::7]:   # B = max(n, m) of the pair itself
                assert engine.align_matrix_batch([(a, b)], mx, *gaps, mode=mode, band=max(len(a), len(b))) == [w]


# ---- 5. ties and low complexity -----------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("band", [0, 3, 100])
def test_ties_and_low_complexity(engine, table, mode, band):
    pairs = list(low_complexity_pairs())
    for n, m in ((600, 600), (520, 700), (700, 520), (1, 40), (64, 1)):
        pairs.append((np.full(n, SYMBOLS[0], np.uint8), np.full(m, SYMBOLS[0], np.uint8)))
        pairs.append((np.full(n, SYMBOLS[3], np.uint8), np.full(m, SYMBOLS[5], np.uint8)))
    for gaps in ((12, 1), (0, 0), (3, 1)):
        both(engine, "low", pairs, table, *gaps, mode, band)


# ---- 6. refused whole, aligned banded ------------------------------------------------------------------------

@pytest.mark.gpu
def test_refused_whole_aligned_banded(engine, request, table):
    request.addfinalizer(lambda: engine.set_option("trace_mb", 1024))
    engine.set_option("trace_mb", 1)
    rng = np.random.default_rng(176)
    a = rand_seq(rng, 3000, 20)
    pairs = [(a, mutated_copy(rng, a, 3000))]
    p = engine.band_plan(3000, 3000, 50)
    assert p["trace_bytes"] <= (1 << 20) < p["full_trace_bytes"]
    with engine.Matrix(SYMBOLS, table) as mx:
        with pytest.raises(engine.SwError, match="needs .* bytes of trace memory, more than option trace_mb = 1 MiB"):
            engine.align_matrix_batch(pairs, mx, 12, 1, mode="global")
    got = both(engine, "refused", pairs, table, 12, 1, "global", 50)
    assert engine.last_stats()["mode"] == 9 and got[0].score > 300
    with engine.Matrix(SYMBOLS, table) as mx:
        engine.align_matrix_batch(pairs, mx, 12, 1, mode="global", band=50)
        before = engine.last_stats()
        assert before["mode"] == 10 and before["boundary_bytes"] == p["trace_bytes"]
        wide = engine.band_plan(3000, 3000, 1000)
        assert wide["trace_bytes"] > (1 << 20)
        with pytest.raises(engine.SwError, match=r"pair 0: a 3000 x 3000 alignment in a band of 1000 needs %d bytes of trace "
                                                 r"memory, more than option trace_mb = 1 MiB" % wide["trace_bytes"]):
            engine.align_matrix_batch(pairs, mx, 12, 1, mode="global", band=1000)
        assert engine.last_stats() == before                # nothing was launched
        with pytest.raises(engine.SwError, match="sw_score_matrix_batch_band: band -1"):
            engine.score_matrix_batch(pairs, mx, 12, 1, mode="global", band=-1)
        with pytest.raises(engine.SwError, match="sw_align_matrix_batch_band: band -1"):
            engine.align_matrix_batch(pairs, mx, 12, 1, mode="global", band=-1)
        assert engine.last_stats() == before


# ---- 7. penalties one unit inside the score-range bound --------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_penalties_one_unit_inside_the_range_bound(engine, mode):
    """tests/test_matrix_limits.py's construction: penalty u, the largest the mode bound admits for
    the shape, under the 32-symbol table; checked against the float restatement."""
    n, m, band = 513, 65, 20
    u = edge_u(n, m)
    assert (n + m + 1024) * u < (1 << 28) <= (n + m + 1024) * (u + 1)
    rng = np.random.default_rng(3377)
    pairs = (pair32(rng, n, m, False), pair32(rng, n, m, True))
    lowest = 0
    for gaps in ((u, u), (u, 1), (1, u)):
        got = both(engine, "edge", pairs, FULL32, *gaps, mode, band, symbols=SYM32, code=CODE32)
        for (a, b), g in zip(pairs, got):
            score, ei, ej = restate_band(a, b, FULL32, *gaps, mode, band, CODE32)
            assert g.score == score and (mode == "local" and score == 0 or (g.end1, g.end2) == (ei + 1, ej + 1)), (mode, gaps, g)
            lowest = min(lowest, g.score)
    assert lowest < -(1 << 24) or mode != "global"
    if mode != "local":                                     # one unit more: refused, nothing launched
        before = engine.last_stats()
        with engine.Matrix(SYM32, FULL32) as mx:
            with pytest.raises(engine.SwError, match="pair 0: score range exceeds the int32 engine in this mode"):
                engine.score_matrix_batch(pairs, mx, u + 1, 1, mode=mode, band=band)
            with pytest.raises(engine.SwError, match="pair 0: score range exceeds the int32 engine in this mode"):
                engine.align_matrix_batch(pairs, mx, u + 1, 1, mode=mode, band=band)
        assert engine.last_stats() == before

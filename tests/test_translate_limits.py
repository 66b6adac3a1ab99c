"""GPU: the translated kernels (csrc/sw_matrix.hip XLATE: score-only W = 1/2/4/8 and the traced one; local,
global, semi-global) at the limits of the domain include/algoGPU.h declares, where tests/test_translate.py
does not run them.  Every comparison is bit-exact, and the reference is independent of the GPU matrix path and
of the library's `translate`: `check_many` (local) and `restate` (the modes) over `py_translate(dna, frame,
code)`, shown to hold at these limits, without a GPU, in tests/test_translate_limits_cpu.py, which also
defines the shared inputs.  Alignments go against that reference and the library's CPU aligner.

A. FULL32 under CODE_ALL32, a code that emits all 32 symbols (row 31 of the table through codons 0 and 63),
   CODE_STRANGE under `other` = 31 and a matrix without 'X' under `other` = 30; B. `any_dna`: every byte value,
   scores, alignments and their DNA ranges; C. global and semi-global with gap penalties one unit inside the
   mode bound; D. local at gap penalties of 2^20; E. the claim loop: one or two workgroups, a wave alternating
   plus and minus frames of different m over one scratch column, and a trace launch split by trace_mb; F. a DNA
   database with records of 0..5 bases.

What these tests were seen to notice on an MI355X, each in a build with that one defect, which the 28 tests of
tests/test_translate.py all pass: a composed codon table that ignores `other` (row 0 for a code byte or an 'X'
that only `other` covers: the six tests of CODE_STRANGE and of the matrix without 'X', and, without a GPU,
test_composed_tables of tests/test_translate_limits_cpu.py); `xl_row_code` indexing the base map with seven
bits of the byte (0xc1 reads as 'A': the same six, B in the three modes and F, whose records hold such
bytes).  The kernels as they are pass everything here."""
import numpy as np
import pytest

from test_matrix import check_many
from test_matrix_limits import force
from test_matrix_limits_cpu import BIG_GAPS, FULL32, LAST, SYM32, edge_u, rand32
from test_translate_cpu import FRAMES, planted_dna
from test_translate_limits_cpu import (CODE_ALL32, EDGE_CASES, RANGE_MESSAGE, SETTINGS, SYM31, FULL31, CODE_STRANGE, against_the_reference,
                                       any_dna, cached, dense_dna, edge_gaps, edge_pairs, frames_of, ref_scores, reference, setting)

MODES = ("local", "global", "semiglobal")
AM = {"local": 0, "global": 1, "semiglobal": 2}
XLATE_MODE, XLATE_TRACE_MODE = 15, 16       # sw_last_stats
W_ALL = (1, 2, 4, 8)


def scores_at(engine, request, pairs, name, gaps, mode, ref, widths=W_ALL):
    """The score-only kernel, six frames a pair, at every forced W against the reference."""
    sym, T, other, code, code_str, rows = setting(name)
    want = ref_scores(ref)
    with engine.Matrix(sym, T, other=other) as mx:
        for W in widths:
            force(engine, request, W=W)
            got = engine.score_matrix_translated_batch(pairs, mx, *gaps, mode=mode, code=code)
            st = engine.last_stats()
            assert (st["mode"], st["variant"]) == (XLATE_MODE, AM[mode]) and (st["W"] == W or (W == 0 and st["W"] in W_ALL))
            assert got.shape == want.shape
            bad = [(k, FRAMES[f], len(pairs[k][0]), len(pairs[k][1]), int(got[k, f]), int(want[k, f])) for k, f in np.argwhere(got != want)]
            assert not bad, (name, mode, gaps, W, len(bad), bad[:8])
    engine.set_option("W", 0)


def alignments_at(engine, pairs, name, gaps, mode, ref):
    """The traced kernel and the walk in all six frames of every pair: the reference (score; in a mode the whole
    alignment), the CPU aligner's alignment, re-scored, the DNA range translated again."""
    sym, T, other, code, code_str, rows = setting(name)
    flat = [p for p in pairs for _ in FRAMES]
    frames = list(FRAMES) * len(pairs)
    with engine.Matrix(sym, T, other=other) as mx:
        cpu = engine.align_matrix_translated_batch(flat, frames, mx, *gaps, cpu=True, mode=mode, code=code)
        got = engine.align_matrix_translated_batch(flat, frames, mx, *gaps, mode=mode, code=code)
        st = engine.last_stats()
    assert (st["mode"], st["W"], st["variant"] >> 28) == (XLATE_TRACE_MODE, 8, AM[mode])
    assert got == cpu, [(k // 6, FRAMES[k % 6], g, c) for k, (g, c) in enumerate(zip(got, cpu)) if g != c][:4]
    against_the_reference(engine, pairs, name, gaps, mode, ref, got=got)
    return got


# ---- A. FULL32 with a code that emits every symbol -----------------------------------------------------------

QUERY_LENGTHS = (1, 64, 65, 513, 1025)
DNA_LENGTHS = (3, 5, 191, 193, 195, 905, 3302)
GRID_GAPS = (25, 3)


def grid():
    """(protein, dna) for every query length x DNA length: half dense random DNA, half a mutated copy of the query
    planted under CODE_ALL32 in a random frame and strand; every query holds the last symbol."""
    def make():
        rng = np.random.default_rng(6400)
        pairs = []
        for i, n in enumerate(QUERY_LENGTHS):
            q = rand32(rng, n)
            q[int(rng.integers(0, n))] = LAST
            for j, L in enumerate(DNA_LENGTHS):
                pairs.append((q, planted_dna(rng, q, L, CODE_ALL32.decode("latin-1")) if (i + j) % 2 else dense_dna(rng, L)))
        return pairs
    return cached("xgrid", make)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W", [0, 1, 2, 4, 8])
def test_every_symbol_scores(engine, request, W, mode):
    pairs = grid()
    ref = reference("xgrid", pairs, "all32", GRID_GAPS, mode)
    scores_at(engine, request, pairs, "all32", GRID_GAPS, mode, ref, widths=(W,))
    want = ref_scores(ref)
    # row 31 is used: the frames hold the last symbol, and the answer changes when its row and column are zeroed
    assert all(any((fr == LAST).any() for fr in frames_of(d, CODE_ALL32.decode("latin-1"))) for _, d in pairs if len(d) > 190)
    if mode == "local":
        def zeroed():
            T = FULL32.copy()
            T[31, :] = T[:, 31] = 0
            flat = [(q, fr) for q, d in pairs for fr in frames_of(d, CODE_ALL32.decode("latin-1"))]
            return np.array(check_many(flat, T, *GRID_GAPS, setting("all32")[5])).reshape(-1, 6)
        assert (cached("xgrid-zeroed", zeroed) != want).sum() > 20
        assert want.max() > 20000 and (want[:, 3:].max(axis=1) > want[:, :3].max(axis=1) + 500).any()   # a minus-frame hit


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_every_symbol_alignments(engine, mode):
    pairs = [p for p in grid() if len(p[0]) in (1, 65, 513)]
    ref = tuple(r for p, r in zip(grid(), reference("xgrid", grid(), "all32", GRID_GAPS, mode)) if len(p[0]) in (1, 65, 513))
    got = alignments_at(engine, pairs, "all32", GRID_GAPS, mode, ref)
    assert sum(1 for g in got if g.frame < 0 and g.score > 2000) >= 2 and sum(1 for g in got if len(g.ops) > 2) > 5


def strange_pairs(name):
    def make():
        rng = np.random.default_rng(6410)
        sym = np.frombuffer(SETTINGS[name][0], np.uint8)
        code_str = SETTINGS[name][3].decode("latin-1")
        pairs = []
        for n, L in ((65, 193), (513, 905), (300, 1500), (1, 700)):
            q = sym[rng.integers(0, len(sym), n)]
            q[int(rng.integers(0, n))] = sym[-1]
            pairs.append((q, planted_dna(rng, q, L, code_str)))
            pairs.append((q, any_dna(rng, max(L, 600))))
        return pairs
    return cached(("xstrange", name), make)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["strange", "no_x"])
def test_what_only_other_covers_lands_on_the_last_row(engine, request, name, mode):
    """strange: the code emits 0x00, 0xff and '*', which the alphabet lacks, under other = 31; no_x: a 31-symbol
    matrix without 'X' under other = 30, so every ambiguous codon of any_dna reads the last row."""
    pairs = strange_pairs(name)
    ref = reference(("xstrange", name), pairs, name, GRID_GAPS, mode)
    scores_at(engine, request, pairs, name, GRID_GAPS, mode, ref, widths=(0, 1, 8))
    alignments_at(engine, pairs, name, GRID_GAPS, mode, ref)
    sym, T, other, code, code_str, rows = setting(name)
    strangers = sum(int((rows[fr] == other).sum()) for _, d in pairs for fr in frames_of(d, code_str))
    assert strangers > 300


@pytest.mark.gpu
def test_refusals_without_other(engine):
    q, d = rand32(np.random.default_rng(1), 30), dense_dna(np.random.default_rng(2), 200)
    with engine.Database.from_records([("r", d)]) as db:
        before = engine.last_stats()
        for sym, T, code, byte in ((SYM32, FULL32, CODE_STRANGE, "0x00"), (SYM31, FULL31, CODE_ALL32, "0x58")):
            with engine.Matrix(sym, T) as mx:
                qq = q[q != ord("X")]
                with pytest.raises(engine.SwError, match="sw_score_matrix_translated_batch: the genetic code emits byte " + byte):
                    engine.score_matrix_translated(qq, d, mx, 12, 1, code=code)
                with pytest.raises(engine.SwError, match="sw_align_matrix_translated_batch: the genetic code emits byte " + byte):
                    engine.align_matrix_translated(qq, d, -2, mx, 12, 1, code=code)
                with pytest.raises(engine.SwError, match="sw_db_search_matrix_translated: the genetic code emits byte " + byte):
                    db.search_translated(qq, mx, 12, 1, code=code)
    assert engine.last_stats() == before


# ---- B. any_dna: every byte value ------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_any_byte_is_a_dna_byte(engine, request, mode):
    def make():
        rng = np.random.default_rng(6420)
        pairs = []
        for n, L in ((40, 600), (65, 601), (300, 905), (513, 1502), (1025, 3302), (1, 3001)):
            q = rand32(rng, n)
            d = any_dna(rng, L)
            assert sorted(set(d.tolist())) == list(range(256))
            pairs.append((q, d))
        return pairs
    pairs = cached("xany", make)
    ref = reference("xany", pairs, "all32", (12, 1), mode)
    scores_at(engine, request, pairs, "all32", (12, 1), mode, ref, widths=(0, 1, 2, 4, 8))
    alignments_at(engine, pairs, "all32", (12, 1), mode, ref)       # with dna_beg / dna_end translated again
    assert ref_scores(reference("xany", pairs, "all32", (12, 1), mode)).max() > 500


# ---- C. gap penalties one unit inside the mode bound ----------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["global", "semiglobal"])
@pytest.mark.parametrize("case", EDGE_CASES, ids=lambda c: "%dx%d-L%d" % c)
def test_gaps_one_unit_inside_the_mode_bound(engine, request, case, mode):
    n, m, L = case                                          # L = 3m: u is taken at the larger m, frame +1's
    u = edge_u(n, m)
    assert (n + m + 1024) * u < (1 << 28) <= (n + m + 1024) * (u + 1)
    pairs = edge_pairs(case)
    assert [(len(q), len(d)) for q, d in pairs] == [(n, L)]
    lowest = 0
    for gaps in edge_gaps(n, m):
        ref = reference(("edge", case), pairs, "all32", gaps, mode)
        scores_at(engine, request, pairs, "all32", gaps, mode, ref)
        alignments_at(engine, pairs, "all32", gaps, mode, ref)
        if gaps == (u, u):
            lowest = ref_scores(ref).min()
    assert lowest < -(1 << 24) or mode == "semiglobal"
    # one unit more: refused before any launch
    before = engine.last_stats()
    with engine.Matrix(SYM32, FULL32) as mx:
        for gaps in ((u + 1, u + 1), (u + 1, 1), (0, u + 1)):
            with pytest.raises(engine.SwError, match="sw_score_matrix_translated_batch: " + RANGE_MESSAGE):
                engine.score_matrix_translated_batch(pairs, mx, *gaps, mode=mode, code=CODE_ALL32)
            with pytest.raises(engine.SwError, match="sw_align_matrix_translated_batch: " + RANGE_MESSAGE):
                engine.align_matrix_translated_batch(pairs, [-1], mx, *gaps, mode=mode, code=CODE_ALL32)
    assert engine.last_stats() == before


# ---- D. local at gap penalties of 2^20 --------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("gaps", BIG_GAPS)
def test_local_at_large_gaps(engine, request, gaps):
    pairs = grid()[::3]
    ref = reference("xgrid/3", pairs, "all32", gaps, "local")
    scores_at(engine, request, pairs, "all32", gaps, "local", ref, widths=(1, 8))
    got = alignments_at(engine, pairs, "all32", gaps, "local", ref)
    assert ref_scores(ref).max() > 3000
    if gaps[0] <= 1:
        assert any(len(x.ops) > 1 for x in got)              # cheap openings are taken, one residue at a time
    else:
        assert all(len(x.ops) <= 1 for x in got)             # no gap is worth 2^20


# ---- E. the claim loop -------------------------------------------------------------------------------------------

def claim_batch():
    """120 DNAs of 3..150 bases and five of 900..3300; queries of 1..48 residues, and 513 and 700 against two of the
    long DNAs; shuffled.  Every pair is six items: with one or two workgroups a wave claims plus and minus frames
    of different m in turn, and its scratch column is reused between them (the queries of 513 and 700 have two or
    more strips at every W)."""
    def make():
        rng = np.random.default_rng(6450)
        code_str = CODE_ALL32.decode("latin-1")
        pairs = []
        for k in range(120):
            q = rand32(rng, int(rng.integers(1, 49)))
            L = int(rng.integers(3, 151))
            pairs.append((q, planted_dna(rng, q, L, code_str) if k % 2 else dense_dna(rng, L)))
        for n, L in ((513, 3300), (700, 2000), (30, 900), (48, 3001), (7, 1502)):
            q = rand32(rng, n)
            pairs.append((q, planted_dna(rng, q, L, code_str)))
        order = rng.permutation(len(pairs))                  # the long ones anywhere in the input
        return [pairs[k] for k in order]
    return cached("xclaim", make)


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_claim_loop_alternates_frames(engine, request, mode, blocks):
    pairs, gaps = claim_batch(), (25, 3)
    ref = reference("xclaim", pairs, "all32", gaps, mode)
    want = ref_scores(ref)
    frames = [FRAMES[k % 6] for k in range(len(pairs))]      # traced: the frames cycle through all six
    picked = [ref[k][k % 6] for k in range(len(pairs))]
    force(engine, request, blocks=blocks, W=0)
    with engine.Matrix(SYM32, FULL32) as mx:
        for W in (0, 1):
            engine.set_option("W", W)
            got = engine.score_matrix_translated_batch(pairs, mx, *gaps, mode=mode, code=CODE_ALL32)
            st = engine.last_stats()
            assert np.array_equal(got, want), (mode, blocks, W, np.argwhere(got != want)[:8])
            assert (st["blocks"], st["mode"], st["variant"]) == (blocks, XLATE_MODE, AM[mode]) and (W == 0 or st["W"] == 1)
            assert st["items"] == 6 * len(pairs)
            back = engine.score_matrix_translated_batch(pairs[::-1], mx, *gaps, mode=mode, code=CODE_ALL32)
            assert np.array_equal(back, want[::-1]), (mode, blocks, W)
        engine.set_option("W", 0)
        cpu = engine.align_matrix_translated_batch(pairs, frames, mx, *gaps, cpu=True, mode=mode, code=CODE_ALL32)
        got = engine.align_matrix_translated_batch(pairs, frames, mx, *gaps, mode=mode, code=CODE_ALL32)
        st = engine.last_stats()
        assert (st["mode"], st["blocks"], st["variant"]) == (XLATE_TRACE_MODE, blocks, (AM[mode] << 28) + 1)
        assert got == cpu
        assert engine.align_matrix_translated_batch(pairs[::-1], frames[::-1], mx, *gaps, mode=mode, code=CODE_ALL32) == cpu[::-1]
    for g, w, f in zip(got, picked, frames):
        assert g.frame == f and g.score == (w[0] if isinstance(w, tuple) else w)
        assert mode == "local" or (g.score, g.beg1, g.end1, g.beg2, g.end2, g.ops) == w
    assert want.max() > 5000 and (mode == "local" or want.min() < 0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_a_split_trace_launch_answers_the_same(engine, request, mode):
    pairs, gaps = claim_batch(), (25, 3)
    ref = reference("xclaim", pairs, "all32", gaps, mode)
    flat = [p for p in pairs for _ in FRAMES]
    frames = list(FRAMES) * len(pairs)
    force(engine, request, blocks=0, trace_mb=1)
    with engine.Matrix(SYM32, FULL32) as mx:
        cpu = engine.align_matrix_translated_batch(flat, frames, mx, *gaps, cpu=True, mode=mode, code=CODE_ALL32)
        got = engine.align_matrix_translated_batch(flat, frames, mx, *gaps, mode=mode, code=CODE_ALL32)
        st = engine.last_stats()
        assert st["mode"] == XLATE_TRACE_MODE and st["variant"] >> 28 == AM[mode] and st["variant"] & 0xFFFFFFF > 1
        assert got == cpu
        assert engine.align_matrix_translated_batch(flat[::-1], frames[::-1], mx, *gaps, mode=mode, code=CODE_ALL32) == cpu[::-1]
    assert [g.score for g in got] == ref_scores(ref).reshape(-1).tolist()


# ---- F. a DNA database ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dna_db():
    """Records of 0..5 bases beside long ones; the query of 150 residues planted in three.  Two records hold every
    byte value a FASTA record can: any_dna without the blanks and line ends the parser drops and without '>'."""
    rng = np.random.default_rng(6460)
    code_str = CODE_ALL32.decode("latin-1")
    q = rand32(rng, 150)
    q[7] = LAST
    lens = [0, 1, 2, 3, 4, 5] + [int(x) for x in rng.integers(60, 2001, 18)]
    recs = [dense_dna(rng, L) for L in lens]
    for i, L in ((8, 800), (9, 1501)):
        d = any_dna(rng, L)
        d[np.isin(d, np.frombuffer(b" \t\r\v\f\n>", np.uint8))] = ord("N")
        recs[i] = d
    for i in (10, 15, 20):
        recs[i] = planted_dna(rng, q, len(recs[i]) + 450, code_str)
    recs += [recs[15].copy(), np.zeros(0, np.uint8), dense_dna(rng, 4)]
    return [("rec%d" % i, r) for i, r in enumerate(recs)], q


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_dna_database_edges(engine, dna_db, mode):
    recs, q = dna_db
    pairs = [(q, d) for _, d in recs]
    gaps = (25, 3)
    ref = reference("xdb", pairs, "all32", gaps, mode)
    want = ref_scores(ref)
    with engine.Database.from_records(recs) as db, engine.Matrix(SYM32, FULL32) as mx:
        got = db.search_translated(q, mx, *gaps, mode=mode, code=CODE_ALL32)
        st = engine.last_stats()
        assert st["mode"] == XLATE_MODE and got.shape == (len(recs), 6)
        assert np.array_equal(got, want), np.argwhere(got != want)[:8]
        assert np.array_equal(got, engine.score_matrix_translated_batch(pairs, mx, *gaps, mode=mode, code=CODE_ALL32))
        for i, (_, d) in enumerate(recs):                      # a frame without a residue
            for fi, f in enumerate(FRAMES):
                if len(d) < abs(f) + 2:
                    assert got[i, fi] == (0 if mode == "local" else -(25 + 149 * 3))
        idx = [i for i in range(len(recs)) for _ in FRAMES]
        frs = list(FRAMES) * len(recs)
        al = db.align_translated(q, idx, frs, mx, *gaps, mode=mode, code=CODE_ALL32)
        assert engine.last_stats()["mode"] == XLATE_TRACE_MODE
        assert al == engine.align_matrix_translated_batch([pairs[i] for i in idx], frs, mx, *gaps, mode=mode, code=CODE_ALL32)
        assert al == engine.align_matrix_translated_batch([pairs[i] for i in idx], frs, mx, *gaps, cpu=True, mode=mode, code=CODE_ALL32)
        against_the_reference(engine, pairs, "all32", gaps, mode, ref, got=al)
        top = db.top_translated(q, 8, mx, *gaps, alignments=True, mode=mode, code=CODE_ALL32)
        flat = sorted(((-int(want[i, k]), i, k) for i in range(len(recs)) for k in range(6)))[:8]
        assert [(h[0], h[1], h[2], h[3]) for h in top] == [(-s, i, FRAMES[k], recs[i][0]) for s, i, k in flat]
        assert [h[4] for h in top] == [al[6 * i + k] for _, i, k in flat]
        twins = [h for h in top if h[1] in (15, len(recs) - 3)]   # two equal records: a tie, ranked by index
        assert mode == "global" or (len(twins) >= 2 and twins[0][0] == twins[1][0] and twins[0][1] == 15 and twins[0][2] == twins[1][2])
        assert want.max() > 5000

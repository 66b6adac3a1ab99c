"""GPU: the profile kernels (csrc/sw_matrix.hip PROFILE: score-only W = 1/2/4/8 and the traced one; local,
global, semi-global) at the limits of the domain include/algoGPU.h declares, where tests/test_profile.py does
not run them.  Every comparison is bit-exact.  Scores go against `profile_scores` (tests/test_profile_cpu.py),
alignments against that score, the library's CPU aligner and `rescore_profile`; both yardsticks are shown to
hold at these limits, without a GPU, in tests/test_profile_limits_cpu.py, which also defines the shared inputs.

A. the alphabet: K = 32 (column 31 of a lane's slot and the sentinel at index 32 are live, beside the dead row
   in the last strip), K = 1 and K = 2, `other` = 31 with arbitrary bytes; B. entries over the whole of
   [-127, 127] on low-complexity input, a profile of period 7: ties; C. global and semi-global with gap
   penalties one unit inside the mode bound; D. local at gap penalties of 2^20; E. re-staging: one or two
   workgroups claim 305 sequences of very different lengths, at every W and traced, and a trace launch split
   by trace_mb; F. a K = 32 profile database with empty and 1-residue records.

What these tests were seen to notice on an MI355X, each in a build with that one defect, which the 44 tests of
tests/test_profile.py all pass: a slot stride of 32 bytes in `setup` and `stage_rows`, eight dwords a row copied
(the sentinel at index 32 is the next slot's column 0: every local test over K = 32 -- the scores at every W,
the alignments, `other` = 31, B, D, E at both grid sizes and split, F -- 19 in all, no mode test and no small
alphabet); a MAT_NEG with 2^16 of headroom above -2^31 instead of 2^30 (every case of C with more than one
profile position, nothing else).  The kernels as they are pass everything here."""
import numpy as np
import pytest

from test_matrix_cpu import byte_codes
from test_matrix_limits import force
from test_matrix_limits_cpu import BIG_GAPS, CODE32, LAST, SYM32, edge_u, rand32
from test_modes_cpu import check_shape
from test_profile_cpu import profile_scores, rescore_profile
from test_profile_limits_cpu import (CODE1, CODE2, EDGE_SHAPES, LOW_GAPS, RANGE_MESSAGE, SYM1, SYM2, cached, edge_case, edge_gaps,
                                     edge_want, float_end, full_profile, limit_seqs, low_complexity, scores_ref, small_profile,
                                     small_seqs, uses_last_column)

MODES = ("local", "global", "semiglobal")
AM = {"local": 0, "global": 1, "semiglobal": 2}
PROFILE_MODE, PROFILE_TRACE_MODE = 13, 14      # sw_last_stats
W_ALL = (1, 2, 4, 8)


def scores_at(engine, request, P, seqs, gaps, mode, want, widths=W_ALL, sym=SYM32, **profile_args):
    """The score-only kernel at every forced W against `want`."""
    with engine.Profile(sym, P, **profile_args) as p:
        for W in widths:
            force(engine, request, W=W)
            got = engine.score_profile_batch(p, seqs, *gaps, mode=mode)
            st = engine.last_stats()
            assert (st["mode"], st["variant"]) == (PROFILE_MODE, AM[mode]) and (st["W"] == W or (W == 0 and st["W"] in W_ALL))
            bad = [(k, len(s), g, w) for k, (s, g, w) in enumerate(zip(seqs, got, want)) if g != w]
            assert not bad, (len(P), mode, gaps, W, len(bad), bad[:8])
    engine.set_option("W", 0)


def alignments_at(engine, P, seqs, gaps, mode, want, sym=SYM32, code=CODE32, **profile_args):
    """The traced kernel and the walk: the restatement's score, the CPU aligner's alignment, re-scored."""
    with engine.Profile(sym, P, **profile_args) as p:
        cpu = engine.align_profile_batch(p, seqs, *gaps, cpu=True, mode=mode)
        got = engine.align_profile_batch(p, seqs, *gaps, mode=mode)
        st = engine.last_stats()
    assert (st["mode"], st["W"], st["variant"] >> 28) == (PROFILE_TRACE_MODE, 8, AM[mode]) and len(got) == len(seqs)
    for k, (s, g, c, w) in enumerate(zip(seqs, got, cpu, want)):
        assert g.score == w and g == c, (len(P), mode, gaps, k, len(s), g, c, w)
        assert rescore_profile(g, P, s, *gaps, mode, code) == g.score, (mode, gaps, k)
        if len(s):
            check_shape(g, np.zeros(len(P)), s, mode)
    return got


# ---- A. the alphabet: K = 32 -----------------------------------------------------------------------------

GRID_N = (1, 64, 65, 130, 513, 1025)
GRID_M = (1, 33, 64, 65, 300, 300, 65, 64, 33, 1)          # each length once random, once a mutated copy
GRID_GAPS = [(12, 1), (90, 7)]


def grid32():
    def make():
        rng = np.random.default_rng(5400)
        grid = []
        for n in GRID_N:
            P, cons = full_profile(rng, n)
            grid.append((P, limit_seqs(rng, cons, GRID_M)))
        return grid
    return cached("pgrid32", make)


def grid_ref(k, gaps, mode):
    P, seqs = grid32()[k]
    return scores_ref(("pgrid32", k), P, seqs, gaps, mode)


def grid_uses_column31(k, mode):
    P, seqs = grid32()[k]
    return cached(("pgrid32-31", k, mode), lambda: uses_last_column(P, seqs, (12, 1), mode, grid_ref(k, (12, 1), mode)))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W", [0, 1, 2, 4, 8])
def test_k32_scores(engine, request, W, mode):
    """n = 130 at W = 8 and n = 513 at every W leave most of the last strip on the dead row."""
    for k, (P, seqs) in enumerate(grid32()):
        assert all((s == LAST).any() for s in seqs)
        for gaps in GRID_GAPS:
            scores_at(engine, request, P, seqs, gaps, mode, grid_ref(k, gaps, mode), widths=(W,))
        assert grid_uses_column31(k, mode) or (len(P) == 1 and mode != "local"), (k, mode)
    assert max(grid_ref(5, (12, 1), mode)) > 5000
    assert mode == "local" or min(grid_ref(5, (90, 7), mode)) < -1000


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gaps", GRID_GAPS)
def test_k32_alignments(engine, gaps, mode):
    gapped = 0
    for k, (P, seqs) in enumerate(grid32()):
        got = alignments_at(engine, P, seqs, gaps, mode, grid_ref(k, gaps, mode))
        gapped += sum(any(op != "M" for _, op in x.ops) for x in got)
    assert gapped > 8


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_k32_strangers_go_to_the_last_column(engine, request, mode):
    """other = 31: every byte outside the alphabet reads column 31 of its position's row."""
    rng = np.random.default_rng(5410)
    code = byte_codes(SYM32, 31)
    strangers = 0
    for n in (70, 513):
        P, cons = full_profile(rng, n)
        seqs = limit_seqs(rng, cons, (90, 65, 300, 700, 1, 40))
        for s in seqs:
            at = rng.integers(0, len(s), 1 + len(s) // 9)
            s[at] = rng.integers(0, 256, len(at))                # any byte
            strangers += int((CODE32[s] < 0).sum())
        want = profile_scores(P, [code[s] for s in seqs], 12, 1, mode)
        assert want != profile_scores(P, [byte_codes(SYM32, 30)[s] for s in seqs], 12, 1, mode)
        scores_at(engine, request, P, seqs, (12, 1), mode, want, widths=(0, 1, 8), other=31)
        alignments_at(engine, P, seqs, (12, 1), mode, want, code=code, other=31)
        with engine.Profile(SYM32, P) as p:                       # other = -1: the same bytes are an error
            with pytest.raises(engine.SwError, match=r"sequence 0: position \d+: byte 0x[0-9a-f]{2} is outside the profile alphabet"):
                engine.score_profile_batch(p, seqs, 12, 1, mode=mode)
    assert strangers > 100


# ---- A. the alphabet: K = 1 and K = 2 --------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [1, 2])
def test_small_alphabets(engine, request, k, mode):
    sym, code = ((SYM1, CODE1), (SYM2, CODE2))[k - 1]

    def make():
        rng = np.random.default_rng(5420 + k)
        return [(small_profile(rng, n, k), small_seqs(rng, sym, (1, 33, 65, 300, 1100))) for n in (1, 65, 513, 1025)]
    for i, (P, seqs) in enumerate(cached(("psmall", k), make)):
        for gaps in ((3, 1), (0, 0)):
            want = scores_ref(("psmall", k, i), P, seqs, gaps, mode, code)
            scores_at(engine, request, P, seqs, gaps, mode, want, sym=sym)
            alignments_at(engine, P, seqs, gaps, mode, want, sym=sym, code=code)
            assert mode != "local" or len(P) == 1 or max(want) >= 127 * 4


# ---- B. full-range entries on low-complexity input: ties meet steps of +-127 ------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gaps", LOW_GAPS)
def test_full_range_ties(engine, request, gaps, mode):
    profs, seqs = low_complexity()
    for n, P in profs.items():
        want = scores_ref(("low", n), P, seqs, gaps, mode)
        scores_at(engine, request, P, seqs, gaps, mode, want, widths=(1, 8))
        got = alignments_at(engine, P, seqs, gaps, mode, want)       # equal to the CPU aligner's, ties and all
        if n == 84:
            several = 0
            for x, s in zip(got[:7], seqs):
                score, end1, end2, cand = float_end(P, CODE32[s], *gaps, mode)
                assert (x.score, x.end1, x.end2) == (score, end1, end2), (mode, gaps, len(s))
                several += cand > 1
            assert several >= 1 or mode == "global"


# ---- C. gap penalties one unit inside the mode bound ------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["global", "semiglobal"])
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_gaps_one_unit_inside_the_mode_bound(engine, request, shape, mode):
    n, m = shape
    u = edge_u(n, m)
    assert (n + m + 1024) * u < (1 << 28) <= (n + m + 1024) * (u + 1)
    P, seqs = edge_case(shape)                                # a batch of its own: the gaps are the batch's
    assert len(P) == n and [len(s) for s in seqs] == [m, m]
    lowest = 0
    for gaps in edge_gaps(n, m):
        want = edge_want(shape, gaps, mode)
        scores_at(engine, request, P, seqs, gaps, mode, want)
        alignments_at(engine, P, seqs, gaps, mode, want)
        if gaps == (u, u):
            lowest = min(want)
    assert lowest < -(1 << 24) or mode == "semiglobal"
    # one unit more: refused with the range message, nothing launched
    before = engine.last_stats()
    with engine.Profile(SYM32, P) as p:
        for gaps in ((u + 1, u + 1), (u + 1, 1), (0, u + 1)):
            with pytest.raises(engine.SwError, match=RANGE_MESSAGE):
                engine.score_profile_batch(p, seqs, *gaps, mode=mode)
            with pytest.raises(engine.SwError, match=RANGE_MESSAGE):
                engine.align_profile_batch(p, seqs, *gaps, mode=mode)
    assert engine.last_stats() == before


# ---- D. local at gap penalties of 2^20 --------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("gaps", BIG_GAPS)
def test_local_at_large_gaps(engine, request, gaps):
    best = 0
    for k in (2, 4, 5):                                       # 65, 513 and 1025 positions
        P, seqs = grid32()[k]
        want = grid_ref(k, gaps, "local")
        scores_at(engine, request, P, seqs, gaps, "local", want, widths=(1, 8))
        got = alignments_at(engine, P, seqs, gaps, "local", want)
        best = max(best, max(want))
        if gaps[0] <= 1:
            assert any(len(x.ops) > 1 for x in got) or k == 2   # cheap openings are taken, one residue at a time
        else:
            assert all(len(x.ops) <= 1 for x in got)            # no gap is worth 2^20
    assert best > 3000


# ---- E. re-staging: the claim loop and launch splitting ----------------------------------------------------

def claim_batch():
    """One profile of 700 positions (11 strips at W = 1, 2 when traced) and 305 sequences, 300 of 1..48 residues
    and five of 300..1100, shuffled: with one or two workgroups a wave claims many sequences, copies its slab
    again before every strip of every one, and reuses its scratch column between sequences of different m."""
    def make():
        rng = np.random.default_rng(5450)
        P, cons = full_profile(rng, 700)
        lengths = [int(x) for x in rng.integers(1, 49, 300)] + [1100, 300, 640, 513, 901]
        seqs = limit_seqs(rng, cons, lengths)
        for k in range(0, 300, 4):                             # some short ones copy a window further inside
            at = int(rng.integers(0, 650))
            seqs[k] = np.ascontiguousarray(cons[at:at + lengths[k]])
        order = rng.permutation(len(seqs))                     # the long ones anywhere in the input
        return P, [seqs[k] for k in order]
    return cached("pclaim", make)


def claim_ref(mode, gaps=(12, 1)):
    """profile_scores of the short and of the long sequences apart (less padding)."""
    def make():
        P, seqs = claim_batch()
        out = [0] * len(seqs)
        for pick in ([k for k, s in enumerate(seqs) if len(s) < 100], [k for k, s in enumerate(seqs) if len(s) >= 100]):
            for k, w in zip(pick, profile_scores(P, [CODE32[seqs[k]] for k in pick], *gaps, mode)):
                out[k] = w
        return tuple(out)
    return cached(("pclaim-ref", mode, gaps), make)


def claim_cpu(engine, mode, gaps=(12, 1)):
    def make():
        P, seqs = claim_batch()
        with engine.Profile(SYM32, P) as p:
            return tuple(engine.align_profile_batch(p, seqs, *gaps, cpu=True, mode=mode))
    return cached(("pclaim-cpu", mode, gaps), make)


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_restaging_in_the_claim_loop(engine, request, mode, blocks):
    (P, seqs), gaps = claim_batch(), (12, 1)
    want = list(claim_ref(mode))
    cpu = list(claim_cpu(engine, mode))
    assert [x.score for x in cpu] == want and len(seqs) == 305
    force(engine, request, blocks=blocks, W=0)
    with engine.Profile(SYM32, P) as p:
        for W in (0, 1, 2, 4, 8):
            engine.set_option("W", W)
            assert engine.score_profile_batch(p, seqs, *gaps, mode=mode) == want, (mode, blocks, W)
            st = engine.last_stats()
            assert (st["blocks"], st["items"], st["mode"], st["variant"]) == (blocks, len(seqs), PROFILE_MODE, AM[mode])
            assert W == 0 or st["W"] == W
            assert engine.score_profile_batch(p, seqs[::-1], *gaps, mode=mode) == want[::-1], (mode, blocks, W)
        engine.set_option("W", 0)
        got = engine.align_profile_batch(p, seqs, *gaps, mode=mode)
        st = engine.last_stats()
        assert (st["mode"], st["blocks"], st["variant"]) == (PROFILE_TRACE_MODE, blocks, (AM[mode] << 28) + 1)
        assert got == cpu
        assert engine.align_profile_batch(p, seqs[::-1], *gaps, mode=mode) == cpu[::-1]
    for s, x in zip(seqs, got):
        assert rescore_profile(x, P, s, *gaps, mode, CODE32) == x.score
        check_shape(x, np.zeros(len(P)), s, mode)
    assert max(want) > 5000 and (mode == "local" or min(want) < 0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_a_split_trace_launch_answers_the_same(engine, request, mode):
    (P, seqs), gaps = claim_batch(), (12, 1)
    cpu = list(claim_cpu(engine, mode))
    assert [x.score for x in cpu] == list(claim_ref(mode))
    force(engine, request, blocks=0, trace_mb=1)
    with engine.Profile(SYM32, P) as p:
        assert engine.align_profile_batch(p, seqs, *gaps, mode=mode) == cpu
        st = engine.last_stats()
        assert st["mode"] == PROFILE_TRACE_MODE and st["variant"] >> 28 == AM[mode] and st["variant"] & 0xFFFFFFF > 1
        assert engine.align_profile_batch(p, seqs[::-1], *gaps, mode=mode) == cpu[::-1]


# ---- F. a K = 32 profile database ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def edge_db():
    """A profile of 600 positions and 40 records: empty ones, 1-residue ones, the consensus itself, a record that
    holds 400 positions of it, mutated copies, random ones."""
    rng = np.random.default_rng(5460)
    P, cons = full_profile(rng, 600)
    recs = []
    for i in range(40):
        if i % 9 == 0:
            r = np.zeros(0, np.uint8)
        elif i % 9 == 1:
            r = rand32(rng, 1)
        else:
            r = limit_seqs(rng, cons, [1, int(rng.integers(2, 700))])[i % 2]
        recs.append(("rec%d" % i, r))
    recs[5] = ("rec5", cons.copy())
    recs[14] = ("rec14", np.concatenate([rand32(rng, 40), cons[100:500], rand32(rng, 60)]))
    return P, cons, recs


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_profile_database_edges(engine, edge_db, mode):
    P, cons, recs = edge_db
    seqs = [r for _, r in recs]
    lens = [len(r) for r in seqs]
    n = len(P)
    assert lens.count(0) == 5 and lens.count(1) >= 4
    with engine.Database.from_records(recs) as db, engine.Profile(SYM32, P) as p:
        for go, ge in ((90, 7), (3, 7)):
            gx = min(go, ge)
            want = scores_ref("pdb", P, seqs, (go, ge), mode)
            cpu = engine.align_profile_batch(p, seqs, go, ge, cpu=True, mode=mode)
            assert [x.score for x in cpu] == list(want)
            scores = db.search_profile(p, go, ge, mode=mode)
            st = engine.last_stats()
            assert (st["mode"], st["items"]) == (PROFILE_MODE, 40)
            assert scores.tolist() == list(want), mode
            # the empty cases, as tests/test_modes_cpu.py::test_empty_sequences states them (the profile is seq1)
            for i, L in enumerate(lens):
                if L == 0:
                    assert scores[i] == (0 if mode == "local" else -(go + (n - 1) * gx))
            idx = list(range(40)) + [0, 0, 5, 1, 1, 9]
            got = db.align_profile(p, idx, go, ge, mode=mode)
            assert engine.last_stats()["mode"] == PROFILE_TRACE_MODE
            assert got == [cpu[i] for i in idx], mode
            for i, x in zip(idx, got):
                assert rescore_profile(x, P, seqs[i], go, ge, mode, CODE32) == x.score
                if lens[i]:
                    check_shape(x, np.zeros(n), seqs[i], mode)
                elif mode == "local":
                    assert x.ops == ()
                else:
                    assert (x.beg1, x.end1, x.beg2, x.end2, x.ops) == (0, n, 0, 0, ((n, "I"),))
            order = sorted(range(40), key=lambda i: (-int(scores[i]), i))[:9]
            top = db.top_profile(p, 9, go, ge, alignments=True, mode=mode)
            assert [t[:3] for t in top] == [(int(scores[i]), i, "rec%d" % i) for i in order]
            assert [t[3] for t in top] == [cpu[i] for i in order]
            # the consensus itself: at least its straight score (a detour round a zero row may still pay), the best hit
            assert got[5].score >= int(P[np.arange(n), CODE32[cons]].sum()) and (got[5].beg1, got[5].end1) == (0, n) and order[0] == 5
            assert (min(scores) < 0 or mode == "local") and max(scores) > 20000
            if mode != "global" and go == 90:                  # the record that holds 400 positions of the consensus
                assert got[14].score > 10000 and any(op == "M" and k > 100 for k, op in got[14].ops)

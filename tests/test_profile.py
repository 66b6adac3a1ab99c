"""GPU: position-specific scoring (include/algoGPU.h sw_*_profile_*; csrc/sw_matrix.hip PROFILE): the
profile kernels at 1, 2, 4 and 8 columns a lane and the traced one, in the three modes, bit-exact against

* the matrix path, for profiles that are rows of a table (Profile.from_matrix);
* `profile_scores` of tests/test_profile_cpu.py, the plain numpy restatement of the recurrence with
  s(i, j) = P[i][code(b_j)], for profiles whose score depends on the position;
* the library's CPU aligner (cpu=True), for the alignments.

Profiles are those of test_profile_cpu.random_profile: per position one favoured symbol scoring 4 to 11,
the others -4 to 3, a tenth of the positions masked (all zero) and a tenth tripled; sequences are half
random and half mutated copies of the consensus."""
import numpy as np
import pytest

from test_matrix_cpu import byte_codes, identity_table, random_table
from test_matrix import CODE, SYMBOLS, mutated_copy, rand_seq
from test_align_cpu import low_complexity_pairs
from test_modes_cpu import check_shape
from test_profile_cpu import profile_scores, profile_seqs, random_profile, rescore_profile

MODES = ("local", "global", "semiglobal")
N_EDGES = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1025)   # every strip edge of W = 1, 2, 4, 8
M_EDGES = (1, 2, 31, 32, 33, 63, 64, 65, 130, 300)                              # every chunk edge
GAPS = [(12, 1), (3, 1), (0, 0), (1, 3)]
W_ALL = (1, 2, 4, 8)
PROFILE_MODE, PROFILE_TRACE_MODE = 13, 14      # sw_last_stats


def force_w(engine, request, W):
    request.addfinalizer(lambda: engine.set_option("W", 0))
    engine.set_option("W", W)


# ---- 1. identity with the matrix path -------------------------------------------------------------------

@pytest.fixture(scope="module")
def table():
    T = random_table(np.random.default_rng(24), 24)
    T[3, :] += 2          # asymmetric: the profile is the table's first index
    return T


@pytest.fixture(scope="module")
def matrix_grid():
    """Per profile length a query and ten sequences, half random, half mutated copies of the query."""
    rng = np.random.default_rng(101)
    grid = []
    for n in N_EDGES:
        a = rand_seq(rng, n)
        grid.append((a, profile_seqs(rng, a, M_EDGES)))
    return grid


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W", W_ALL)
def test_from_matrix_equals_the_matrix_path(engine, request, table, matrix_grid, W, mode):
    force_w(engine, request, W)
    with engine.Matrix(SYMBOLS, table) as mx:
        for a, seqs in matrix_grid:
            want = engine.score_matrix_batch([(a, s) for s in seqs], mx, 12, 1, mode=mode)
            assert engine.last_stats()["mode"] == 6
            with engine.Profile.from_matrix(mx, a) as p:
                got = engine.score_profile_batch(p, seqs, 12, 1, mode=mode)
            st = engine.last_stats()
            assert (st["W"], st["mode"], st["variant"]) == (W, PROFILE_MODE, MODES.index(mode)), st
            assert got == want, (len(a), W, mode)


# ---- 2. position-specific profiles ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def profile_grid():
    rng = np.random.default_rng(102)
    grid = []
    for n in N_EDGES:
        P, cons = random_profile(rng, n)
        grid.append((P, cons, profile_seqs(rng, cons, M_EDGES)))
    return grid


@pytest.fixture(scope="module")
def grid_reference(profile_grid):
    """profile_scores of every grid profile against its ten sequences, computed once per (gaps, mode)."""
    cache = {}

    def ref(k, gaps, mode, flat=False):
        key = (k, gaps, mode, flat)
        if key not in cache:
            P, cons, seqs = profile_grid[k]
            if flat:   # the consensus under one identity-like table: what a kernel that ignored the position would score
                P = identity_table(24, 5, -2)[CODE[cons]]
            cache[key] = profile_scores(P, [CODE[s] for s in seqs], *gaps, mode)
        return cache[key]
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W", W_ALL)
def test_position_specific_scores(engine, request, profile_grid, grid_reference, W, mode):
    """A third of the grid per W (cell c of the 14 x 10 grid goes to the W's with index c mod 3)."""
    force_w(engine, request, W)
    third = W_ALL.index(W) % 3
    differ = 0
    for k, (P, cons, seqs) in enumerate(profile_grid):
        pick = [j for j in range(len(seqs)) if (k * len(seqs) + j) % 3 == third]
        with engine.Profile(SYMBOLS, P) as p:
            for gaps in GAPS:
                want = grid_reference(k, gaps, mode)
                got = engine.score_profile_batch(p, [seqs[j] for j in pick], *gaps, mode=mode)
                st = engine.last_stats()
                assert (st["W"], st["mode"]) == (W, PROFILE_MODE)
                assert got == [want[j] for j in pick], (len(P), W, mode, gaps)
        differ += grid_reference(k, (12, 1), mode, flat=True) != grid_reference(k, (12, 1), mode)
    assert differ == len(profile_grid)     # every profile of the grid, the one of a single position included


# ---- 3. traced ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def traced_grid():
    rng = np.random.default_rng(103)
    grid = []
    for n in (1, 511, 512, 513, 1025):
        P, cons = random_profile(rng, n)
        grid.append((P, cons, profile_seqs(rng, cons, (1, 63, 64, 65, 300))))
    return grid


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gaps", [(12, 1), (0, 0), (1, 3)])
def test_traced_equals_the_cpu_aligner(engine, table, traced_grid, gaps, mode):
    gapped = 0
    for P, cons, seqs in traced_grid:
        want = profile_scores(P, [CODE[s] for s in seqs], *gaps, mode)
        with engine.Profile(SYMBOLS, P) as p:
            cpu = engine.align_profile_batch(p, seqs, *gaps, cpu=True, mode=mode)
            got = engine.align_profile_batch(p, seqs, *gaps, mode=mode)
            st = engine.last_stats()
            assert (st["W"], st["mode"], st["variant"] >> 28) == (8, PROFILE_TRACE_MODE, MODES.index(mode)), st
        assert got == cpu, (len(P), mode, gaps)                # score, ranges and operations
        assert [x.score for x in got] == want
        for x, s in zip(got, seqs):
            assert rescore_profile(x, P, s, *gaps, mode) == x.score
            check_shape(x, np.zeros(len(P)), s, mode)
            gapped += any(op != "M" for _, op in x.ops)
    assert gapped > 3
    # many equally good alignments: the tie rules are the matrix path's
    with engine.Matrix(SYMBOLS, table) as mx:
        for a, b in low_complexity_pairs():
            with engine.Profile.from_matrix(mx, a) as p:
                got = engine.align_profile(p, b, *gaps, mode=mode)
                assert got == engine.align_profile(p, b, *gaps, cpu=True, mode=mode)
            assert got == engine.align_matrix(a, b, mx, *gaps, cpu=True, mode=mode)


# ---- 4. re-staging between items and strips ------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_one_workgroup_restages_every_strip(engine, request, mode):
    """One workgroup, W = 1, 130 positions: four waves claim ten sequences each, three strips a sequence, and
    copy their slabs again before every strip."""
    def restore():
        engine.set_option("blocks", 0)
        engine.set_option("W", 0)
    request.addfinalizer(restore)
    rng = np.random.default_rng(104)
    P, cons = random_profile(rng, 130)
    lengths = [1, 400, 2, 399, 64, 65] + [int(x) for x in rng.integers(1, 401, 34)]
    seqs = profile_seqs(rng, cons, lengths)
    want = profile_scores(P, [CODE[s] for s in seqs], 12, 1, mode)
    with engine.Profile(SYMBOLS, P) as p:
        wide = engine.score_profile_batch(p, seqs, 12, 1, mode=mode)
        engine.set_option("blocks", 1)
        engine.set_option("W", 1)
        one = engine.score_profile_batch(p, seqs, 12, 1, mode=mode)
        st = engine.last_stats()
        assert (st["blocks"], st["W"], st["mode"]) == (1, 1, PROFILE_MODE)
    assert one == wide == want


# ---- 5. never swapped ----------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["local", "semiglobal"])
def test_the_profile_is_never_swapped(engine, mode):
    """A short profile against long sequences and a long one against short sequences: the matrix path would
    lay the shorter side across the lanes in local mode; a profile always lies across the lanes."""
    rng = np.random.default_rng(105)
    for n, m in ((40, 900), (900, 40)):
        P, cons = random_profile(rng, n)
        assert len({tuple(r) for r in P}) > 0.7 * n            # the rows differ from one another: a swap would show
        seqs = profile_seqs(rng, np.concatenate([rand_seq(rng, m // 3), cons]) if n < m else cons[300:], [m] * 6)
        want = profile_scores(P, [CODE[s] for s in seqs], 5, 1, mode)
        with engine.Profile(SYMBOLS, P) as p:
            assert engine.score_profile_batch(p, seqs, 5, 1, mode=mode) == want
            assert engine.last_stats()["mode"] == PROFILE_MODE
            assert [x.score for x in engine.align_profile_batch(p, seqs, 5, 1, mode=mode)] == want
        if mode == "local" or n < m:      # (900 positions end to end inside 40 residues are mostly one gap run)
            assert max(want) > 40
        else:
            assert max(want) < 0


# ---- 6. the alphabet -------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_other_and_fold_case(engine):
    rng = np.random.default_rng(106)
    P, cons = random_profile(rng, 90)
    seqs = profile_seqs(rng, cons, (50, 90, 120, 7))
    odd = []
    for s in seqs:
        s = s.copy()
        s[::5] += 32                                          # lower case
        s[3::11] = ord("@")                                   # outside the alphabet
        odd.append(s)
    for other, fold in ((23, True), (23, False), (5, True)):
        code = byte_codes(SYMBOLS, other, fold)
        with engine.Profile(SYMBOLS, P, other=other, fold_case=fold) as p:
            for mode in MODES:
                want = profile_scores(P, [code[s] for s in odd], 3, 1, mode)
                assert engine.score_profile_batch(p, odd, 3, 1, mode=mode) == want
                assert [x.score for x in engine.align_profile_batch(p, odd, 3, 1, mode=mode)] == want
    assert profile_scores(P, [byte_codes(SYMBOLS, 23, True)[s] for s in odd], 3, 1, "local") != \
        profile_scores(P, [byte_codes(SYMBOLS, 23, False)[s] for s in odd], 3, 1, "local")


@pytest.mark.gpu
def test_a_byte_outside_the_alphabet_and_empty_sequences(engine):
    rng = np.random.default_rng(107)
    P, cons = random_profile(rng, 70)
    good = profile_seqs(rng, cons, (30, 70))
    bad = good[1].copy()
    bad[17] = ord("@")
    e = np.zeros(0, np.uint8)
    with engine.Profile(SYMBOLS[:23], P[:, :23]) as p:
        with pytest.raises(engine.SwError, match="sequence 1: position 17: byte 0x40 is outside the profile alphabet"):
            engine.score_profile_batch(p, [good[0], bad], 12, 1)
        with pytest.raises(engine.SwError, match="sequence 2: position 17: byte 0x40"):
            engine.align_profile_batch(p, [good[0], e, bad], 12, 1, mode="global")
        # an empty sequence is answered on the host, beside sequences that are launched
        for mode in MODES:
            seqs = [e, good[0], e, good[1]]
            want = profile_scores(P[:, :23], [CODE[s] for s in seqs], 12, 1, mode)
            assert want[0] == (0 if mode == "local" else -(12 + 69))
            assert engine.score_profile_batch(p, seqs, 12, 1, mode=mode) == want
            got = engine.align_profile_batch(p, seqs, 12, 1, mode=mode)
            assert got == engine.align_profile_batch(p, seqs, 12, 1, cpu=True, mode=mode)
            assert [x.score for x in got] == want
            assert engine.score_profile_batch(p, [e, e], 12, 1, mode=mode) == [want[0]] * 2
        assert engine.score_profile(p, good[1], 12, 1) == profile_scores(P[:, :23], [CODE[good[1]]], 12, 1, "local")[0]
        assert engine.score_profile_batch(p, [], 12, 1) == []


# ---- 7. a database ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def profile_db():
    """200 records of 1 to 600 residues, one of them empty; a profile of 300 positions."""
    rng = np.random.default_rng(108)
    P, cons = random_profile(rng, 300)
    lengths = [int(x) for x in rng.integers(1, 601, 200)]
    lengths[:3] = [600, 1, 300]
    recs = profile_seqs(rng, cons, lengths)
    for i in range(0, 200, 8):                                # some hold the consensus further inside
        recs[i] = mutated_copy(rng, np.concatenate([rand_seq(rng, 40), cons]), lengths[i])
    recs[77] = np.zeros(0, np.uint8)
    return P, [("rec%d" % i, r) for i, r in enumerate(recs)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_database(engine, profile_db, mode):
    P, recs = profile_db
    seqs = [r for _, r in recs]
    with engine.Database.from_records(recs) as db, engine.Profile(SYMBOLS, P) as p:
        want = engine.score_profile_batch(p, seqs, 12, 1, mode=mode)
        scores = db.search_profile(p, 12, 1, mode=mode)
        st = engine.last_stats()
        assert (st["mode"], st["items"]) == (PROFILE_MODE, 200)
        assert scores.tolist() == want                        # record order
        assert want[77] == (0 if mode == "local" else -(12 + 299))
        order = sorted(range(200), key=lambda i: (-want[i], i))[:10]
        al = db.align_profile(p, order + [77, order[0]], 12, 1, mode=mode)
        assert engine.last_stats()["mode"] == PROFILE_TRACE_MODE
        assert al == engine.align_profile_batch(p, [seqs[i] for i in order + [77, order[0]]], 12, 1, mode=mode)
        assert [x.score for x in al[:10]] == [want[i] for i in order]
        for x, i in zip(al, order):
            assert rescore_profile(x, P, seqs[i], 12, 1, mode) == x.score
        assert db.top_profile(p, 10, 12, 1, mode=mode) == [(want[i], i, "rec%d" % i) for i in order]
        top = db.top_profile(p, 10, 12, 1, alignments=True, mode=mode)
        assert [t[1] for t in top] == order and [t[3] for t in top] == al[:10]
        # the second search reuses the alphabet check of the first and answers the same
        assert db.search_profile(p, 12, 1, mode=mode).tolist() == want
        assert max(want) > 300
    # records outside a narrower alphabet are named once, by record and position
    with engine.Database.from_records(recs) as db, engine.Profile(SYMBOLS[:12], P[:, :12]) as q:
        with pytest.raises(engine.SwError, match=r"record \d+: position \d+: byte 0x[0-9a-f]{2} is outside the profile alphabet"):
            db.search_profile(q, 12, 1, mode=mode)
        with pytest.raises(engine.SwError, match="record index 200"):
            db.align_profile(q, [0, 200], 12, 1, mode=mode)


# ---- 8. refusals -----------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_refusals(engine, request):
    rng = np.random.default_rng(109)
    P, cons = random_profile(rng, 40)
    s = rand_seq(rng, 40)
    p = engine.Profile(SYMBOLS, P)
    with engine.Database.from_records([("r", s)]) as db:
        for mode in ("global", "semiglobal"):                # a pair over mode_range_ok's bound
            with pytest.raises(engine.SwError, match="sequence 0: score range exceeds the int32 engine in this mode"):
                engine.score_profile(p, s, 1 << 20, 1, mode=mode)
            with pytest.raises(engine.SwError, match="sequence 0: score range exceeds the int32 engine in this mode"):
                engine.align_profile(p, s, 1, 1 << 20, mode=mode)
            with pytest.raises(engine.SwError, match="record 0: score range exceeds the int32 engine in this mode"):
                db.search_profile(p, 1 << 20, 1, mode=mode)
            with pytest.raises(engine.SwError, match="record 0: score range exceeds the int32 engine in this mode"):
                db.align_profile(p, [0], 1 << 20, 1, mode=mode)
        assert engine.score_profile(p, s, 1 << 20, 1) >= 0     # local mode has no such bound
        assert engine.lib().sw_score_profile_batch(p._handle(), None, None, 0, 1, 1, 5, None) == -1
        assert b"sw_score_profile_batch: unknown alignment mode 5" in engine.lib().sw_last_error()
        with pytest.raises(engine.SwError, match="gap penalties"):
            engine.score_profile(p, s, -1, 1)
        # a sequence whose trace does not fit trace_mb: refused, and there is no long path to send it to
        request.addfinalizer(lambda: engine.set_option("trace_mb", 1024))
        engine.set_option("trace_mb", 1)
        big = rand_seq(rng, 60000)
        with pytest.raises(engine.SwError, match="sequence 1: a 40 x 60000 alignment needs .* no long path with a profile"):
            engine.align_profile_batch(p, [s, big], 12, 1)
        engine.set_option("trace_mb", 1024)
        p.close()                                              # a closed profile
        with pytest.raises(engine.SwError, match="profile is closed"):
            engine.score_profile(p, s, 12, 1)
        with pytest.raises(engine.SwError, match="profile is closed"):
            engine.align_profile(p, s, 12, 1)
        with pytest.raises(engine.SwError, match="profile is closed"):
            db.search_profile(p, 12, 1)
    # a score range over 2^28: min(n, m) * largest entry, refused before anything is launched
    n = (1 << 28) // 127 + 1
    with engine.Profile(b"A", np.full((n, 1), 127, np.int8)) as huge:
        long_seq = np.full(n, ord("A"), np.uint8)
        with pytest.raises(engine.SwError, match="sequence 0: score range exceeds the int32 engine"):
            engine.score_profile(huge, long_seq, 12, 1)
        with pytest.raises(engine.SwError, match="sequence 0: score range exceeds the int32 engine"):
            engine.align_profile(huge, long_seq, 12, 1)

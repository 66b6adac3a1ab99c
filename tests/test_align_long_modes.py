"""GPU: long pairs end to end -- checkpointed traceback in global and semi-global mode, on one wave and
on many (include/algoGPU.h sw_align_matrix_long_mode, sw_align_matrix_long_coop_mode and their sw_db_
namesakes; csrc/sw_matrix.hip, the mode instantiations of the locate, cooperative locate and strip-fill
kernels and the resumable walks).

Every alignment is compared for equality -- score, the four coordinates, the operation list -- with the
library's CPU aligner (align_matrix_batch(cpu=True, mode=mode), itself checked against a restatement of the
recurrence in tests/test_modes_cpu.py) and re-scored in Python from its operations alone (rescore_ops).  The
comparison is exact, so there is no tolerance.  Every call runs with option coop_poison = 1 (a checkpoint row
consumed before it was stored carries H of about 10^9), and every option a test touches is put back.  All
tests run in both modes and with coop False and True.  The shapes are a few strips of 512 seq1 positions by
a few chunks of 64 seq2 positions; n is the seq1 length, across the lanes.  What a case is there for is
asserted on the CPU result, so an input that stops exercising it fails the test.  The host arithmetic is
tested without a GPU in tests/test_align_long_modes_cpu.py."""
import threading

import numpy as np
import pytest

from test_matrix_cpu import identity_table, random_table
from test_matrix import SYMBOLS, mutated_copy, rand_seq, table  # noqa: F401  (fixtures)
from test_align_cpu import low_complexity_pairs
from test_align_long import runs, strip_bytes
from test_align_long_coop import coop as poisoned, items_of  # noqa: F401  (fixture)
from test_modes import MODES
from test_modes_cpu import check_shape, rescore_ops

STRIP = 512
MIB = 1 << 20
AM = {"local": 0, "global": 1, "semiglobal": 2}
COOP = (False, True)
_cpu_cache = {}


def cpu_ref(engine, key, pairs, T, go, ge, mode):
    """The CPU aligner's alignments of a named set of pairs: computed once, shared, never changed."""
    k = (key, go, ge, mode)
    if k not in _cpu_cache:
        with engine.Matrix(SYMBOLS, T) as mx:
            _cpu_cache[k] = tuple(engine.align_matrix_batch(pairs, mx, go, ge, cpu=True, mode=mode))
    return _cpu_cache[k]


def both(engine, key, pairs, T, go, ge, mode, coop):
    """The alignments of align_matrix_long(mode=mode, coop=coop) with the call's stats and device times, after
    comparing them with the CPU aligner's and re-scoring each."""
    want = cpu_ref(engine, key, pairs, T, go, ge, mode)
    with engine.Matrix(SYMBOLS, T) as mx:
        got = engine.align_matrix_long(pairs, mx, go, ge, coop=coop, mode=mode)
        st, ms = engine.last_stats(), engine.last_align_long_ms()
    assert (st["mode"], st["W"], st["C"]) == (12 if coop else 8, 8, 64)
    assert st["items"] == (items_of(pairs) if coop else len(pairs))
    assert st["variant"] >> 28 == AM[mode] and st["variant"] & 0xFFFFFFF >= 1
    assert len(got) == len(pairs)
    for k, ((a, b), g, w) in enumerate(zip(pairs, got, want)):
        assert g == w, (mode, coop, k, len(a), len(b), g, w)
        if len(a) and len(b):
            assert rescore_ops(g, a, b, T, go, ge) == g.score, k
            check_shape(g, a, b, mode)
    return got, st, ms


def lead(x, op="I"):
    """The length of the alignment's leading run of `op` (0: it begins otherwise)."""
    return x.ops[0][0] if x.ops and x.ops[0][1] == op else 0


# 1. the grid: strips of 512 by chunks of 64, unrelated and mutated-copy pairs in one batch
@pytest.fixture(scope="module")
def grid():
    rng = np.random.default_rng(181)
    pairs = []
    for n in (1, 511, 512, 513, 1024, 1025, 1537):
        for m in (1, 37, 63, 64, 65, 700):
            a = rand_seq(rng, n)
            pairs += [(a, rand_seq(rng, m)), (a, mutated_copy(rng, a[max(0, n - m - 5):], m))]
    return pairs


@pytest.mark.gpu
@pytest.mark.parametrize("coop", COOP)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gaps", [(12, 1), (3, 1), (0, 0), (1, 3)])      # (1, 3): gx = min(G_INIT, G_EXT)
def test_grid(poisoned, table, grid, gaps, mode, coop):
    got, st, ms = both(poisoned, "grid", grid, table, *gaps, mode, coop)
    assert len(grid) == 84 and ms["rounds"] >= 1 and ms["locate_ms"] > 0 and st["boundary_bytes"] > 0
    assert max(x.score for x in got) > 300 and (min(x.score for x in got) < 0 or gaps == (0, 0))
    assert any(lead(x) > 0 for x in got) and any(x.ops[-1][1] != "M" for x in got)


# 2. negative and zero scores: a full alignment each, never the empty one of a local pair without a score
@pytest.mark.gpu
@pytest.mark.parametrize("coop", COOP)
@pytest.mark.parametrize("mode", MODES)
def test_negative_and_zero_scores(poisoned, table, mode, coop):
    rng = np.random.default_rng(182)
    T = table - 3
    assert T.mean() < 0
    pairs = [(rand_seq(rng, n), rand_seq(rng, m)) for n, m in ((1, 1), (40, 90), (600, 1030), (1030, 64), (1537, 300))]
    got, _, _ = both(poisoned, "negative", pairs, T, 12, 1, mode, coop)
    assert any(x.score < 0 for x in got) and all(x.ops for x in got)
    assert all(x.end1 - x.beg1 == len(a) for (a, b), x in zip(pairs, got))
    Z = table.copy()
    Z[0, 0] = 0                                              # A against A scores nothing
    A = np.full(1, SYMBOLS[0], np.uint8)
    zero = [(np.repeat(A, 600), np.repeat(A, 600)), (np.repeat(A, 1030), np.repeat(A, 1030))]
    got, _, _ = both(poisoned, "zero", zero, Z, 12, 1, mode, coop)
    assert [(x.score, x.ops) for x in got] == [(0, ((600, "M"),)), (0, ((1030, "M"),))]


# 3. leading runs: the walk leaves the matrix at j < 0 strips away from column 0, or at i < 0
@pytest.mark.gpu
@pytest.mark.parametrize("coop", COOP)
@pytest.mark.parametrize("mode", MODES)
def test_leading_runs(poisoned, table, mode, coop):
    rng = np.random.default_rng(183)
    a = rand_seq(rng, 1700, 20)
    # n = 1700, m = 60: seq2 is seq1[1200, 1260), so the walk leaves at j < 0 in strip 2, two strips from the
    # left, after a trailing I run that crosses the boundary at 1536 in state E; and seq2 = the tail of seq1
    pairs = [(a, a[1200:1260].copy()), (a, a[1640:].copy())]
    got, _, ms = both(poisoned, "lead_i", pairs, table, 12, 1, mode, coop)
    assert got[0].ops == ((1200, "I"), (60, "M"), (440, "I")) and got[1].ops == ((1640, "I"), (60, "M"))
    assert lead(got[0]) > 1024 and lead(got[1]) > 1024
    if not coop:                                             # strips 3 and 2, then no further round for the leading run
        assert ms["rounds"] == 2
    if mode == "global":                                     # the exit at i < 0: a leading D run
        b = rand_seq(rng, 600, 20)
        pairs = [(b, np.concatenate([rand_seq(rng, 900, 20), b]))]
        got, _, _ = both(poisoned, "lead_d", pairs, table, 12, 1, mode, coop)
        assert len(pairs[0][1]) == 1500 and got[0].ops == ((900, "D"), (600, "M"))
    else:
        # a whole query planted at the start of a record: the fills have n of the record's m rows; and a query
        # whose tail opens a record that shares no letter with it otherwise: the end row is small, so every
        # fill has rows of a few
        q = rand_seq(rng, 1100, 10)
        other = np.frombuffer(SYMBOLS, np.uint8)[10 + rng.integers(0, 10, 600)]
        pairs = [(q, np.concatenate([q, other]))]
        got, _, _ = both(poisoned, "planted", pairs, table, 12, 1, mode, coop)
        assert (got[0].beg2, got[0].end2, got[0].ops) == (0, 1100, ((1100, "M"),))
        pairs = [(q, np.concatenate([q[1085:], other[:200]]))]
        got, _, _ = both(poisoned, "few_rows", pairs, identity_table(24, 5, -4), 12, 1, mode, coop)
        assert got[0].end2 == 15 and got[0].ops == ((1085, "I"), (15, "M"))


# 4. trailing gaps -- the walk's first cell has source E or F -- and state E across a whole strip
@pytest.mark.gpu
@pytest.mark.parametrize("coop", COOP)
@pytest.mark.parametrize("mode", MODES)
def test_trailing_gaps_and_a_gap_across_a_strip(poisoned, table, mode, coop):
    rng = np.random.default_rng(184)
    a = rand_seq(rng, 1100, 20)
    pairs = [(a, a[:700].copy()), (a, a[:400].copy()), (a[:600].copy(), a)]
    got, _, _ = both(poisoned, "trail", pairs, table, 12, 1, mode, coop)
    assert got[0].ops == ((700, "M"), (400, "I")) and got[1].ops == ((400, "M"), (700, "I"))     # 700 I: across 1024 and 512
    if mode == "global":
        assert got[2].ops == ((600, "M"), (500, "D"))
    # a 1300-long gap: as test_align_long_coop.py::test_a_gap_longer_than_a_window
    T = identity_table(24, 5, -4)
    a = rand_seq(rng, 700 + 1300 + 700, 20)
    if a[699] == a[1999]:                                    # the run cannot slide to the left
        a[699] = SYMBOLS[(SYMBOLS.index(bytes([a[699]])) + 1) % 20]
    b = np.concatenate([a[:700], a[2000:]])
    pairs = [(a, b), (b, a)]
    want = cpu_ref(poisoned, "gap1300", pairs, T, 5, 0, mode)
    assert runs(want[0]) == [("M", 0, 700, 0, 700), ("I", 700, 2000, 700, 700), ("M", 2000, 2700, 700, 1400)]
    assert runs(want[1]) == [("M", 0, 700, 0, 700), ("D", 700, 700, 700, 2000), ("M", 700, 1400, 2000, 2700)]
    for G, rounds in ((2, 3), (1, 6), (0, 1)):
        poisoned.set_option("long_window", G)
        _, _, ms = both(poisoned, "gap1300", pairs, T, 5, 0, mode, coop)
        assert ms["rounds"] == (rounds if coop else 6), G


# 5. ties: two symbols, many alignments reach the score, across strip boundaries
@pytest.mark.gpu
@pytest.mark.parametrize("coop", COOP)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gaps", [(0, 0), (1, 1)])
def test_ties(poisoned, table, gaps, mode, coop):
    rng = np.random.default_rng(185)
    AR = np.frombuffer(SYMBOLS, np.uint8)[[SYMBOLS.index(b"A"), SYMBOLS.index(b"R")]]
    two = lambda n: AR[rng.integers(0, 2, n)]
    polyA = lambda n: np.repeat(AR[:1], n)
    pairs = low_complexity_pairs() + [(two(600), two(560)), (two(1030), two(100)), (two(100), two(1030)),
                                      (polyA(1100), polyA(70)), (polyA(600), polyA(600)), (polyA(1025), two(513))]
    got, _, _ = both(poisoned, "ties", pairs, table, *gaps, mode, coop)
    if mode == "semiglobal":                                 # the smallest j: the first full cover of poly-A by poly-A
        assert (got[2].beg2, got[2].end2) == (0, 5) and (got[13].beg2, got[13].end2) == (0, 600)


# 6. what the cooperative path adds, and the budgets of both paths
@pytest.mark.gpu
@pytest.mark.parametrize("coop", COOP)
@pytest.mark.parametrize("mode", MODES)
def test_more_strips_than_waves(poisoned, table, mode, coop):
    rng = np.random.default_rng(186)
    a = rand_seq(rng, 20 * STRIP)
    pairs = [(a, mutated_copy(rng, a[4000:], 1000))]
    poisoned.set_option("blocks", 1)
    for _ in range(2):                                       # twice: the progress words must be zeroed again
        got, st, _ = both(poisoned, "strips20", pairs, table, 12, 1, mode, coop)
        assert st["blocks"] == 1 and st["items"] == (20 if coop else 1)
    assert lead(got[0]) > 2 * STRIP and got[0].ops[-1][1] == "I"


@pytest.mark.gpu
@pytest.mark.parametrize("coop", COOP)
@pytest.mark.parametrize("mode", MODES)
def test_windows(poisoned, table, mode, coop):
    rng = np.random.default_rng(187)
    a = rand_seq(rng, 3000)
    pairs = [(a, mutated_copy(rng, a, 3000))]
    want = cpu_ref(poisoned, "six", pairs, table, 12, 1, mode)
    assert lead(want[0]) < STRIP                             # the walk reads all six strips
    for G in (1, 2, 3, 0):
        poisoned.set_option("long_window", G)
        _, st, ms = both(poisoned, "six", pairs, table, 12, 1, mode, coop)
        assert ms["rounds"] == (-(-6 // G) if coop and G else 1 if coop else 6) == st["variant"] & 0xFFFFFFF, G


@pytest.mark.gpu
@pytest.mark.parametrize("coop", COOP)
@pytest.mark.parametrize("mode", MODES)
def test_a_round_of_several_launches(poisoned, table, mode, coop):
    rng = np.random.default_rng(188)
    pairs = []
    for k in range(6):
        a = rand_seq(rng, 1537)
        pairs.append((a, mutated_copy(rng, a[20 * k:], 700)))
    poisoned.set_option("trace_mb", 1)
    poisoned.set_option("long_window", 3)
    assert 3 * strip_bytes(700) <= MIB < 4 * strip_bytes(700)           # three strip traces a launch
    got, st, ms = both(poisoned, "launches", pairs, table, 12, 1, mode, coop)
    assert all(lead(x) < STRIP for x in got)                 # every walk reads its four strips
    held = 6 * 3 * 704 * 8 + (24 * 4 + 24 * 16 if coop else 0)          # checkpoints; progress words, end records
    assert st["boundary_bytes"] == held + 3 * strip_bytes(700)
    # one wave: four rounds of six strips, three a launch; many waves: a round of six windows of three strips, a
    # launch each, then the six strips 0, three a launch
    assert ms["rounds"] == (2 if coop else 4) and st["variant"] & 0xFFFFFFF == (6 + 2 if coop else 4 * 2)


@pytest.mark.gpu
@pytest.mark.parametrize("coop", COOP)
@pytest.mark.parametrize("mode", MODES)
def test_two_groups(poisoned, table, mode, coop, monkeypatch):
    rng = np.random.default_rng(189)
    pairs = []
    for k in range(40):
        a = rand_seq(rng, 2600)
        pairs.append((a, mutated_copy(rng, a[int(rng.integers(0, 1900)):], 700) if k % 4 else rand_seq(rng, 700)))
    monkeypatch.setenv("SWMI_ALIGN_CKPT_MB", "1")
    poisoned.set_option("long_window", 1)
    assert poisoned.align_long_plan(2600, 700)["ckpt_bytes"] == 28160 and 37 * 28160 <= MIB < 38 * 28160
    got, st, _ = both(poisoned, "groups", pairs, table, 12, 1, mode, coop)
    assert st["boundary_bytes"] <= MIB + 37 * strip_bytes(700) + 37 * 6 * 20 < 40 * (28160 + strip_bytes(700))
    monkeypatch.delenv("SWMI_ALIGN_CKPT_MB")
    _, st, _ = both(poisoned, "groups", pairs, table, 12, 1, mode, coop)
    assert st["boundary_bytes"] >= 40 * (28160 + strip_bytes(700))     # one group: every pair's first round at once


# 7. the entry points
@pytest.mark.gpu
@pytest.mark.parametrize("coop", COOP)
@pytest.mark.parametrize("mode", MODES)
def test_empty_sequences_beside_launched_pairs(poisoned, table, mode, coop):
    rng = np.random.default_rng(190)
    e = np.zeros(0, np.uint8)
    a = rand_seq(rng, 1100)
    pairs = [(e, a), (a, mutated_copy(rng, a, 300)), (a, e), (e, e), (a[:40], a[:40].copy())]
    got, st, _ = both(poisoned, "empties", pairs, table, 12, 1, mode, coop)
    assert got[2].ops == ((1100, "I"),) and got[3].ops == () and got[4].ops == ((40, "M"),)
    assert got[0].ops == (((1100, "D"),) if mode == "global" else ())
    with poisoned.Matrix(SYMBOLS, table) as mx:
        assert poisoned.align_matrix_long([], mx, 12, 1, coop=coop, mode=mode) == []
        only = poisoned.align_matrix_long([(e, a), (a, e)], mx, 12, 1, coop=coop, mode=mode)
        assert only == [got[0], got[2]]


@pytest.mark.gpu
@pytest.mark.parametrize("coop", COOP)
@pytest.mark.parametrize("mode", MODES)
def test_database(poisoned, table, mode, coop):
    rng = np.random.default_rng(191)
    q = rand_seq(rng, 1500)
    long_rec = np.concatenate([rand_seq(rng, 1500), mutated_copy(rng, q[600:], 880), rand_seq(rng, 620)])
    recs = [("short", rand_seq(rng, 80)), ("long", long_rec), ("none", np.zeros(0, np.uint8)), ("copy", q.copy()),
            ("mid", rand_seq(rng, 700))]
    idx = [1, 2, 0, 1, 3, 4]
    pairs = [(q, recs[i][1]) for i in idx]
    want, _, _ = both(poisoned, "db", pairs, table, 12, 1, mode, coop)
    with poisoned.Database.from_records(recs) as db, poisoned.Matrix(SYMBOLS, table) as mx:
        poisoned.set_option("trace_mb", 1)                   # the whole trace of (q, long) does not fit
        with pytest.raises(poisoned.SwError, match="record 1: a 1500 x 3000 alignment needs .* local only"):
            db.align(q, idx, mx, 12, 1, mode=mode)
        got = db.align_long(q, idx, mx, 12, 1, mode=mode, coop=coop)
        st = poisoned.last_stats()
        assert got == want and got[4].ops == ((1500, "M"),) and got[0] == got[3]
        assert st["mode"] == (12 if coop else 8) and st["items"] == (5 * 3 if coop else 6) and st["variant"] >> 28 == AM[mode]
        assert db.align_long(q, [], mx, 12, 1, mode=mode, coop=coop) == []
        with pytest.raises(poisoned.SwError, match="record index 5"):
            db.align_long(q, [3, 5], mx, 12, 1, mode=mode, coop=coop)


@pytest.mark.gpu
@pytest.mark.parametrize("coop", COOP)
@pytest.mark.parametrize("mode", MODES)
def test_equals_the_whole_trace_path(poisoned, table, mode, coop):
    rng = np.random.default_rng(192)
    a = rand_seq(rng, 2600)
    pairs = [(a, mutated_copy(rng, a[900:], 700)), (a, rand_seq(rng, 700))]
    got, _, _ = both(poisoned, "whole", pairs, table, 12, 1, mode, coop)
    with poisoned.Matrix(SYMBOLS, table) as mx:
        assert poisoned.align_matrix_batch(pairs, mx, 12, 1, mode=mode) == got
        assert poisoned.last_stats()["mode"] == 7


@pytest.mark.gpu
@pytest.mark.parametrize("coop", COOP)
def test_local_through_the_new_entry_points(poisoned, table, grid, coop):
    L = poisoned.lib()
    pairs = grid[::3]
    with poisoned.Matrix(SYMBOLS, table) as mx:
        old = poisoned.align_matrix_long(pairs, mx, 12, 1, coop=coop)
        before = poisoned.last_stats()
        f = L.sw_align_matrix_long_coop_mode if coop else L.sw_align_matrix_long_mode
        assert poisoned._align_pairs(f, pairs, mx, 12, 1, 1 << 16, mode=poisoned.SW_MODE_LOCAL) == old
        st = poisoned.last_stats()
        assert (st["mode"], st["items"], st["variant"]) == (before["mode"], before["items"], before["variant"])
        assert st["variant"] >> 28 == 0
        assert poisoned.align_matrix_long(pairs, mx, 12, 1, coop=coop, mode="local") == old
        assert old == poisoned.align_matrix_batch(pairs, mx, 12, 1, cpu=True) and max(x.score for x in old) > 300
        q = pairs[-1][0]
        with poisoned.Database.from_records([("r%d" % k, b) for k, (_, b) in enumerate(pairs)]) as db:
            idx = list(range(len(pairs)))
            assert db.align_long(q, idx, mx, 12, 1, coop=coop) == db.align(q, idx, mx, 12, 1, long=True, coop=coop)
        with pytest.raises(poisoned.SwError, match="unknown alignment mode 3"):
            poisoned._align_pairs(f, pairs, mx, 12, 1, mode=3)


@pytest.mark.gpu
@pytest.mark.parametrize("coop", COOP)
@pytest.mark.parametrize("mode", MODES)
def test_two_host_threads(poisoned, mode, coop):
    rng = np.random.default_rng(193)
    jobs = []
    for t in range(2):
        T = random_table(rng, 24)
        pairs = []
        for k in range(40):
            a = rand_seq(rng, int(rng.integers(1, 1400)))
            pairs.append((a, mutated_copy(rng, a[int(rng.integers(0, len(a))):], int(rng.integers(1, 400)))))
        jobs.append((T, pairs, (12, 1) if t == 0 else (4, 2)))
    got, errors = [None, None], []
    start = threading.Barrier(2)

    def run(t):
        try:
            T, pairs, gaps = jobs[t]
            with poisoned.Matrix(SYMBOLS, T) as mx:
                start.wait(timeout=60)
                for _ in range(3):
                    got[t] = poisoned.align_matrix_long(pairs, mx, *gaps, coop=coop, mode=mode)
        except Exception as e:      # reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t, (T, pairs, gaps) in enumerate(jobs):
        with poisoned.Matrix(SYMBOLS, T) as mx:
            assert got[t] == poisoned.align_matrix_batch(pairs, mx, *gaps, cpu=True, mode=mode)
        for (a, b), x in zip(pairs, got[t]):
            assert rescore_ops(x, a, b, T, *gaps) == x.score
        assert any(lead(x) > STRIP for x in got[t])

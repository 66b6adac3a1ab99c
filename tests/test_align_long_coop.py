"""GPU: long pairs on many waves (include/algoGPU.h sw_align_matrix_long_coop,
sw_db_align_matrix_long_coop; csrc/sw_matrix.hip sw_matrix_locate_coop_kernel, the windowed rounds and
sw_matrix_walk_window_kernel).

Every alignment is compared bit for bit -- score, the four coordinates, the operation list -- with the
library's CPU aligner (align_matrix_batch(cpu=True)) and re-scored in Python independently of both
(rescore); the cooperative path is never compared with itself.  Every test runs with option
coop_poison = 1: the host fills the checkpoint columns with 0x3F bytes before the locate launch, so a
row consumed before it was stored carries H of about 10^9 into the score and the end cell.  The
shapes are a few strips of 512 seq1 positions by a few chunks of 64 seq2 positions; n is the seq1
length, across the lanes.  The host arithmetic is tested without a GPU in
tests/test_align_long_coop_cpu.py."""
import os
import threading

import numpy as np
import pytest

from test_matrix_cpu import identity_table, matrix_text, random_table
from test_matrix import CODE, SYMBOLS, mutated_copy, rand_seq, table  # noqa: F401  (fixtures)
from test_align_cpu import end_cell, low_complexity_pairs, rescore
from test_align import parse_hits, small_db  # noqa: F401  (fixtures)
from test_align_long import X, deletion_pairs, grid_pairs, runs, strip_bytes, strips_covered  # noqa: F401  (fixtures)

STRIP = 512
MIB = 1 << 20
OPTS = ("blocks", "trace_mb", "coop_poison", "long_window")


@pytest.fixture
def coop(engine, request):
    """The engine with coop_poison = 1; every option a test may touch, and SWMI_ALIGN_CKPT_MB, is put back afterwards."""
    before = {k: engine.get_option(k) for k in OPTS}
    old_env = os.environ.get("SWMI_ALIGN_CKPT_MB")

    def restore():
        for k, v in before.items():
            engine.set_option(k, v)
        if old_env is None:
            os.environ.pop("SWMI_ALIGN_CKPT_MB", None)
        else:
            os.environ["SWMI_ALIGN_CKPT_MB"] = old_env
    request.addfinalizer(restore)
    os.environ.pop("SWMI_ALIGN_CKPT_MB", None)
    engine.set_option("coop_poison", 1)
    return engine


def items_of(pairs):
    """The strips of every pair with two non-empty sequences: what last_stats()["items"] must report."""
    return sum(-(-len(a) // STRIP) for a, b in pairs if len(a) and len(b))


def cpu(engine, pairs, T, gap_init, gap_ext, symbols=SYMBOLS):
    with engine.Matrix(symbols, T) as mx:
        return engine.align_matrix_batch(pairs, mx, gap_init, gap_ext, cpu=True)


def both(engine, pairs, T, gap_init, gap_ext, want=None, symbols=SYMBOLS, code=CODE):
    """The alignments of align_matrix_long(coop=True) with the call's stats and device times, after comparing them
    with the CPU aligner's (want, when the caller has them already) and re-scoring each."""
    with engine.Matrix(symbols, T) as mx:
        got = engine.align_matrix_long(pairs, mx, gap_init, gap_ext, coop=True)
        st, ms = engine.last_stats(), engine.last_align_long_ms()
    if want is None:
        want = cpu(engine, pairs, T, gap_init, gap_ext, symbols)
    assert (st["mode"], st["W"], st["C"], st["items"]) == (12, 8, 64, items_of(pairs))
    assert len(got) == len(pairs)
    for k, ((a, b), g, w) in enumerate(zip(pairs, got, want)):
        assert g == w, (k, len(a), len(b), g, w)
        assert rescore(g, a, b, T, gap_init, gap_ext, code) == g.score, k
    return got, st, ms


def visited(x):
    """The strips a walk reads: from the end cell's down to the strip of the cell at which it stops.  After its
    last operation the walk stands at (beg1 - 1, beg2 - 1); outside the matrix it has ended, else it reads that
    cell (H = 0 there) and ends."""
    if x.score == 0:
        return 0
    stop = (x.beg1 - 1) // STRIP if x.beg1 > 0 and x.beg2 > 0 else x.beg1 // STRIP
    return (x.end1 - 1) // STRIP - stop + 1


def rounds_of(got, G):
    """Rounds of a call whose every window is G strips, cut by strip 0 alone: the slowest pair's."""
    return max([-(-visited(x) // G) for x in got] + [0])


# 1. the grid: strips of 512 by chunks of 64, many pairs' items interleaved in one locate launch
@pytest.mark.gpu
@pytest.mark.parametrize("gaps", [(12, 1), (3, 1), (0, 0), (1, 3)])
def test_grid(coop, table, grid_pairs, gaps):
    got, st, ms = both(coop, grid_pairs, table, *gaps)
    assert st["items"] == sum(-(-n // STRIP) for n in (1, 511, 512, 513, 1024, 1025, 1100, 1537, 2600)) * 6 == 138
    assert st["variant"] >= 1 and st["boundary_bytes"] > 0 and ms["rounds"] >= 1 and ms["locate_ms"] > 0
    assert max(x.score for x in got) > 300
    assert any(strips_covered(x) >= 3 and len(x.ops) > 2 for x in got)
    assert sum(strips_covered(x) == 2 for x in got) > 5


# 2. more strips than waves: one workgroup's four waves work through 20 strips; the same call twice, so the
#    progress words must be zeroed again
@pytest.mark.gpu
def test_more_strips_than_waves(coop, table):
    rng = np.random.default_rng(270)
    a = rand_seq(rng, 20 * STRIP)
    pairs = [(a, mutated_copy(rng, a[4000:], 1000))]
    want = cpu(coop, pairs, table, 12, 1)
    assert strips_covered(want[0]) >= 2
    coop.set_option("blocks", 1)
    for _ in range(2):
        got, st, _ = both(coop, pairs, table, 12, 1, want)
        assert st["items"] == 20 and st["blocks"] == 1


# 3. short rows: with m < 64 a strip's first publication is its last; m = 1
@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 37])
def test_short_rows(coop, table, m):
    rng = np.random.default_rng(280 + m)
    a = rand_seq(rng, 10 * STRIP - 3)
    pairs = [(a, mutated_copy(rng, a[2040:], m)), (a, rand_seq(rng, m)), (a, a[5 * STRIP - m // 2:5 * STRIP - m // 2 + m].copy())]
    got, st, _ = both(coop, pairs, table, 3, 1)
    assert st["items"] == 30 and len(got) == 3


# 4. stale lines: two different pairs of one shape in one launch on one workgroup, then the same shapes with
#    the contents exchanged: a consumer served from a cached line of the other pair's checkpoints, or of the
#    call before, reports the other pair's alignment
@pytest.mark.gpu
def test_stale_lines(coop, table):
    rng = np.random.default_rng(290)
    a, c = rand_seq(rng, 6 * STRIP), rand_seq(rng, 6 * STRIP)
    p, q = (a, mutated_copy(rng, a[1300:], 500)), (c, mutated_copy(rng, c[2300:], 500))
    want = cpu(coop, [p, q], table, 12, 1)
    assert want[0] != want[1] and want[0].score != want[1].score
    coop.set_option("blocks", 1)
    assert coop.align_long_coop_plan(6 * STRIP, 500)["strips"] == 6
    both(coop, [p, q], table, 12, 1, want)
    both(coop, [q, p], table, 12, 1, want[::-1])
    both(coop, [p, q], table, 12, 1, want)


# 5. ties across waves: many cells reach the score, in several strips, which now run on several waves; the end
#    cell -- the host's merge of the strips' records -- and the path are the CPU aligner's
@pytest.mark.gpu
@pytest.mark.parametrize("gaps", [(12, 1), (2, 1), (0, 0)])
def test_ties(coop, table, gaps):
    rng = np.random.default_rng(73)
    A = np.full(1, SYMBOLS[0], np.uint8)
    pairs = low_complexity_pairs() + [(np.repeat(A, 1100), np.repeat(A, 70)), (np.repeat(A, 600), np.repeat(A, 600)),
                                      (np.tile(rand_seq(rng, 7), 90), np.tile(rand_seq(rng, 7), 30)),
                                      (np.tile(rand_seq(rng, 7), 160), np.tile(rand_seq(rng, 7), 100))]
    got, _, _ = both(coop, pairs, table, *gaps)
    several = 0
    for (a, b), x in zip(pairs[:9], got):
        score, i, j, cand = end_cell(a, b, table, *gaps)
        assert (x.score, x.end1, x.end2) == (score, i + 1, j + 1)
        several += cand > 1
    assert several >= 1
    assert (got[9].end1, got[9].end2) == (70, 70) and (got[10].end1, got[10].end2) == (600, 600)


# 6. windows: the same alignments whatever the window, in ceil(strips / G) rounds
@pytest.mark.gpu
def test_windows(coop, table):
    rng = np.random.default_rng(300)
    a = rand_seq(rng, 3000)
    pairs = [(a, mutated_copy(rng, a, 3000))]
    want = cpu(coop, pairs, table, 12, 1)
    assert visited(want[0]) == strips_covered(want[0]) == 6
    with coop.Matrix(SYMBOLS, table) as mx:
        assert coop.align_matrix_long(pairs, mx, 12, 1) == want          # the one-wave path, one strip a round
        assert coop.last_stats()["mode"] == 8
        old_rounds = coop.last_align_long_ms()["rounds"]
    assert old_rounds == 6
    for G in (1, 2, 3, 8):
        coop.set_option("long_window", G)
        _, st, ms = both(coop, pairs, table, 12, 1, want)
        assert ms["rounds"] == -(-6 // G) == st["variant"], G
        assert st["boundary_bytes"] == 5 * 3008 * 8 + 32 + 96 + min(G, 6) * strip_bytes(3000)
    coop.set_option("long_window", 1)
    assert both(coop, pairs, table, 12, 1, want)[2]["rounds"] == old_rounds
    coop.set_option("long_window", 0)                                   # automatic: all six strips at once
    assert both(coop, pairs, table, 12, 1, want)[2]["rounds"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("gaps", [(12, 1), (5, 0)])
@pytest.mark.parametrize("B", [512, 1024])
def test_windows_at_boundary_crossings(coop, table, gaps, B):
    """test_align_long.py::test_boundary_crossings' pairs with two strips a round: gaps across the boundary in both
    orientations, begin and end cells on it, walks that end inside a window, windows cut by strip 0."""
    rng = np.random.default_rng(72 + B)
    dels = deletion_pairs(rng, B)
    pairs = []
    for at, a, b in dels:
        pairs += [(a, b), (b, a)]
    T = identity_table(24, 5, -4)
    a = rand_seq(rng, B + 380, 20)                           # no 'X' in it
    n = len(a)
    junk = np.repeat(X, 25)
    cases = [
        (a, a[B - 100:B + 100].copy(), (B - 100, B + 100)),
        (a, np.concatenate([junk, a[B:B + 60], junk]), (B, B + 60)),             # begins at i = B: a round that ends at once
        (a, np.concatenate([junk, a[B - 1:B + 60], junk]), (B - 1, B + 60)),
        (a, a[B:B + 60].copy(), (B, B + 60)),                                    # leaves the strip and the matrix at once
        (a, a[B - 1:B + 60].copy(), (B - 1, B + 60)),
        (a, np.concatenate([junk, a[B - 40:B], junk]), (B - 40, B)),             # ends in a strip's last column
        (a, np.concatenate([junk, a[B - 40:B + 1], junk]), (B - 40, B + 1)),     # in the next strip's first column
        (a, np.concatenate([junk, a[n - 60:]]), (n - 60, n)),
        (a, a[:B + 8].copy(), (0, B + 8)),
    ]
    flat = []
    for p, q, _ in cases:
        flat += [(p, q), (q, p)]
    for batch, tab in ((pairs, table), (flat, T)):
        want = cpu(coop, batch, tab, *gaps)
        with coop.Matrix(SYMBOLS, tab) as mx:
            assert coop.align_matrix_long(batch, mx, *gaps) == want
            old_rounds = coop.last_align_long_ms()["rounds"]
        assert old_rounds == rounds_of(want, 1)
        for G in (1, 2):
            coop.set_option("long_window", G)
            _, _, ms = both(coop, batch, tab, *gaps, want)
            assert ms["rounds"] == rounds_of(want, G), G
    got = cpu(coop, flat, T, *gaps)
    for k, (p, q, (lo, hi)) in enumerate(cases):
        assert (got[2 * k].beg1, got[2 * k].end1, got[2 * k].ops) == (lo, hi, ((hi - lo, "M"),)), k
    assert visited(got[2]) == 2 and strips_covered(got[2]) == 1          # begins at i = B: one more strip is read


# 7. a gap longer than a window
@pytest.mark.gpu
def test_a_gap_longer_than_a_window(coop):
    rng = np.random.default_rng(310)
    T = identity_table(24, 5, -4)
    a = rand_seq(rng, 700 + 1300 + 700, 20)
    if a[699] == a[1999]:                                      # the run cannot slide to the left (deletion_pairs)
        a[699] = SYMBOLS[(SYMBOLS.index(bytes([a[699]])) + 1) % 20]
    b = np.concatenate([a[:700], a[2000:]])
    pairs = [(a, b), (b, a)]
    want = cpu(coop, pairs, T, 5, 0)
    assert runs(want[0]) == [("M", 0, 700, 0, 700), ("I", 700, 2000, 700, 700), ("M", 2000, 2700, 700, 1400)]
    assert runs(want[1]) == [("M", 0, 700, 0, 700), ("D", 700, 700, 700, 2000), ("M", 700, 1400, 2000, 2700)]
    # (a, b): six strips; with two a round the I-run crosses strip 2 inside the window [2, 3] and leaves it, at
    # i = 1023, in state E.  (b, a): the D-run stays in column 699 of strip 1 while j falls by 1300.
    for G, rounds in ((2, 3), (1, 6), (0, 1)):
        coop.set_option("long_window", G)
        _, _, ms = both(coop, pairs, T, 5, 0, want)
        assert ms["rounds"] == rounds, G


# 8. budgets: windows never take a launch over trace_mb
@pytest.mark.gpu
@pytest.mark.parametrize("window", [0, 3])
def test_budgets(coop, table, window):
    rng = np.random.default_rng(76)
    pairs = []
    for k in range(6):
        a = rand_seq(rng, 1537)
        pairs.append((a, mutated_copy(rng, a[400 + 20 * k:], 700)))
    coop.set_option("trace_mb", 1)
    coop.set_option("long_window", window)
    assert 3 * strip_bytes(700) <= MIB < 4 * strip_bytes(700)       # three strip traces a launch
    want = cpu(coop, pairs, table, 12, 1)
    assert min(strips_covered(x) for x in want) >= 3
    got, st, ms = both(coop, pairs, table, 12, 1, want)
    held = 6 * 3 * 704 * 8 + 24 * 4 + 24 * 16                       # checkpoints, progress words, end records
    assert st["boundary_bytes"] <= MIB + held
    if window == 3:      # a pair's three strips fill a launch: six launches in the first round
        assert ms["rounds"] == rounds_of(want, 3) and st["variant"] >= 6
        assert st["boundary_bytes"] == held + 3 * strip_bytes(700)
    else:                # six pairs walking: floor(1 MiB / six strips) = 0, so a strip a pair until pairs finish
        assert st["variant"] >= 2 * 3
    again, _, _ = both(coop, pairs[::-1], table, 12, 1, want[::-1])
    assert again == got[::-1]


# 9. databases and the command line
@pytest.mark.gpu
def test_database(coop, table, small_db):
    recs, q = small_db
    rng = np.random.default_rng(79)
    with coop.Database.from_records(recs) as db, coop.Matrix(SYMBOLS, table) as mx:
        idx = list(range(48)) + [9, 9, 0]                    # repeated indices; records 5, 22 and 39 are empty
        want = db.align(q, idx, mx, 12, 1, long=True)
        assert coop.last_stats()["mode"] == 8
        got = db.align(q, idx, mx, 12, 1, long=True, coop=True)
        st = coop.last_stats()
        assert got == want == coop.align_matrix_batch([(q, recs[i][1]) for i in idx], mx, 12, 1, cpu=True)
        assert st["mode"] == 12 and st["items"] == sum(1 for i in idx if len(recs[i][1]))
        assert got[9].ops == ((260, "M"),) and got[5].score == 0 and len(recs[5][1]) == 0
        assert db.align(q, [], mx, 12, 1, long=True, coop=True) == []
        with pytest.raises(coop.SwError, match="sw_db_align_matrix_long_coop: record index 48"):
            db.align(q, [3, 48], mx, 12, 1, long=True, coop=True)
    # a three-strip query against a 3000-residue record that holds a copy of its strips 1 and 2
    q2 = rand_seq(rng, 1500)
    long_rec = np.concatenate([rand_seq(rng, 1500), mutated_copy(rng, q2[600:], 880), rand_seq(rng, 620)])
    recs2 = [("short", rand_seq(rng, 80)), ("long", long_rec), ("none", np.zeros(0, np.uint8)), ("copy", q2.copy())]
    with coop.Database.from_records(recs2) as db, coop.Matrix(SYMBOLS, table) as mx:
        coop.set_option("trace_mb", 1)
        idx = [1, 2, 0, 1, 3]
        got = db.align(q2, idx, mx, 12, 1, long=True, coop=True)
        st = coop.last_stats()
        want = coop.align_matrix_batch([(q2, recs2[i][1]) for i in idx], mx, 12, 1, cpu=True)
        assert got == want and got[0] == got[3] and got[1].score == 0 and got[4].ops == ((1500, "M"),)
        assert st["mode"] == 12 and st["items"] == 4 * 3 and strips_covered(got[0]) >= 2 and got[0].end2 > 2000
        assert rescore(got[0], q2, long_rec, table, 12, 1) == got[0].score


@pytest.mark.gpu
def test_align_command_line(coop, table, small_db, tmp_path, capsys):
    from concurrentproject_amd.align import main
    recs, q = small_db
    queries = [q, recs[4][1][:50]]
    dbf, qf, mf = tmp_path / "d.fa", tmp_path / "q.fa", tmp_path / "M.txt"
    dbf.write_bytes(b"".join(b">%s\n%s\n" % (h.encode(), s.tobytes()) for h, s in recs))
    qf.write_bytes(b"".join(b">query%d\n%s\n" % (k, x.tobytes()) for k, x in enumerate(queries)))
    mf.write_bytes(matrix_text(SYMBOLS, table))
    base = ["--query", str(qf), "--db", str(dbf), "--matrix", str(mf), "--gaps", "12,1", "--top", "5"]
    assert main(base + ["--alignments", "--long"]) == 0
    whole = capsys.readouterr().out
    assert coop.last_stats()["mode"] == 8
    assert main(base + ["--alignments", "--long", "--coop"]) == 0
    assert capsys.readouterr().out == whole and coop.last_stats()["mode"] == 12
    assert len(parse_hits(whole)) == 10
    with pytest.raises(SystemExit):                           # --coop is a way of running --long
        main(base + ["--alignments", "--coop"])
    capsys.readouterr()


# 10. two host threads, each with its own table and batch
@pytest.mark.gpu
def test_two_host_threads(coop):
    rng = np.random.default_rng(80)
    jobs = []
    for t in range(2):
        T = random_table(rng, 24)
        pairs = []
        for k in range(60):
            a = rand_seq(rng, int(rng.integers(1, 1400)))
            pairs.append((a, mutated_copy(rng, a[int(rng.integers(0, len(a))):], int(rng.integers(1, 400)))))
        jobs.append((T, pairs, (12, 1) if t == 0 else (4, 2)))
    got, errors = [None, None], []
    start = threading.Barrier(2)

    def run(t):
        try:
            T, pairs, gaps = jobs[t]
            with coop.Matrix(SYMBOLS, T) as mx:
                start.wait(timeout=60)
                for _ in range(3):
                    got[t] = coop.align_matrix_long(pairs, mx, *gaps, coop=True)
        except Exception as e:      # reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t, (T, pairs, gaps) in enumerate(jobs):
        assert got[t] == cpu(coop, pairs, T, *gaps)
        for (a, b), x in zip(pairs, got[t]):
            assert rescore(x, a, b, T, *gaps) == x.score
        assert any(strips_covered(x) >= 2 for x in got[t])

"""GPU: local-alignment scores under a substitution matrix (include/algoGPU.h sw_score_matrix*,
sw_db_search_matrix; csrc/sw_matrix.hip), bit-exact against the plain restatement of the
recurrence in tests/test_matrix_cpu.py (checker_batch, itself pinned to the oracle there).

Tables are random with diagonal entries in [4, 11] and off-diagonal entries in [-4, 3] over 24
symbols unless a test says otherwise."""
import threading

import numpy as np
import pytest

from test_matrix_cpu import AA, byte_codes, checker_batch, identity_table, matrix_text, random_table

SYMBOLS = b"ARNDCQEGHILKMFPSTWYVBZX*"
CODE = byte_codes(SYMBOLS)
SYM = np.frombuffer(SYMBOLS, np.uint8)


def rand_seq(rng, n, k=23):
    return SYM[rng.integers(0, k, n)]


def mutated_copy(rng, a, m):
    """A sequence of length m made from `a`: a window of it with ~6 % substitutions, a few
    deletions and insertions (so that alignments take gaps), cut or padded to m."""
    b = a[:max(1, min(len(a), m + 3))].copy()
    if len(b) > 8:
        sub = rng.random(len(b)) < 0.06
        b[sub] = rand_seq(rng, int(sub.sum()))
        for _ in range(1 + len(b) // 80):
            at = int(rng.integers(1, len(b) - 1))
            if rng.random() < 0.5:
                b = np.delete(b, slice(at, at + int(rng.integers(1, 4))))
            else:
                b = np.insert(b, at, rand_seq(rng, int(rng.integers(1, 4))))
    if len(b) < m:
        b = np.concatenate([b, rand_seq(rng, m - len(b))])
    return np.ascontiguousarray(b[:m])


def check_many(pairs, table, gap_init, gap_ext, code=CODE):
    """checker_batch over byte pairs, in chunks of similar size (less padding)."""
    order = sorted(range(len(pairs)), key=lambda k: (len(pairs[k][0]), len(pairs[k][1])))
    out = [0] * len(pairs)
    for c in range(0, len(order), 48):
        idx = order[c:c + 48]
        got = checker_batch([(code[pairs[k][0]], code[pairs[k][1]]) for k in idx], table, gap_init, gap_ext)
        for k, s in zip(idx, got):
            out[k] = s
    return out


@pytest.fixture(scope="module")
def table():
    return random_table(np.random.default_rng(24), 24)


@pytest.fixture(scope="module")
def edge_pairs():
    rng = np.random.default_rng(1)
    pairs = []
    for i, n in enumerate((1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1025)):
        for j, m in enumerate((1, 2, 31, 32, 33, 63, 64, 65, 130, 300)):
            a = rand_seq(rng, n)
            b = rand_seq(rng, m) if (i + j) % 2 == 0 else mutated_copy(rng, a, m)   # half random, half a mutated copy
            pairs.append((a, b))
    return pairs


# 1. every strip boundary for W in {1, 2, 4, 8}, every chunk edge
@pytest.mark.gpu
@pytest.mark.parametrize("gaps", [(12, 1), (3, 1), (2, 2), (0, 0), (1, 3)])
def test_strip_and_chunk_edges(engine, table, edge_pairs, gaps):
    want = check_many(edge_pairs, table, *gaps)
    with engine.Matrix(SYMBOLS, table) as mx:
        got = engine.score_matrix_batch(edge_pairs, mx, *gaps)
        assert got == want
        swapped = engine.score_matrix_batch([(b, a) for a, b in edge_pairs], engine.Matrix(SYMBOLS, table.T), *gaps)
        assert swapped == want
    assert max(want) > 300


@pytest.mark.gpu
@pytest.mark.parametrize("W", [1, 2, 4, 8])
def test_every_columns_per_lane_variant(engine, request, table, edge_pairs, W):
    request.addfinalizer(lambda: engine.set_option("W", 0))
    engine.set_option("W", W)
    pairs = edge_pairs[::3]
    with engine.Matrix(SYMBOLS, table) as mx:
        got = engine.score_matrix_batch(pairs, mx, 12, 1)
        assert engine.last_stats()["W"] == W
    assert got == check_many(pairs, table, 12, 1)


# 2. an asymmetric table, both orientations
@pytest.mark.gpu
def test_asymmetric_table_and_orientation(engine):
    rng = np.random.default_rng(2)
    T = random_table(rng, 24)
    T[3, :] += 2          # markedly asymmetric
    assert (T != T.T).any()
    a = rand_seq(rng, 900)
    b = mutated_copy(rng, a[400:], 40)
    c = rand_seq(rng, 40)
    d = mutated_copy(rng, np.concatenate([rand_seq(rng, 300), c, rand_seq(rng, 600)]), 900)
    pairs = [(a, b), (c, d)]
    want = check_many(pairs, T, 5, 1)
    assert want != check_many(pairs, T.T, 5, 1)      # the orientation matters for these inputs
    with engine.Matrix(SYMBOLS, T) as M, engine.Matrix(SYMBOLS, T.T) as MT:
        assert engine.score_matrix_batch(pairs, M, 5, 1) == want
        for (x, y), w in zip(pairs, want):
            assert engine.score_matrix(x, y, M, 5, 1) == w
            assert engine.score_matrix(y, x, MT, 5, 1) == w
        assert engine.score_matrix_batch([(y, x) for x, y in pairs], MT, 5, 1) == want


# 3. two workgroups: every wave claims many pairs, the scratch is reused between pairs of different lengths
@pytest.mark.gpu
@pytest.mark.parametrize("W", [0, 1])
def test_claim_loop(engine, request, table, W):
    def restore():
        engine.set_option("blocks", 0)
        engine.set_option("W", 0)
    request.addfinalizer(restore)
    rng = np.random.default_rng(3)
    pairs = [(rand_seq(rng, int(rng.integers(1, 49))), rand_seq(rng, int(rng.integers(1, 49)))) for _ in range(300)]
    for _ in range(2):
        a = rand_seq(rng, 700)
        pairs.append((a, mutated_copy(rng, a[100:], 500)))
    a = rand_seq(rng, 640)                       # more multi-strip pairs of other lengths
    pairs += [(a, mutated_copy(rng, a, 333)), (rand_seq(rng, 90), rand_seq(rng, 1100))]
    want = check_many(pairs, table, 12, 1)
    engine.set_option("blocks", 2)
    engine.set_option("W", W)
    with engine.Matrix(SYMBOLS, table) as mx:
        assert engine.score_matrix_batch(pairs, mx, 12, 1) == want
        st = engine.last_stats()
        assert st["blocks"] == 2 and st["items"] == len(pairs) and st["boundary_bytes"] > 0
        assert engine.score_matrix_batch(pairs[::-1], mx, 12, 1) == want[::-1]


# 4. edge values
@pytest.mark.gpu
def test_edge_values(engine, table):
    rng = np.random.default_rng(4)
    a = rand_seq(rng, 70)
    empty = np.zeros(0, np.uint8)
    with engine.Matrix(SYMBOLS, table) as mx:
        assert engine.score_matrix_batch([], mx, 12, 1) == []
        assert engine.lib().sw_score_matrix_batch(mx._handle(), None, None, None, None, 0, 12, 1, None) == 0
        assert engine.score_matrix(empty, a, mx, 12, 1) == 0
        assert engine.score_matrix(a, empty, mx, 12, 1) == 0
        assert engine.score_matrix(empty, empty, mx, 12, 1) == 0
        got = engine.score_matrix_batch([(empty, a), (a, a), (a, empty), (a[:1], a[:1])], mx, 12, 1)
        assert got == [0, int(table[CODE[a], CODE[a]].sum()), 0, int(table[CODE[a[0]], CODE[a[0]]])]
        for bad in ((-1, 1), (1, -1), ((1 << 20) + 1, 1)):
            with pytest.raises(engine.SwError, match="gap penalties"):
                engine.score_matrix(a, a, mx, *bad)
        assert engine.score_matrix(a, a, mx, 1 << 20, 1 << 20) == int(table[CODE[a], CODE[a]].sum())
    neg = -1 - np.abs(table)
    with engine.Matrix(SYMBOLS, neg) as mx:
        assert engine.score_matrix(a, a, mx, 1, 1) == 0
    # int32: 3000 residues against themselves, 127 on the diagonal
    with engine.Matrix(SYMBOLS, identity_table(24, 127, -127)) as mx:
        s = rand_seq(rng, 3000)
        assert engine.score_matrix(s, s, mx, 12, 1) == 381000
        # over the 2^28 bound: refused with a message, nothing launched
        before = engine.last_stats()
        n = (1 << 28) // 127 + 1
        big = np.full(n, SYMBOLS[0], np.uint8)
        with pytest.raises(engine.SwError, match=r"pair 1: score range exceeds .*2\^28"):
            engine.score_matrix_batch([(a, a), (big, big)], mx, 12, 1)
        assert engine.last_stats() == before
        assert engine.score_matrix(big[:n - 2], big[:5], mx, 12, 1) == 5 * 127   # long, but in range


# 5. bytes outside the alphabet
@pytest.mark.gpu
def test_bytes_outside_the_alphabet(engine, table):
    rng = np.random.default_rng(5)
    pairs = []
    for _ in range(12):
        a, b = rand_seq(rng, int(rng.integers(30, 400))), rand_seq(rng, int(rng.integers(30, 400)))
        a[rng.integers(0, len(a), 5)] = rng.integers(0, 256, 5)      # any byte
        b[rng.integers(0, len(b), 5)] = np.frombuffer(b"acxz@", np.uint8)
        pairs.append((a, b))
    other = SYMBOLS.index(b"X")
    with engine.Matrix(SYMBOLS, table, other=other) as mx:
        assert engine.score_matrix_batch(pairs, mx, 12, 1) == check_many(pairs, table, 12, 1, byte_codes(SYMBOLS, other))
    with engine.Matrix(SYMBOLS, table, other=other, fold_case=True) as mx:
        code = byte_codes(SYMBOLS, other, True)
        assert code[ord("a")] == CODE[ord("A")] and code[ord("@")] == other
        assert engine.score_matrix_batch(pairs, mx, 12, 1) == check_many(pairs, table, 12, 1, code)
    lower = [(np.char.lower(a.view("S1")).view(np.uint8), b) for a, b in
             [(rand_seq(rng, 200, 20), rand_seq(rng, 150, 20)) for _ in range(4)]]
    upper = [(np.char.upper(a.view("S1")).view(np.uint8), b) for a, b in lower]
    with engine.Matrix(SYMBOLS, table, fold_case=True) as mx:
        assert engine.score_matrix_batch(lower, mx, 3, 1) == check_many(upper, table, 3, 1)
    with engine.Matrix(SYMBOLS, table) as mx:       # other = -1: an error that names index, position, byte
        good = (rand_seq(rng, 50), rand_seq(rng, 60))
        bad = rand_seq(rng, 40)
        bad[17] = ord("J")
        with pytest.raises(engine.SwError, match="pair 1: seq2 position 17: byte 0x4a"):
            engine.score_matrix_batch([good, (good[0], bad)], mx, 12, 1)
        with pytest.raises(engine.SwError, match="pair 0: seq1 position 17: byte 0x4a"):
            engine.score_matrix(bad, good[0], mx, 12, 1)
        with pytest.raises(engine.SwError, match="pair 0: seq1 position 2: byte 0x61"):
            engine.score_matrix(b"RNaD", good[0], mx, 12, 1)                # lower case without fold_case


# 6. the identity table against the existing engine and the oracle
@pytest.mark.gpu
def test_identity_table_against_the_engine(engine, oracle_mod):
    rng = np.random.default_rng(6)
    pairs = []
    for k in range(64):
        a = AA[rng.integers(0, 20, int(rng.integers(1, 701)))]
        b = AA[rng.integers(0, 20, int(rng.integers(1, 701)))]
        if k % 2:
            b = np.delete(a, rng.integers(0, len(a), len(a) // 20))
        pairs.append((a, b))
    with engine.Matrix(AA.tobytes(), identity_table(20, 2, -3)) as mx:
        got = engine.score_matrix_batch(pairs, mx, 5, 2)
    assert got == engine.score_batch(pairs, engine.Params(2, -3, 5, 2))
    assert got == [oracle_mod.score_linear(a, b, oracle_mod.Params(2, -3, 5, 2)) for a, b in pairs]


# 7. databases
@pytest.fixture(scope="module")
def db_case(table):
    rng = np.random.default_rng(7)
    recs = []
    for i in range(400):
        n = 0 if i % 37 == 0 else int(rng.integers(1, 601))
        recs.append(("rec%d" % i, rand_seq(rng, n)))
    queries = [rand_seq(rng, 300), rand_seq(rng, 1), rand_seq(rng, 77)]
    for q in queries[::2]:     # homologues of the query among the records
        for i in rng.integers(0, 400, 6):
            recs[int(i)] = (recs[int(i)][0], mutated_copy(rng, q, int(rng.integers(len(q) // 2, 500))))
    recs[5] = (recs[5][0], queries[0].copy())
    want = [check_many([(q, s) for _, s in recs], table, 12, 1) for q in queries]
    return recs, queries, want


@pytest.mark.gpu
def test_database_search(engine, oracle_mod, table, db_case):
    recs, queries, want = db_case
    q = queries[0]
    with engine.Database.from_records(recs) as db, engine.Matrix(SYMBOLS, table) as mx:
        got = db.search(q, matrix=mx, gap_init=12, gap_ext=1)
        assert got.dtype == np.int32 and got.tolist() == want[0]
        assert engine.last_stats()["mode"] == 6
        eq = db.search(q)                                       # an equality search in between
        assert eq.tolist() == [oracle_mod.score_linear(q, s) for _, s in recs]
        assert db.search(q, matrix=mx, gap_init=12, gap_ext=1).tolist() == want[0]
        with engine.Database.from_records([("q%d" % k, x) for k, x in enumerate(queries)]) as qdb:
            many = db.search_db(qdb, matrix=mx, gap_init=12, gap_ext=1)
        assert many.shape == (3, 400) and many.tolist() == want
        top = db.top(q, k=12, matrix=mx, gap_init=12, gap_ext=1)
        order = sorted(range(400), key=lambda i: (-want[0][i], i))[:12]
        assert top == [(want[0][i], i, "rec%d" % i) for i in order]
        assert top[0][1] == 5
        assert db.search(np.zeros(0, np.uint8), matrix=mx, gap_init=12, gap_ext=1).tolist() == [0] * 400
        with pytest.raises(engine.SwError, match="gap_init"):
            db.search(q, matrix=mx)
        with pytest.raises(engine.SwError, match="matrix="):
            db.search(q, gap_init=12, gap_ext=1)
        bad = q.copy()
        bad[9] = ord("J")
        with pytest.raises(engine.SwError, match="query 0: position 9: byte 0x4a"):
            db.search(bad, matrix=mx, gap_init=12, gap_ext=1)
    bad_recs = list(recs[:8])
    s = recs[7][1].copy()
    s[3] = ord("a")
    bad_recs[7] = ("bad", s)
    with engine.Database.from_records(bad_recs) as db, engine.Matrix(SYMBOLS, table) as mx:
        with pytest.raises(engine.SwError, match="record 7: position 3: byte 0x61"):
            db.search(q, matrix=mx, gap_init=12, gap_ext=1)
        with engine.Matrix(SYMBOLS, table, fold_case=True) as folded:      # another matrix is checked anew
            assert len(db.search(q, matrix=folded, gap_init=12, gap_ext=1)) == 8


@pytest.mark.gpu
def test_align_command_line(engine, table, db_case, tmp_path, capsys):
    from concurrentproject_amd.align import main
    recs, queries, want = db_case
    dbf, qf, mf = tmp_path / "d.fa", tmp_path / "q.fa", tmp_path / "M.txt"
    dbf.write_bytes(b"".join(b">%s\n%s\n" % (h.encode(), s.tobytes()) for h, s in recs))
    qf.write_bytes(b"".join(b">query%d\n%s\n" % (k, x.tobytes()) for k, x in enumerate(queries)))
    mf.write_bytes(matrix_text(SYMBOLS, table))
    assert main(["--query", str(qf), "--db", str(dbf), "--matrix", str(mf), "--gaps", "12,1", "--top", "5"]) == 0
    lines = capsys.readouterr().out.split("\n")[:-1]
    exp = []
    for k in range(3):
        order = sorted(range(400), key=lambda i: (-want[k][i], i))[:5]
        exp += ["%d\tquery%d\t%d\t%d\t%d\trec%d" % (k, k, r + 1, want[k][i], i, i) for r, i in enumerate(order)]
    assert lines == exp
    with pytest.raises(SystemExit):
        main(["--query", str(qf), "--db", str(dbf), "--matrix", str(mf)])     # --gaps is required with --matrix


# 8. two host threads, each with its own table and batch
@pytest.mark.gpu
def test_two_host_threads(engine):
    rng = np.random.default_rng(8)
    jobs = []
    for t in range(2):
        T = random_table(rng, 24)
        pairs = [(rand_seq(rng, int(rng.integers(1, 400))), rand_seq(rng, int(rng.integers(1, 400)))) for _ in range(150)]
        jobs.append((T, pairs, (12, 1) if t == 0 else (4, 2)))
    got, errors = [None, None], []
    start = threading.Barrier(2)

    def run(t):
        try:
            T, pairs, gaps = jobs[t]
            with engine.Matrix(SYMBOLS, T) as mx:
                start.wait(timeout=60)
                for _ in range(3):
                    got[t] = engine.score_matrix_batch(pairs, mx, *gaps)
        except Exception as e:      # reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t, (T, pairs, gaps) in enumerate(jobs):
        assert got[t] == check_many(pairs, T, *gaps)


# 9. the launch statistics
@pytest.mark.gpu
def test_last_stats_mode(engine, table):
    rng = np.random.default_rng(9)
    pairs = [(rand_seq(rng, 500, 20), rand_seq(rng, 300, 20)) for _ in range(8)]
    with engine.Matrix(SYMBOLS, table) as mx:
        engine.score_matrix_batch(pairs, mx, 12, 1)
    st = engine.last_stats()
    assert st["mode"] == 6 and st["items"] == 8 and st["dna"] == 0 and st["cells"] == 8 * 500 * 300
    assert st["W"] in (1, 2, 4, 8) and st["C"] == 64 and st["kernel_ms"] > 0 and st["total_ms"] >= st["kernel_ms"]
    assert st["boundary_bytes"] >= 0
    engine.score_batch(pairs)
    assert engine.last_stats()["mode"] != 6
    # the process-wide constants are neither read nor written by matrix calls
    assert engine.get_params() == engine.Params()

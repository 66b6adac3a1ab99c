"""Substitution matrices, host side (include/algoGPU.h sw_matrix_*; csrc/sw_matrix_host.cpp), no GPU:

* the library's NCBI-format parse against a plain-Python parse written here (comments, a '*'
  column, CRLF, tabs and runs of blanks, no final newline, an asymmetric table), and every
  malformed case returning an error with a message;
* sw_matrix_score against the table for every byte pair, `other` and fold-case included;
* the checker of the GPU tests (tests/test_matrix.py imports it from here): a plain restatement
  of the recurrence over a K x K table, pinned to the reference-pinned oracle on the identity
  table;
* the parser under AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone program
  (tests/asan/matrix_parse_driver.cpp, `make -C concurrentproject_amd/csrc asan-matrix`)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
BIG = 1 << 24   # a padding cell's score: far below any real H, far from int32 overflow


# ---- the checker ---------------------------------------------------------------------------------

def byte_codes(symbols: bytes, other: int = -1, fold_case: bool = False) -> np.ndarray:
    """byte -> symbol index (-1: outside the alphabet), as include/algoGPU.h defines it."""
    code = np.full(256, other, dtype=np.int64)
    if fold_case:
        for i, s in enumerate(symbols):
            if ord("A") <= s <= ord("Z") and (s + 32) not in symbols:
                code[s + 32] = i
    for i, s in enumerate(symbols):
        code[s] = i
    return code


def checker_batch(pairs, table, gap_init, gap_ext):
    """The recurrence restated (main.cpp:54-66 with s a table lookup): borders 0,
    E[i][j] = max(E[i][j-1] - G_EXT, H[i][j-1] - G_INIT), F[i][j] = max(F[i-1][j] - G_EXT,
    H[i-1][j] - G_INIT), H = max(0, H[i-1][j-1] + table[a_i][b_j], E, F), score = max H.
    ``pairs``: (a, b) arrays of symbol indices; all pairs advance together, one anti-diagonal per
    NumPy step.  Shorter pairs are padded with a symbol that scores -BIG: padded cells lie below
    and right of every real cell, so no real cell depends on one, and their H never exceeds an
    H they inherit through E or F, so the maximum is the pair's."""
    P = len(pairs)
    if P == 0:
        return []
    T = np.asarray(table, dtype=np.int32)
    K = T.shape[0]
    N = max(len(a) for a, _ in pairs)
    M = max(len(b) for _, b in pairs)
    if N == 0 or M == 0:
        return [0] * P
    Tp = np.full((K + 1, K + 1), -BIG, dtype=np.int32)
    Tp[:K, :K] = T
    A = np.full((P, N), K, dtype=np.int64)
    B = np.full((P, M), K, dtype=np.int64)
    for k, (a, b) in enumerate(pairs):
        A[k, :len(a)] = a
        B[k, :len(b)] = b
    go, ge = np.int32(gap_init), np.int32(gap_ext)
    rows = np.arange(P)[:, None]
    # diagonal d - 1: H1, E1, F1; diagonal d - 2: H2; cell (i, j) at index i + 1, borders 0
    H1 = np.zeros((P, N + 1), np.int32)
    H2 = np.zeros((P, N + 1), np.int32)
    E1 = np.zeros((P, N + 1), np.int32)
    F1 = np.zeros((P, N + 1), np.int32)
    best = np.zeros(P, np.int32)
    for d in range(N + M - 1):
        lo, hi = max(0, d - M + 1), min(N - 1, d)
        s = Tp[A[:, lo:hi + 1], B[rows, d - np.arange(lo, hi + 1)[None, :]]]
        E = np.maximum(E1[:, lo + 1:hi + 2] - ge, H1[:, lo + 1:hi + 2] - go)   # from (i, j - 1)
        F = np.maximum(F1[:, lo:hi + 1] - ge, H1[:, lo:hi + 1] - go)           # from (i - 1, j)
        H = np.maximum(np.maximum(H2[:, lo:hi + 1] + s, 0), np.maximum(E, F))
        best = np.maximum(best, H.max(axis=1))
        Hn = np.zeros((P, N + 1), np.int32)
        En = np.zeros((P, N + 1), np.int32)
        Fn = np.zeros((P, N + 1), np.int32)
        Hn[:, lo + 1:hi + 2] = H
        En[:, lo + 1:hi + 2] = E
        Fn[:, lo + 1:hi + 2] = F
        H2, H1, E1, F1 = H1, Hn, En, Fn
    return [int(x) for x in best]


def checker(a, b, table, gap_init, gap_ext, code=None):
    """One pair of byte strings (``code``: byte -> symbol index) or of symbol indices."""
    a = np.frombuffer(bytes(a), np.uint8) if isinstance(a, (bytes, bytearray)) else np.asarray(a)
    b = np.frombuffer(bytes(b), np.uint8) if isinstance(b, (bytes, bytearray)) else np.asarray(b)
    if code is not None:
        a, b = code[a], code[b]
        assert (a >= 0).all() and (b >= 0).all()
    return checker_batch([(a, b)], table, gap_init, gap_ext)[0]


def identity_table(k, match, mismatch):
    return np.where(np.eye(k, dtype=bool), match, mismatch).astype(np.int32)


def test_checker_small_cases():
    T = identity_table(4, 2, -1)
    assert checker([0, 1, 2, 3], [0, 1, 2, 3], T, 3, 1) == 8
    assert checker([0, 1, 2, 3], [3, 2, 1, 0], T, 3, 1) == 2
    assert checker([0, 1, 2, 3, 0, 1], [0, 1, 0, 1], T, 1, 1) == 2 + 2 - 2 + 2 + 2   # one gap of two residues
    assert checker([], [0], T, 1, 1) == 0
    # asymmetric: only (0 in seq1, 1 in seq2) scores
    U = np.full((2, 2), -5, np.int32)
    U[0, 1] = 7
    assert checker([0, 0], [1], U, 1, 1) == 7 and checker([1], [0, 0], U, 1, 1) == 0
    assert checker([1], [0, 0], U.T, 1, 1) == 7


@pytest.mark.parametrize("prm", [(1, -1, 1, 1), (2, -3, 5, 2)])
def test_checker_equals_oracle_on_identity_table(oracle_mod, prm):
    """Pins the checker to the reference-pinned oracle: on the identity table over the 20
    amino-acid letters it is oracle.score_linear."""
    rng = np.random.default_rng(11 + prm[0])
    code = byte_codes(AA.tobytes())
    T = identity_table(20, prm[0], prm[1])
    op = oracle_mod.Params(*prm)
    pairs = []
    for k in range(30):
        n, m = (int(x) for x in rng.integers(1, 201, 2))
        a = AA[rng.integers(0, 20, n)]
        b = AA[rng.integers(0, 20, m)]
        if k % 3 == 0:   # a mutated copy, so that gaps are taken
            b = np.delete(a, rng.integers(0, n, min(n - 1, 3)))
            b = np.concatenate([b, AA[rng.integers(0, 20, 2)]])
        pairs.append((a, b))
    got = checker_batch([(code[a], code[b]) for a, b in pairs], T, prm[2], prm[3])
    assert got == [oracle_mod.score_linear(a, b, op) for a, b in pairs]
    assert max(got) > 5


# ---- the parser ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sw():
    import concurrentproject_amd as sw
    sw.lib()
    return sw


def py_parse(text: bytes):
    """The format restated: '#' comment lines, a header line of symbols, K labelled rows of K
    integers, any run of blanks between tokens, CRLF accepted; '*' becomes `other`."""
    lines = [ln.split() for ln in text.replace(b"\r", b" ").split(b"\n")]
    lines = [ln for ln in lines if ln and not ln[0].startswith(b"#")]
    symbols = b"".join(lines[0])
    assert len(symbols) == len(lines[0]) == len(lines) - 1
    table = []
    for s, ln in zip(symbols, lines[1:]):
        assert ln[0] == bytes([s]) and len(ln) == len(symbols) + 1
        table.append([int(x) for x in ln[1:]])
    return symbols, np.array(table, dtype=np.int32), symbols.find(b"*")


def matrix_text(symbols: bytes, table, sep=b"  ", nl=b"\n", final_newline=True, comments=True):
    out = [b"# a test matrix", b"#  second comment line"] if comments else []
    out.append(b"   " + sep.join(bytes([s]) for s in symbols))
    for s, row in zip(symbols, table):
        out.append(bytes([s]) + sep + sep.join(b"%d" % v for v in row))
    return nl.join(out) + (nl if final_newline else b"")


def random_table(rng, k, symmetric=False):
    """Diagonal entries in [4, 11], off-diagonal in [-4, 3]."""
    T = rng.integers(-4, 4, (k, k)).astype(np.int32)
    if symmetric:
        T = np.triu(T) + np.triu(T, 1).T
    T[np.arange(k), np.arange(k)] = rng.integers(4, 12, k)
    return T


GOOD_TEXTS = {
    "plain": lambda T: matrix_text(b"ARNDCQEGHILKMFPSTWYVBZX*", T),
    "crlf": lambda T: matrix_text(b"ARNDCQEGHILKMFPSTWYVBZX*", T, nl=b"\r\n"),
    "tabs": lambda T: matrix_text(b"ARNDCQEGHILKMFPSTWYVBZX*", T, sep=b"\t \t"),
    "noeol": lambda T: matrix_text(b"ARNDCQEGHILKMFPSTWYVBZX*", T, final_newline=False),
    "nocomment": lambda T: b"\n\n" + matrix_text(b"ARNDCQEGHILKMFPSTWYVBZX*", T, comments=False) + b"\n  \n",
}


@pytest.mark.parametrize("name", sorted(GOOD_TEXTS))
def test_parse_matches_python(sw, name):
    rng = np.random.default_rng(5)
    T = random_table(rng, 24)          # asymmetric
    assert (T != T.T).any()
    text = GOOD_TEXTS[name](T)
    symbols, table, other = py_parse(text)
    assert (table == T).all() and other == 23
    with sw.Matrix.parse(text) as m:
        assert m.symbols == symbols
        for i, a in enumerate(symbols):
            for j, b in enumerate(symbols):
                assert m.score(bytes([a]), bytes([b])) == table[i, j]
        assert m.score(b"@", b"A") == table[other, 0]      # '*' is `other`
        assert m.score(b"A", b"a") == table[0, other]      # no case folding from a file


def test_open_file_and_small_matrices(sw, tmp_path):
    p = tmp_path / "m.txt"
    p.write_bytes(b"#c\nA C\nA 5 -3\nC -2 4")
    with sw.Matrix.open(p) as m:
        assert m.symbols == b"AC" and m.score(b"A", b"C") == -3 and m.score(b"C", b"A") == -2
        with pytest.raises(sw.SwError, match="0x47"):
            m.score(b"A", b"G")                              # no '*': outside the alphabet
    with sw.Matrix.parse(b"A\nA +127\n") as m:
        assert m.symbols == b"A" and m.score(b"A", b"A") == 127
    with pytest.raises(sw.SwError, match="cannot open"):
        sw.Matrix.open(tmp_path / "missing.txt")


MALFORMED = {
    "short_row": (b"A C\nA 1 2\nC 3\n", "not square"),
    "long_row": (b"A C\nA 1 2 3\nC 3 4\n", "not square"),
    "missing_row": (b"A C G\nA 1 2 3\nC 3 4 5\n", "not square"),
    "extra_row": (b"A C\nA 1 2\nC 3 4\nG 1 2\n", "not square"),
    "label": (b"A C\nA 1 2\nG 3 4\n", "row label"),
    "long_label": (b"A C\nA 1 2\nCC 3 4\n", "row label"),
    "duplicate": (b"A C A\nA 1 2 3\nC 1 2 3\nA 1 2 3\n", "duplicate symbol"),
    "too_many": (b" ".join(bytes([48 + i]) for i in range(33)) + b"\n", "at most 32"),
    "range_hi": (b"A C\nA 1 128\nC 3 4\n", r"outside \[-127, 127\]"),
    "range_lo": (b"A C\nA 1 2\nC -128 4\n", r"outside \[-127, 127\]"),
    "not_int": (b"A C\nA 1 x\nC 3 4\n", "not an integer"),
    "float": (b"A C\nA 1 2.5\nC 3 4\n", "not an integer"),
    "sign_only": (b"A C\nA 1 -\nC 3 4\n", "not an integer"),
    "huge": (b"A C\nA 1 99999999999999999999\nC 3 4\n", "not an integer"),
    "no_rows": (b"# only a header\nA C G\n", "no rows"),
    "empty": (b"", "no header"),
    "comments_only": (b"# nothing\n#\n", "no header"),
    "wide_symbol": (b"AB C\nA 1 2\nC 3 4\n", "one byte"),
}


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_is_an_error_with_a_message(sw, name):
    text, want = MALFORMED[name]
    with pytest.raises(sw.SwError, match=want):
        sw.Matrix.parse(text)


def test_create_errors(sw):
    with pytest.raises(sw.SwError, match="duplicate"):
        sw.Matrix(b"AA", [[1, 2], [3, 4]])
    with pytest.raises(sw.SwError, match="1 to 32"):
        sw.Matrix(bytes(range(65, 98)), np.zeros((33, 33)))
    with pytest.raises(sw.SwError, match="1 to 32"):
        sw.Matrix(b"", [])
    with pytest.raises(sw.SwError, match="other"):
        sw.Matrix(b"AC", [[1, 2], [3, 4]], other=2)
    with pytest.raises(sw.SwError, match="127"):
        sw.Matrix(b"AC", [[1, 200], [3, 4]])
    with pytest.raises(sw.SwError, match="not 2 x 2"):
        sw.Matrix(b"AC", [1, 2, 3])
    m = sw.Matrix(b"AC", [[1, 2], [3, 4]])
    m.close()
    m.close()
    with pytest.raises(sw.SwError, match="closed"):
        m.symbols


@pytest.mark.parametrize("other,fold", [(-1, False), (5, False), (-1, True), (7, True)])
def test_score_agrees_with_the_table_for_every_byte_pair(sw, other, fold):
    rng = np.random.default_rng(9)
    symbols = b"ARNDCQEGHILKMFPSTWYVx*q"      # 'x' and 'q' are symbols themselves: never folded onto
    T = random_table(rng, len(symbols))
    code = byte_codes(symbols, other, fold)
    if fold:
        assert code[ord("a")] == 0 and code[ord("x")] == symbols.index(b"x") and code[ord("b")] == other
    lib = sw.lib()
    import ctypes
    out = ctypes.c_int()
    with sw.Matrix(symbols, T, other=other, fold_case=fold) as m:
        for a in range(256):
            for b in range(256):
                rc = lib.sw_matrix_score(m._handle(), a, b, ctypes.byref(out))
                if code[a] < 0 or code[b] < 0:
                    assert rc == -1
                else:
                    assert rc == 0 and out.value == T[code[a], code[b]], (a, b)


# ---- the parser under the sanitizers ---------------------------------------------------------------

def test_matrix_parser_under_sanitizers(tmp_path):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "concurrentproject_amd", "csrc"), "asan-matrix"], check=True)
    exe = os.path.join(ROOT, "build", "asan", "matrix_parse_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    rng = np.random.default_rng(5)
    T = random_table(rng, 24)
    files = {}
    for name in sorted(GOOD_TEXTS):
        # every byte pair has a score: '*' takes the bytes outside the alphabet
        files["good_" + name] = (GOOD_TEXTS[name](T), "ok 24 %d 65536" % int(T.sum()))
    files["good_small"] = (b"A C\nA 5 -3\nC -2 4", "ok 2 4 4")
    for name in sorted(MALFORMED):
        files["bad_" + name] = (MALFORMED[name][0], "error ")
    files["bad_binary"] = (bytes(rng.integers(0, 256, 4096, dtype=np.uint8)), "error ")
    files["bad_long_line"] = (b"A C\nA " + b"1 " * 100000 + b"\n", "error ")
    files["bad_long_token"] = (b"A C\nA 1 " + b"7" * 100000 + b"\nC 1 2\n", "error ")
    files["bad_nul"] = (b"A C\nA 1 \x00\nC 1 2\n", "error ")
    paths = []
    for name, (data, _) in files.items():
        p = tmp_path / name
        p.write_bytes(data)
        paths.append(str(p))
    paths.append(str(tmp_path / "does_not_exist"))
    r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(files) + 1
    for (name, (_, want)), line in zip(files.items(), lines):
        assert line.startswith(want), (name, line)
        assert "MISMATCH" not in line and len(line) > len("error "), (name, line)
    assert lines[-1].startswith("error cannot open")

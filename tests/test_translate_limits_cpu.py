"""Translated search at the limits of its declared domain, host side, no GPU: the yardsticks that
tests/test_translate_limits.py leans on, shown to hold where that file uses them, and its shared inputs.

The reference of both files is the plain restatements -- `check_many` (local), `restate` (global, semi-global)
-- over `py_translate(dna, frame, code)` of tests/test_translate_cpu.py: a str, a dict and a reverse, sharing
no code with the library.  (One byte is taken out of py_translate's way: str.upper() turns 0xdf into "SS",
two characters, so `sane` replaces 0xdf by '?' first -- neither is a base.)

The inputs: CODE_ALL32, a genetic code over SYM32 that emits all 32 symbols, the last one for codon 0 (TTT)
and codon 63 (GGG); CODE_STRANGE, which emits bytes 0x00, 0xff and '*', all outside SYM32, for `other` = 31; a
31-symbol matrix without 'X' under `other` = 30, so that ambiguous codons land on its last row; `any_dna`, in
which every one of the 256 byte values occurs; `dense_dna`, unambiguous bases in both cases with U and u; and
the range-edge cases: four shapes with L = 3m + 2 (six frames of the same m) and one with L = 3m, gap penalties
one unit inside the mode bound.

1. sw_translated_tables under each (matrix, code) against a table composed here, all 256 + 65 entries;
2. sw_translate against py_translate on any_dna and dense_dna in the six frames under the three codes;
3. sw_align_matrix_translated_cpu against the reference in the three modes: on a short grid, under the strange
   code and the no-'X' matrix, at local gap penalties of 2^20 and at every range-edge case."""
import ctypes

import numpy as np
import pytest

from test_matrix_cpu import byte_codes
from test_matrix import check_many
from test_align_cpu import rescore
from test_modes_cpu import check_shape, rescore_ops, restate
from test_matrix_limits_cpu import BIG_GAPS, FULL32, LAST, S32, SYM32, as_tuple, edge_u, rand32
from test_translate_cpu import FRAMES, planted_dna, py_translate, revcomp

MODES = ("local", "global", "semiglobal")
RANGE_MESSAGE = "pair 0: score range exceeds the int32 engine in this mode"
BASES = np.frombuffer(b"ACGT", np.uint8)


def _code_all32():
    rng = np.random.default_rng(6100)
    rest = np.concatenate([S32[:31], S32[:31]])[rng.permutation(62)]
    return bytes([LAST]) + rest.tobytes() + bytes([LAST])


def _code_strange():
    c = bytearray(CODE_ALL32)
    c[5], c[21], c[40], c[58] = 0x00, 0xFF, ord("*"), 0x00
    return bytes(c)


CODE_ALL32 = _code_all32()
CODE_STRANGE = _code_strange()
SYM31 = SYM32.replace(b"X", b"")
FULL31 = np.ascontiguousarray(np.delete(np.delete(FULL32, 23, 0), 23, 1))
# name -> (symbols, table, other, genetic code): the three settings both files run
SETTINGS = {"all32": (SYM32, FULL32, -1, CODE_ALL32), "strange": (SYM32, FULL32, 31, CODE_STRANGE),
            "no_x": (SYM31, FULL31, 30, CODE_ALL32)}


def setting(name):
    """(symbols, table, other, code bytes, code str for py_translate, byte -> row map)."""
    sym, T, other, code = SETTINGS[name]
    return sym, T, other, code, code.decode("latin-1"), byte_codes(sym, other)


@pytest.fixture(scope="module")
def sw():
    import concurrentproject_amd as sw
    sw.lib()
    return sw


# ---- the inputs ---------------------------------------------------------------------------------------

def any_dna(rng, L):
    """L >= 600 bytes: bases, and every one of the 256 byte values at a place of its own."""
    d = BASES[rng.integers(0, 4, L)].copy()
    d[rng.permutation(L)[:256]] = np.arange(256, dtype=np.uint8)
    return d


def dense_dna(rng, L):
    """Unambiguous bases only: both cases, U and u for some T."""
    return np.frombuffer(b"ACGTUacgtu", np.uint8)[rng.integers(0, 10, L)]


def sane(d) -> bytes:
    return bytes(d).replace(b"\xdf", b"?")


def frames_of(d, code: str):
    """The six frames by py_translate, as arrays."""
    return [np.frombuffer(py_translate(sane(d), f, code), np.uint8) for f in FRAMES]


_cache = {}


def cached(key, make):
    """An input or a reference: computed once, shared among the tests of both files, never changed."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def empty_answer(n, go, ge):
    """A frame without a residue in a mode: the query as one gap run (tests/test_modes_cpu.py::test_empty_sequences)."""
    return (-(go + (n - 1) * min(go, ge)), 0, n, 0, 0, ((n, "I"),))


def reference(key, pairs, name, gaps, mode):
    """Per pair the six frames' answers: local, the scores of check_many; in a mode, restate's tuples."""
    def make():
        sym, T, other, code, code_str, rows = setting(name)
        flat = [(q, fr) for q, d in pairs for fr in frames_of(d, code_str)]
        if mode == "local":
            got = check_many(flat, T, *gaps, rows)
        else:
            got = [restate(q, fr, T, *gaps, mode, rows) if len(fr) else empty_answer(len(q), *gaps) for q, fr in flat]
        return tuple(tuple(got[6 * k:6 * k + 6]) for k in range(len(pairs)))
    return cached(("ref", key, name, gaps, mode), make)


def ref_scores(ref):
    return np.array([[w[0] if isinstance(w, tuple) else w for w in six] for six in ref], dtype=np.int64)


EDGE_SHAPES = [(513, 65), (130, 1025), (1025, 1), (1, 1025)]      # (query residues, residues a frame)
EDGE_CASES = [(n, m, 3 * m + 2) for n, m in EDGE_SHAPES] + [(513, 65, 195)]   # the last: frames of 65, 64, 64


def edge_gaps(n, m):
    u = edge_u(n, m)
    return [(u, u), (u, 1), (1, u), (0, u), (u, 0)]


def edge_pairs(case):
    """One (query, dna): a mutated copy of the query planted under CODE_ALL32, with N, lower case and U sprinkled in."""
    def make():
        n, m, L = case
        rng = np.random.default_rng(6300 + EDGE_CASES.index(case))
        q = rand32(rng, n)
        q[int(rng.integers(0, n))] = LAST
        return [(q, planted_dna(rng, q, L, CODE_ALL32.decode("latin-1")))]
    return cached(("edge", case), make)


def short_grid(name):
    """Queries of 1 to 100 residues against DNAs of 0 to 450 bytes: planted, dense, and (from 600 on) any_dna."""
    def make():
        rng = np.random.default_rng(6200)
        code_str = SETTINGS[name][3].decode("latin-1")
        sym = np.frombuffer(SETTINGS[name][0], np.uint8)
        pairs = []
        for k, L in enumerate([0, 2, 3, 4, 5, 6, 8, 189, 191, 192, 193, 194, 195, 391, 450, 700, 905]):
            q = sym[rng.integers(0, len(sym), int(rng.choice([1, 5, 40, 64, 100])))]
            d = any_dna(rng, L) if L >= 600 else planted_dna(rng, q, L, code_str) if k % 2 else dense_dna(rng, L)
            pairs.append((q, d))
        return pairs
    return cached(("short", name), make)


# ---- 1. the composed tables -----------------------------------------------------------------------------

def test_inputs():
    assert len(CODE_ALL32) == 64 and set(CODE_ALL32) == set(SYM32) and CODE_ALL32[0] == CODE_ALL32[63] == LAST
    assert {0x00, 0xFF, ord("*")} <= set(CODE_STRANGE) and not {0x00, 0xFF, ord("*")} & set(SYM32)
    assert len(SYM31) == 31 and b"X" not in SYM31 and FULL31.shape == (31, 31) and FULL31[30, 30] == FULL32[31, 31]
    rng = np.random.default_rng(1)
    assert sorted(set(any_dna(rng, 600).tolist())) == list(range(256))
    assert set(dense_dna(rng, 500).tobytes()) == set(b"ACGTUacgtu")
    for n, m, L in EDGE_CASES:
        assert [len(fr) for fr in frames_of(edge_pairs((n, m, L))[0][1], "A" * 64)] == ([m] * 6 if L % 3 else [m, m - 1, m - 1] * 2)
        assert (n + m + 1024) * edge_u(n, m) < (1 << 28) <= (n + m + 1024) * (edge_u(n, m) + 1)


@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_composed_tables(sw, name):
    sym, T, other, code, code_str, rows = setting(name)
    base = (ctypes.c_ubyte * 256)()
    codon = (ctypes.c_ubyte * 65)()
    c64 = (ctypes.c_ubyte * 64)(*code)
    with sw.Matrix(sym, T, other=other) as mx:
        assert sw.lib().sw_translated_tables(mx._handle(), c64, base, codon) == 0
    want = np.full(256, 4)
    for cls, letters in enumerate(("TtUu", "Cc", "Aa", "Gg")):
        want[[ord(x) for x in letters]] = cls
    assert list(base) == list(want)
    assert list(codon) == [int(rows[b]) for b in code + b"X"]
    assert len(sym) - 1 in list(codon)                     # the last row is reached
    if name != "all32":
        assert sum(b not in sym for b in code + b"X") >= 1 and list(codon).count(other) >= 3   # only `other` covers them
    with sw.Matrix(sym, T) as mx:                             # other = -1
        rc = sw.lib().sw_translated_tables(mx._handle(), c64, base, codon)
        assert rc == (0 if name == "all32" else -1)
        if name == "strange":
            assert b"the genetic code emits byte 0x00 ('?', codon 5)" in sw.lib().sw_last_error()
        if name == "no_x":
            assert b"the genetic code emits byte 0x58 ('X'" in sw.lib().sw_last_error()


# ---- 2. translate ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frame", FRAMES)
def test_translate_any_byte(sw, frame):
    rng = np.random.default_rng(6110 + frame)
    for L in (600, 601, 602, 905, 3302):
        for d in (any_dna(rng, L), dense_dna(rng, L)):
            for code in (None, CODE_ALL32, CODE_STRANGE):
                want = py_translate(sane(d), frame, *([code.decode("latin-1")] if code else []))
                assert sw.translate(d, frame, code) == want, (L, frame)
                assert len(want) == (L - abs(frame) + 1) // 3
    d = dense_dna(rng, 3000)
    got = sw.translate(d, frame, CODE_ALL32)
    assert set(got) == set(SYM32) and got.count(b"X") < 200 < sw.translate(any_dna(rng, 3000), frame, CODE_ALL32).count(b"X")


# ---- 3. the CPU aligner over translated frames -----------------------------------------------------------------

def against_the_reference(sw, pairs, name, gaps, mode, ref, got=None):
    """align_matrix_translated_batch(cpu=True) -- or `got`, six alignments a pair -- against `reference`."""
    sym, T, other, code, code_str, rows = setting(name)
    if got is None:
        flat = [p for p in pairs for _ in FRAMES]
        with sw.Matrix(sym, T, other=other) as mx:
            got = sw.align_matrix_translated_batch(flat, list(FRAMES) * len(pairs), mx, *gaps, cpu=True, mode=mode, code=code)
    assert len(got) == 6 * len(pairs)
    for k, (q, d) in enumerate(pairs):
        for fi, (f, prot) in enumerate(zip(FRAMES, frames_of(d, code_str))):
            g, w = got[6 * k + fi], ref[k][fi]
            assert g.frame == f
            if mode == "local":
                assert g.score == w, (name, gaps, k, f, g, w)
                assert rescore(g, q, prot, T, *gaps, rows) == g.score
            else:
                assert as_tuple(g) == w, (name, mode, gaps, k, f, g, w)
                assert rescore_ops(g, q, prot, T, *gaps, rows) == g.score
                check_shape(g, q, prot, mode)
            check_dna_range(sw, g, d, prot, code_str)
    return got


def check_dna_range(sw, g, d, prot, code_str):
    """dna_beg / dna_end: sw_translated_range's, and the piece translated again gives the residues aligned."""
    assert (g.dna_beg, g.dna_end) == sw.translated_range(len(d), g.frame, g.beg2, g.end2)
    assert 0 <= g.dna_beg <= g.dna_end <= len(d) and g.dna_end - g.dna_beg == 3 * (g.end2 - g.beg2)
    piece = np.asarray(d)[g.dna_beg:g.dna_end]
    assert py_translate(sane(piece if g.frame > 0 else revcomp(piece)), 1, code_str) == prot[g.beg2:g.end2].tobytes()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_cpu_aligner_on_the_short_grid(sw, name, mode):
    pairs = short_grid(name)
    for gaps in ((12, 1), (0, 0), (127, 127)):
        ref = reference(("short", name), pairs, name, gaps, mode)
        got = against_the_reference(sw, pairs, name, gaps, mode, ref)
        assert any(g.frame < 0 and g.end2 > g.beg2 for g in got)
    assert ref_scores(reference(("short", name), pairs, name, (12, 1), mode)).max() > 1000


@pytest.mark.parametrize("gaps", BIG_GAPS)
def test_local_cpu_aligner_at_large_gaps(sw, gaps):
    pairs = short_grid("all32")
    against_the_reference(sw, pairs, "all32", gaps, "local", reference(("short", "all32"), pairs, "all32", gaps, "local"))


@pytest.mark.parametrize("mode", ["global", "semiglobal"])
@pytest.mark.parametrize("case", EDGE_CASES, ids=lambda c: "%dx%d-L%d" % c)
def test_cpu_aligner_at_the_range_edge(sw, case, mode):
    n, m, L = case
    pairs = edge_pairs(case)
    u = edge_u(n, m)
    for gaps in edge_gaps(n, m):
        against_the_reference(sw, pairs, "all32", gaps, mode, reference(("edge", case), pairs, "all32", gaps, mode))
    if mode == "global":
        assert ref_scores(reference(("edge", case), pairs, "all32", (u, u), mode)).min() < -(1 << 24)
    with sw.Matrix(SYM32, FULL32) as mx:
        for gaps in ((u + 1, 1), (1, u + 1)):               # one unit more is refused
            with pytest.raises(sw.SwError, match=RANGE_MESSAGE):
                sw.align_matrix_translated_batch(pairs, [-3], mx, *gaps, cpu=True, mode=mode, code=CODE_ALL32)

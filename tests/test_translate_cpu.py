"""Translated search, host side (include/algoGPU.h sw_translate, sw_translated_range, sw_translated_tables,
sw_align_matrix_translated_cpu; csrc/sw_matrix_host.cpp, csrc/sw_align_host.cpp), no GPU:

* `translate` against a plain-Python restatement written here (a dict from the 64-byte string, str reverse and
  complement), all six frames, with N, lower case and U sprinkled in -- tests/test_translate.py imports the
  restatement and the DNA generators from here;
* the standard code pinned by its invariants (no copy of NCBI's table is on the build machines): the residue
  multiplicities, ATG = M, TGG = W, the three stops;
* sw_translated_range: the bases it names, translated on their own, are the residues asked for;
* the composed tables against the matrix's own byte-to-code map;
* align_matrix_translated_batch(cpu=True) = align_matrix_batch(cpu=True) on the translated frame plus the range;
* the refusals, by name; the exports; the host code under AddressSanitizer + UndefinedBehaviorSanitizer in a
  stand-alone program (tests/asan/translate_driver.cpp, `make -C concurrentproject_amd/csrc asan-translate`)."""
import collections
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_matrix_cpu import random_table
from test_matrix import SYMBOLS, mutated_copy, rand_seq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("local", "global", "semiglobal")
FRAMES = (1, 2, 3, -1, -2, -3)
STANDARD = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
CPU_LENGTHS = list(range(0, 9)) + list(range(189, 198)) + [391, 905]


@pytest.fixture(scope="module")
def sw():
    import concurrentproject_amd as sw
    sw.lib()
    return sw


@pytest.fixture(scope="module")
def table():
    return random_table(np.random.default_rng(24), 24)


# ---- the restatement and the test DNA ---------------------------------------------------------------

def py_translate(dna: bytes, frame: int, code: str = STANDARD) -> bytes:
    """Plain Python: upper-case, U as T, the reverse complement as a str for a minus frame, then codon by codon
    through a dict; a codon with any other letter is X."""
    table = {a + b + c: code[16 * i + 4 * j + k] for i, a in enumerate("TCAG") for j, b in enumerate("TCAG")
             for k, c in enumerate("TCAG")}
    s = dna.decode("latin-1").upper().replace("U", "T")
    if frame < 0:
        s = s[::-1].translate(str.maketrans("ACGT", "TGCA"))   # other letters stay: still not a base
    o = abs(frame) - 1
    return "".join(table.get(s[i:i + 3], "X") for i in range(o, len(s) - 2, 3)).encode("latin-1")


def sprinkle(rng, dna: np.ndarray, rate=0.02) -> np.ndarray:
    """About `rate` of the bases replaced by N, by their lower case, or (T) by U / u."""
    d = dna.copy()
    hit = np.flatnonzero(rng.random(len(d)) < rate)
    for i in hit:
        kind = int(rng.integers(0, 3))
        if kind == 0:
            d[i] = ord("N") if rng.random() < 0.8 else ord("n")
        elif kind == 1:
            d[i] = d[i] | 0x20
        else:
            d[i] = rng.choice([ord("U"), ord("u")]) if d[i] == ord("T") else d[i] | 0x20
    return d


def rand_dna(rng, n, rate=0.02) -> np.ndarray:
    return sprinkle(rng, np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)], rate)


def back_translate(rng, protein, code: str = STANDARD) -> np.ndarray:
    """A DNA whose frame +1 is `protein` (a random codon of each residue; a residue the code never emits gets a
    random codon)."""
    by_aa = collections.defaultdict(list)
    for i, a in enumerate("TCAG"):
        for j, b in enumerate("TCAG"):
            for k, c in enumerate("TCAG"):
                by_aa[ord(code[16 * i + 4 * j + k])].append(a + b + c)
    every = [c for v in by_aa.values() for c in v]
    out = "".join(str(rng.choice(by_aa.get(int(r), every))) for r in protein)
    return np.frombuffer(out.encode(), np.uint8)


def revcomp(dna: np.ndarray) -> np.ndarray:
    comp = np.arange(256, dtype=np.uint8)
    comp[np.frombuffer(b"ACGTUacgtu", np.uint8)] = np.frombuffer(b"TGCAAtgcaa", np.uint8)
    return np.ascontiguousarray(comp[dna[::-1]])


def planted_dna(rng, protein, length, code: str = STANDARD, rate=0.02) -> np.ndarray:
    """`length` bases: a back-translated mutated copy of `protein` in a random frame and strand between random
    flanks (cut to `length` when it is too short for all of it)."""
    gene = back_translate(rng, mutated_copy(rng, np.asarray(protein), max(1, min(len(protein), length // 3))), code)
    if rng.random() < 0.5:
        gene = revcomp(gene)
    lead = int(rng.integers(0, max(1, length - len(gene) + 1)))
    d = np.concatenate([rand_dna(rng, lead, 0), gene, rand_dna(rng, max(0, length - lead - len(gene)), 0)])[:length]
    return sprinkle(rng, np.ascontiguousarray(d), rate)


# ---- translate ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frame", FRAMES)
def test_translate_matches_python(sw, frame):
    rng = np.random.default_rng(100 + frame)
    for L in CPU_LENGTHS:
        for rate in (0.0, 0.02, 0.3):
            d = rand_dna(rng, L, rate).tobytes()
            got = sw.translate(d, frame)
            assert got == py_translate(d, frame), (L, frame, rate)
            o = abs(frame) - 1
            assert len(got) == ((L - o) // 3 if L >= o + 3 else 0)
    shuffled = "".join(np.random.default_rng(7).permutation(list(STANDARD)))
    d = rand_dna(rng, 905).tobytes()
    assert sw.translate(d, frame, code=shuffled.encode()) == py_translate(d, frame, shuffled)
    assert sw.translate(b"CTN" + b"ctg" + b"UUU" + b"AT-", 1) == b"XLFX"     # degenerate codons are not resolved


def test_standard_code(sw):
    assert sw.STANDARD_CODE == STANDARD.encode()
    out = (ctypes.c_ubyte * 64)()
    sw.lib().sw_standard_code(out)
    assert bytes(out) == STANDARD.encode()
    want = dict.fromkeys("LSR", 6)
    want.update(dict.fromkeys("AGPTV", 4))
    want.update(dict.fromkeys("I*", 3))
    want.update(dict.fromkeys("FYHQNKDEC", 2))
    want.update(dict.fromkeys("MW", 1))
    assert collections.Counter(STANDARD) == want and sum(want.values()) == 64
    assert sw.translate(b"ATG", 1) == b"M" and sw.translate(b"TGG", 1) == b"W"
    assert sw.translate(b"TAATAGTGA", 1) == b"***"
    assert sw.translate(b"CAT", -1) == b"M"                                   # the reverse complement of ATG


def test_translated_range(sw):
    rng = np.random.default_rng(3)
    for _ in range(400):
        L = int(rng.choice([0, 2, 3, 4, 5, 7, 64, 191, 192, 193, 600]))
        frame = int(rng.choice(FRAMES))
        d = rand_dna(rng, L, 0.05)
        prot = sw.translate(d, frame)
        m = len(prot)
        beg2 = int(rng.integers(0, m + 1))
        end2 = int(rng.integers(beg2, m + 1))
        lo, hi = sw.translated_range(L, frame, beg2, end2)
        assert 0 <= lo <= hi <= L and hi - lo == 3 * (end2 - beg2)
        piece = d[lo:hi]
        if frame < 0:
            piece = revcomp(piece)
        assert py_translate(piece.tobytes(), 1) == prot[beg2:end2], (L, frame, beg2, end2)
    with pytest.raises(sw.SwError, match="sw_translated_range: residues .* are outside frame"):
        sw.translated_range(10, 1, 0, 4)
    with pytest.raises(ValueError, match="frame 0"):
        sw.translated_range(10, 0, 0, 1)


def test_composed_tables(sw, table):
    base = (ctypes.c_ubyte * 256)()
    codon = (ctypes.c_ubyte * 65)()
    with sw.Matrix(SYMBOLS, table) as mx:
        assert sw.lib().sw_translated_tables(mx._handle(), None, base, codon) == 0
    want = np.full(256, 4)
    for cls, letters in enumerate(("TtUu", "Cc", "Aa", "Gg")):
        want[[ord(x) for x in letters]] = cls
    assert list(base) == list(want)
    assert [SYMBOLS[c] for c in codon] == list((STANDARD + "X").encode())


# ---- the CPU aligner ------------------------------------------------------------------------------------

def cpu_cases():
    rng = np.random.default_rng(17)
    pairs, frames = [], []
    for k, L in enumerate(CPU_LENGTHS + [300, 450]):
        n = int(rng.choice([1, 5, 40, 64, 100]))
        q = rand_seq(rng, n, 20)
        d = planted_dna(rng, q, L) if k % 2 else rand_dna(rng, L)
        for f in FRAMES if L in (0, 2, 4, 5, 193, 391) else (FRAMES[k % 6],):
            pairs.append((q, d))
            frames.append(f)
    pairs.append((np.zeros(0, np.uint8), rand_dna(rng, 30)))
    frames.append(-2)
    return pairs, frames


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gaps", [(12, 1), (1, 3), (0, 0)])
def test_cpu_aligner_is_the_matrix_aligner_on_the_frame(sw, table, mode, gaps):
    pairs, frames = cpu_cases()
    with sw.Matrix(SYMBOLS, table) as mx:
        got = sw.align_matrix_translated_batch(pairs, frames, mx, *gaps, cpu=True, mode=mode)
        want = sw.align_matrix_batch([(q, sw.translate(d, f)) for (q, d), f in zip(pairs, frames)], mx, *gaps, cpu=True,
                                     mode=mode)
    assert len(got) == len(want) == len(pairs)
    for g, w, (q, d), f in zip(got, want, pairs, frames):
        assert (g.score, g.beg1, g.end1, g.beg2, g.end2, g.ops) == (w.score, w.beg1, w.end1, w.beg2, w.end2, w.ops)
        assert g.frame == f and (g.dna_beg, g.dna_end) == sw.translated_range(len(d), f, g.beg2, g.end2)
        assert g.columns(q, sw.translate(d, f)) == w.columns(q, sw.translate(d, f))
    assert any(g.score > 20 for g in got) and any(g.end2 > g.beg2 and g.frame < 0 for g in got)


# ---- refusals, exports ----------------------------------------------------------------------------------

def _raw_align_cpu(sw, mx, q, dna_len, frame, dna=b"ACGTACGT"):
    """sw_align_matrix_translated_cpu called directly, with a DNA length the buffer need not have."""
    L = sw.lib()
    u8p = ctypes.POINTER(ctypes.c_ubyte)
    qa, da = np.frombuffer(q, np.uint8), np.frombuffer(dna, np.uint8)
    A = (u8p * 1)(qa.ctypes.data_as(u8p))
    D = (u8p * 1)(da.ctypes.data_as(u8p))
    out = (sw._Alignment * 1)()
    used = ctypes.c_longlong()
    cig = (ctypes.c_uint * 16)()
    rc = L.sw_align_matrix_translated_cpu(mx._handle(), A, (ctypes.c_int * 1)(len(q)), D, (ctypes.c_int * 1)(dna_len),
                                          (ctypes.c_int * 1)(frame), 1, 12, 1, 0, None, out, cig, 16, ctypes.byref(used))
    return rc, L.sw_last_error().decode()


def test_refusals_by_name(sw, table):
    q, d = b"ARND", b"GCTCGTAACGAT"
    no_star, no_x = SYMBOLS[:23], SYMBOLS[:22] + b"*"
    for call in ("sw_align_matrix_translated_cpu",):
        with sw.Matrix(no_star, table[:23, :23]) as mx:
            with pytest.raises(sw.SwError, match=call + r": the genetic code emits byte 0x2a \('\*'"):
                sw.align_matrix_translated(q, d, 1, mx, 12, 1, cpu=True)
        with sw.Matrix(no_x, table[:23, :23]) as mx:
            with pytest.raises(sw.SwError, match=call + r": a codon with an ambiguous base translates to byte 0x58"):
                sw.align_matrix_translated(q, d, 1, mx, 12, 1, cpu=True)
    with sw.Matrix(no_star, table[:23, :23], other=0) as mx:      # covered by `other`: accepted
        assert sw.align_matrix_translated(q, d, 1, mx, 12, 1, cpu=True).score > 0
    with sw.Matrix(SYMBOLS, table) as mx:
        for bad in (0, 4, -4):
            with pytest.raises(ValueError, match="frame %d is not one of" % bad):
                sw.align_matrix_translated(q, d, bad, mx, 12, 1, cpu=True)
            rc, err = _raw_align_cpu(sw, mx, q, 8, bad)
            assert rc == -1 and ("sw_align_matrix_translated_cpu: pair 0: frame %d is not one of" % bad) in err
        with pytest.raises(ValueError, match="a genetic code is 64 bytes"):
            sw.align_matrix_translated(q, d, 1, mx, 12, 1, cpu=True, code=STANDARD[:63].encode())
        with pytest.raises(ValueError, match="a genetic code is 64 bytes"):
            sw.translate(d, 1, code=b"")
        rc, err = _raw_align_cpu(sw, mx, q, 1 << 27, 1)           # refused before a byte of it is read
        assert rc == -1 and "sw_align_matrix_translated_cpu: pair 0: a length of 4 residues / 134217728 bases" in err
        with pytest.raises(sw.SwError, match="sw_align_matrix_translated_cpu: pair 0: seq1 position 1: byte 0x6f"):
            sw.align_matrix_translated(b"Ao", d, 1, mx, 12, 1, cpu=True)
        with pytest.raises(ValueError, match="unknown alignment mode"):
            sw.align_matrix_translated(q, d, 1, mx, 12, 1, cpu=True, mode="banded")
        assert sw.align_matrix_translated_batch([], [], mx, 12, 1, cpu=True) == []
        with pytest.raises(ValueError, match="1 frames for 2 pairs"):
            sw.align_matrix_translated_batch([(q, d), (q, d)], [1], mx, 12, 1, cpu=True)
    rc = sw.lib().sw_translate(None, 5, 1, None, None, 0)
    assert rc == -1 and b"sw_translate: invalid arguments" in sw.lib().sw_last_error()
    out = (ctypes.c_ubyte * 1)()
    rc = sw.lib().sw_translate((ctypes.c_ubyte * 9)(*b"ATGATGATG"), 9, 1, None, out, 1)
    assert rc == -1 and b"sw_translate: 3 residues do not fit the output buffer of 1" in sw.lib().sw_last_error()


def test_exports(sw):
    L = ctypes.CDLL(sw.LIB_PATH)
    for name in ("sw_standard_code", "sw_translate", "sw_translated_range", "sw_translated_tables",
                 "sw_score_matrix_translated_batch", "sw_align_matrix_translated_batch", "sw_align_matrix_translated_cpu",
                 "sw_db_search_matrix_translated", "sw_db_align_matrix_translated"):
        assert hasattr(L, name), name
        assert name + "(" in open(os.path.join(ROOT, "include", "algoGPU.h")).read()
    for name in ("STANDARD_CODE", "translate", "score_matrix_translated", "score_matrix_translated_batch",
                 "align_matrix_translated", "align_matrix_translated_batch", "TranslatedAlignment"):
        assert name in sw.__all__ and hasattr(sw, name), name
    for name in ("search_translated", "align_translated", "top_translated"):
        assert hasattr(sw.Database, name), name


def test_align_command_line_refusals(sw, capsys):
    from concurrentproject_amd import align
    for extra, msg in ((["--translate"], "--translate requires --matrix"),
                       (["--translate", "--matrix", "m", "--gaps", "12,1", "--alignments", "--long"], "not with --long"),
                       (["--translate", "--matrix", "m", "--gaps", "12,1", "--alignments", "--long", "--coop"], "not with --long")):
        with pytest.raises(SystemExit):
            align.main(["--query", "q", "--db", "d"] + extra)
        assert msg in capsys.readouterr().err


# ---- the host code under the sanitizers -----------------------------------------------------------------

def test_translate_under_sanitizers():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "concurrentproject_amd", "csrc"), "asan-translate"], check=True)
    exe = os.path.join(ROOT, "build", "asan", "translate_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, "11"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]
    assert r.stdout.startswith("ok "), r.stdout

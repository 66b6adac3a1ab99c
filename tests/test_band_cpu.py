"""Banded alignment, host side (include/algoGPU.h sw_*_band: sw_align_matrix_cpu_band, sw_band_plan;
csrc/sw_align_host.cpp), no GPU.

The yardstick is `restate_band` below: the banded recurrence written out again over float matrices,
one anti-diagonal at a time, with -inf outside the band and for the borders' E and F (local mode:
H = 0 outside the band).  It shares no constant and no code with the library and returns the score
and the end cell of each mode.

1. `align_matrix_batch(cpu=True, band=)` against it: n, m from {1, 2, 63, 64, 65, 130}, B from
   {0, 1, 5, 64, 200}, gaps (12,1), (0,0), (1,3), (5,0), random pairs and mutated copies, the three
   modes; every alignment re-scored from its operations, every aligned column in the band, global
   alignments covering both sequences;
2. the condition that keeps (1) from being vacuous: in each mode at least a quarter of the pairs
   with B <= 5 score strictly below their unbanded score, and a pair has B = 0 with n != m;
3. B >= max(n, m) equals cpu=True without a band, all three modes;
4. band_plan: dlo and dhi by the formula, cells against a brute-force count, the trace of
   (60000, 60000, 500) below the whole matrix's, monotone in B;
5. refusals: band=-1 (by the function's name), band with long=True;
6. the stand-alone sanitizer driver (make asan-align-band)."""
import os
import subprocess

import numpy as np
import pytest

from test_matrix_cpu import random_table
from test_matrix import CODE, SYMBOLS, mutated_copy, rand_seq
from test_modes_cpu import rescore_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (1, 2, 63, 64, 65, 130)
BANDS = (0, 1, 5, 64, 200)
GAPS = [(12, 1), (0, 0), (1, 3), (5, 0)]
MODES = ("local", "global", "semiglobal")
INF = float("inf")


@pytest.fixture(scope="module")
def sw():
    import concurrentproject_amd as sw
    sw.lib()
    return sw


# ---- the restatement --------------------------------------------------------------------------------

def band_range(n, m, B):
    return min(0, m - n) - B, max(0, m - n) + B


def restate_band(a, b, table, go, ge, mode, B, code=CODE):
    """(score, end i, end j) of seq1 = a (index i) against seq2 = b (index j) within band B (None: the
    whole matrix); matrices are indexed [i + 1][j + 1], row / column 0 the border.  Local: (0, 0, 0)
    when nothing scores."""
    ca, cb = code[np.asarray(a)], code[np.asarray(b)]
    n, m = len(ca), len(cb)
    assert n > 0 and m > 0
    dlo, dhi = band_range(n, m, B) if B is not None else (-n, m)
    gx = min(ge, go)
    S = np.asarray(table, np.float64)[ca][:, cb]
    local = mode == "local"
    H = np.full((n + 1, m + 1), 0.0 if local else -INF)   # outside the band: no cell
    E = np.full((n + 1, m + 1), -INF)
    F = np.full((n + 1, m + 1), -INF)
    T = np.full((n, m), -INF)                              # the diagonal arrivals (local end rule)
    if not local:
        H[0, 0] = 0
        H[1:, 0] = -(go + np.arange(n) * gx)
        H[0, 1:] = -(go + np.arange(m) * gx) if mode == "global" else 0
    for d in range(n + m - 1):
        I = np.arange(max(0, d - m + 1), min(n - 1, d) + 1)
        J = d - I
        keep = (J - I >= dlo) & (J - I <= dhi)
        I, J = I[keep], J[keep]
        if len(I) == 0:
            continue
        E[I + 1, J + 1] = np.maximum(E[I, J + 1] - ge, H[I, J + 1] - go)
        F[I + 1, J + 1] = np.maximum(F[I + 1, J] - ge, H[I + 1, J] - go)
        T[I, J] = H[I, J] + S[I, J]
        h = np.maximum(T[I, J], np.maximum(E[I + 1, J + 1], F[I + 1, J + 1]))
        H[I + 1, J + 1] = np.maximum(h, 0) if local else h
    if local:
        best = T.max()
        if best <= 0:
            return 0, 0, 0
        ii, jj = np.nonzero(T == best)
        k = np.lexsort((jj, ii + jj))[0]                   # the smallest i + j, then the smallest j
        return int(best), int(ii[k]), int(jj[k])
    if mode == "global":
        assert dlo <= (m - 1) - (n - 1) <= dhi
        return int(H[n, m]), n - 1, m - 1
    col = H[n, 1:]
    ej = int(np.argmax(col))                               # the first maximum: the smallest j
    assert np.isfinite(col[ej]) and dlo <= ej - (n - 1) <= dhi
    return int(col[ej]), n - 1, ej


def columns_in_band(al, n, m, B):
    """Every cell the alignment's operations stand on lies in the band (a leading gap run stands on
    a border, which is no cell)."""
    dlo, dhi = band_range(n, m, B)
    i, j = al.beg1, al.beg2
    for k, op in al.ops:
        for _ in range(k):
            if op == "M":
                ci, cj = i, j
                i, j = i + 1, j + 1
            elif op == "I":
                ci, cj = i, j - 1
                i += 1
            else:
                ci, cj = i - 1, j
                j += 1
            if ci >= 0 and cj >= 0:
                assert ci < n and cj < m and dlo <= cj - ci <= dhi, (al, ci, cj, dlo, dhi)
    return True


@pytest.fixture(scope="module")
def table():
    return random_table(np.random.default_rng(124), 24)


@pytest.fixture(scope="module")
def band_pairs():
    """One pair for every (n, m) of LENGTHS x LENGTHS, alternately random and a mutated copy; and for
    every (n, m) with both at least 63 a copy shifted by 20 residues away from the band: its best
    alignments run along the diagonal j - i = -20 (m >= n: the band's low side is -B) or + 20 (m < n:
    its high side is B), which a band B <= 5 does not hold."""
    rng = np.random.default_rng(1401)
    pairs = []
    for n in LENGTHS:
        for m in LENGTHS:
            a = rand_seq(rng, n)
            pairs.append((a, mutated_copy(rng, a, m) if len(pairs) % 2 and min(n, m) > 2 else rand_seq(rng, m)))
    for n in LENGTHS[2:]:
        for m in LENGTHS[2:]:
            a = rand_seq(rng, n)
            b = np.concatenate([a[20:], rand_seq(rng, m)])[:m] if m >= n else np.concatenate([rand_seq(rng, 20), a])[:m]
            pairs.append((a, b))
    return pairs


def cpu(sw, pairs, table, go, ge, mode, band=None):
    with sw.Matrix(SYMBOLS, table) as mx:
        return sw.align_matrix_batch(pairs, mx, go, ge, cpu=True, mode=mode, band=band)


# ---- 1, 2. the CPU banded aligner against the restatement ---------------------------------------------

@pytest.mark.parametrize("gaps", GAPS)
def test_cpu_banded_aligner_against_the_restatement(sw, table, band_pairs, gaps):
    for mode in MODES:
        whole = [restate_band(a, b, table, *gaps, mode, None)[0] for a, b in band_pairs]
        narrow = lower = 0
        for B in BANDS:
            got = cpu(sw, band_pairs, table, *gaps, mode, band=B)
            assert len(got) == len(band_pairs)
            for k, ((a, b), x) in enumerate(zip(band_pairs, got)):
                n, m = len(a), len(b)
                score, ei, ej = restate_band(a, b, table, *gaps, mode, B)
                assert x.score == score, (mode, B, k, n, m, x, score)
                if mode != "local" or score > 0:
                    assert (x.end1, x.end2) == (ei + 1, ej + 1), (mode, B, k, n, m, x, ei, ej)
                assert rescore_ops(x, a, b, table, *gaps) == x.score, (mode, B, k)
                assert columns_in_band(x, n, m, B)
                if mode == "global":
                    assert (x.beg1, x.end1, x.beg2, x.end2) == (0, n, 0, m)
                elif mode == "semiglobal":
                    assert (x.beg1, x.end1) == (0, n)
                assert score <= whole[k]
                if B <= 5:
                    narrow += 1
                    lower += score < whole[k]
        print("%s gaps %s: %d of %d pairs with B <= 5 score below their unbanded score" % (mode, gaps, lower, narrow))
        assert 4 * lower >= narrow, (mode, gaps, lower, narrow)     # the band cuts: the test is not vacuous
    assert any(len(a) != len(b) for a, b in band_pairs) and 0 in BANDS


# ---- 3. a band that holds the whole matrix --------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_whole_matrix_band_equals_no_band(sw, table, band_pairs, mode):
    for gaps in GAPS:
        want = cpu(sw, band_pairs, table, *gaps, mode)
        for extra in (0, 1, 1000):
            B = max(max(len(a), len(b)) for a, b in band_pairs) + extra
            assert cpu(sw, band_pairs, table, *gaps, mode, band=B) == want, (mode, gaps, B)
        for (a, b), w in zip(band_pairs[::5], want[::5]):            # B = max(n, m) of the pair itself
            assert cpu(sw, [(a, b)], table, *gaps, mode, band=max(len(a), len(b))) == [w]


# ---- 4. band_plan ------------------------------------------------------------------------------------

def test_band_plan(sw):
    for n, m, B in [(1, 1, 0), (7, 7, 0), (7, 7, 2), (10, 3, 0), (3, 10, 1), (64, 65, 5), (130, 63, 0), (63, 130, 64),
                    (513, 700, 37), (700, 513, 1000)]:
        p = sw.band_plan(n, m, B)
        dlo, dhi = band_range(n, m, B)
        assert (p["dlo"], p["dhi"]) == (dlo, dhi)
        i, j = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
        assert p["cells"] == int(((j - i >= dlo) & (j - i <= dhi)).sum()), (n, m, B)
        assert 0 < p["cells"] <= n * m and p["trace_bytes"] > 0
        assert (p["cells"] == n * m) == (B >= max(n, m) or (dlo <= -(n - 1) and dhi >= m - 1))
    p = sw.band_plan(60000, 60000, 500)
    assert p["trace_bytes"] < p["full_trace_bytes"]
    assert p["cells"] == 60000 * 1001 - 500 * 501
    last = None
    for B in (0, 1, 2, 63, 64, 65, 500, 4000, 60000, 100000):           # monotone in B
        p = sw.band_plan(6000, 5000, B)
        if last is not None:
            assert p["cells"] >= last["cells"] and p["trace_bytes"] >= last["trace_bytes"] and p["dlo"] < last["dlo"]
        last = p
    assert last["cells"] == 6000 * 5000
    assert sw.band_plan(0, 5, 3)["cells"] == 0 and sw.band_plan(5, 0, 3)["trace_bytes"] == 0


# ---- 5. refusals ---------------------------------------------------------------------------------------

def test_refusals(sw, table):
    a, b = np.frombuffer(b"ARND", np.uint8), np.frombuffer(b"ARND", np.uint8)
    with sw.Matrix(SYMBOLS, table) as mx:
        with pytest.raises(sw.SwError, match="sw_align_matrix_cpu_band: band -1"):
            sw.align_matrix_batch([(a, b)], mx, 12, 1, cpu=True, mode="global", band=-1)
        with pytest.raises(sw.SwError, match="sw_band_plan: band -1"):
            sw.band_plan(10, 10, -1)
        with pytest.raises(ValueError, match="long=True"):
            sw.align_matrix_batch([(a, b)], mx, 12, 1, long=True, band=3)
        with pytest.raises(ValueError, match="long=True"):
            sw.align_matrix(a, b, mx, 12, 1, long=True, band=3)
        with pytest.raises(ValueError):
            sw.align_matrix_batch([(a, b)], mx, 12, 1, cpu=True, band="3")
        with pytest.raises(ValueError, match="unknown alignment mode"):
            sw.align_matrix_batch([(a, b)], mx, 12, 1, cpu=True, mode="banded", band=3)
        # empty sequences are answered on the host as without a band
        e = np.zeros(0, np.uint8)
        for mode in MODES:
            assert (sw.align_matrix_batch([(e, b), (a, e), (e, e)], mx, 3, 1, cpu=True, mode=mode, band=2)
                    == sw.align_matrix_batch([(e, b), (a, e), (e, e)], mx, 3, 1, cpu=True, mode=mode))


# ---- 6. the sanitizer driver ---------------------------------------------------------------------------

def test_asan_driver():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "concurrentproject_amd", "csrc"), "asan-align-band"], check=True,
                   timeout=300)
    exe = os.path.join(ROOT, "build", "asan", "align_band_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, "11", "64"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[1]) == 45 * 64 and int(words[3]) >= int(words[1]) // 2

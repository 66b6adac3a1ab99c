"""Long pairs on many waves, host side (include/algoGPU.h sw_align_long_coop_plan, option long_window;
csrc/sw_align_host.cpp), no GPU: what sw_align_matrix_long_coop holds in device
memory, the window of strips a round fills, and what the call refuses.

* align_long_coop_plan against the formulas restated here, over the grid of tests/test_align_long.py:
  strips = ceil(n / 512); checkpoints as align_long_plan; a 4-byte progress word a strip in a whole
  number of 16 bytes; a 16-byte end-cell record a strip; the window of a lone pair, automatic
  (floor(trace_mb / one strip's trace)) and forced (long_window), cut to 64, to the strips and to
  trace_mb; the window's trace bytes;
* the same under trace_mb = 1 and SWMI_ALIGN_CKPT_MB = 1, at n or m = 0 and at 2^27 - 1: no overflow;
* the refusals, which are align_long_plan's, word for word;
* the ValueErrors of coop=True without long=True, with cpu=True, band= or a non-local mode;
* include/algoGPU.h declares the new entry points and the library exports them;
* option long_window: default 0, 0 .. 64, not enumerated by sw_option_name;
* the planner, the window rule and the host merge of end-cell records under AddressSanitizer + UBSan
  in a stand-alone program (tests/asan/align_long_coop_driver.cpp,
  `make -C concurrentproject_amd/csrc asan-align-long-coop`)."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID_N = (1, 511, 512, 513, 1024, 1025, 1100, 1537, 2600)
GRID_M = (1, 63, 64, 65, 300, 700)
MIB = 1 << 20
LONGEST = (1 << 27) - 1


@pytest.fixture(scope="module")
def sw():
    import concurrentproject_amd as sw
    sw.lib()
    return sw


@pytest.fixture()
def budgets(sw):
    """Sets trace_mb, long_window and SWMI_ALIGN_CKPT_MB; all three are restored afterwards."""
    old_env = os.environ.get("SWMI_ALIGN_CKPT_MB")
    old = {k: sw.get_option(k) for k in ("trace_mb", "long_window")}

    def set_budgets(trace_mb=1024, ckpt_mb=None, window=0):
        sw.set_option("trace_mb", trace_mb)
        sw.set_option("long_window", window)
        if ckpt_mb is None:
            os.environ.pop("SWMI_ALIGN_CKPT_MB", None)
        else:
            os.environ["SWMI_ALIGN_CKPT_MB"] = str(ckpt_mb)
    yield set_budgets
    for k, v in old.items():
        sw.set_option(k, v)
    if old_env is None:
        os.environ.pop("SWMI_ALIGN_CKPT_MB", None)
    else:
        os.environ["SWMI_ALIGN_CKPT_MB"] = old_env


def plan(n, m, trace_mb=1024, window=0):
    """The formulas of include/algoGPU.h, restated."""
    if n == 0 or m == 0:
        return {"strips": 0, "ckpt_bytes": 0, "progress_bytes": 0, "end_bytes": 0, "window": 0, "window_trace_bytes": 0}
    strips = -(-n // 512)
    strip = -(-(m + 511) // 64) * 64 * 256
    fits = trace_mb * MIB // strip
    g = max(1, min(64, strips, fits if window == 0 else min(window, fits)))
    return {"strips": strips, "ckpt_bytes": (strips - 1) * (-(-m // 64) * 64) * 8, "progress_bytes": -(-strips * 4 // 16) * 16,
            "end_bytes": strips * 16, "window": g, "window_trace_bytes": g * strip}


def test_plan_over_the_grid(sw, budgets):
    for trace_mb, ckpt_mb in ((1024, None), (1, 1)):
        for window in (0, 1, 2, 5, 64):
            budgets(trace_mb, ckpt_mb, window)
            for n in GRID_N + (0,):
                for m in GRID_M + (0,):
                    got = sw.align_long_coop_plan(n, m)
                    assert got == plan(n, m, trace_mb, window), (n, m, trace_mb, window)
                    old = sw.align_long_plan(n, m)
                    assert (got["strips"], got["ckpt_bytes"]) == (old["strips"], old["ckpt_bytes"])
                    assert got["window_trace_bytes"] <= trace_mb * MIB
    budgets(1024, None, 0)
    big = sw.align_long_coop_plan(32768, 32768)     # the measured pair: 64 strips, 63 traced at once
    assert big == {"strips": 64, "ckpt_bytes": 63 * 32768 * 8, "progress_bytes": 256, "end_bytes": 1024, "window": 64,
                   "window_trace_bytes": 64 * 8519680}
    assert sw.align_long_coop_plan(65536, 65536)["window"] == 1024 * MIB // 16908288 == 63
    budgets(1, None, 0)
    assert sw.align_long_coop_plan(1537, 700)["window"] == 3 and sw.align_long_coop_plan(2600, 300)["window"] == 4
    budgets(1, None, 64)
    assert sw.align_long_coop_plan(1537, 700)["window"] == 3      # forced, cut to what fits trace_mb
    budgets(1, None, 2)
    assert sw.align_long_coop_plan(1537, 700) == {"strips": 4, "ckpt_bytes": 16896, "progress_bytes": 16, "end_bytes": 64,
                                                  "window": 2, "window_trace_bytes": 2 * 311296}


def test_refusals_are_those_of_the_long_plan(sw, budgets):
    for window in (0, 3):
        budgets(1, None, window)
        with pytest.raises(sw.SwError, match=r"pair 0: a 600 x 5000 alignment needs 1425408 bytes of trace memory for one "
                                             r"strip, more than option trace_mb = 1 MiB"):
            sw.align_long_coop_plan(600, 5000)
        assert sw.align_long_coop_plan(131072, 576)["ckpt_bytes"] == 255 * 576 * 8
        budgets(1, 1, window)
        with pytest.raises(sw.SwError, match=r"pair 0: a 131072 x 576 alignment needs 1175040 bytes of checkpoints, more "
                                             r"than SWMI_ALIGN_CKPT_MB = 1 MiB"):
            sw.align_long_coop_plan(131072, 576)
    for n, m in ((600, 5000), (131072, 576)):       # the same text from both planners
        texts = []
        for f in (sw.align_long_plan, sw.align_long_coop_plan):
            with pytest.raises(sw.SwError) as e:
                f(n, m)
            texts.append(str(e.value))
        assert texts[0] == texts[1]
    for bad in ("0", "-1", "x", "1.5", ""):
        budgets(1024, bad)
        with pytest.raises(sw.SwError, match="SWMI_ALIGN_CKPT_MB"):
            sw.align_long_coop_plan(100, 100)


def test_empty_and_longest(sw, budgets):
    budgets(3072, 1 << 30)
    zero = plan(0, 0)
    assert sw.align_long_coop_plan(0, 700) == sw.align_long_coop_plan(700, 0) == sw.align_long_coop_plan(0, 0) == zero
    assert sw.align_long_coop_plan(LONGEST, 0) == zero
    got = sw.align_long_coop_plan(LONGEST, 64)
    assert got == plan(LONGEST, 64, 3072) and got["strips"] == 1 << 18 and got["progress_bytes"] == 1 << 20
    assert got["end_bytes"] == 1 << 22 and got["window"] == 64
    got = sw.align_long_coop_plan(LONGEST, 65536)
    assert got == plan(LONGEST, 65536, 3072) and got["window_trace_bytes"] == 64 * 16908288
    with pytest.raises(sw.SwError, match=r"a 64 x 134217727 alignment needs 34359869440 bytes of trace memory"):
        sw.align_long_coop_plan(64, LONGEST)
    budgets(3072, None)
    with pytest.raises(sw.SwError, match=r"needs %d bytes of checkpoints" % (((1 << 18) - 1) << 30)):
        sw.align_long_coop_plan(LONGEST, LONGEST)
    for bad in ((-1, 5), (5, -1), (LONGEST + 1, 5), (5, LONGEST + 1)):
        with pytest.raises(sw.SwError, match="sw_align_long_coop_plan: invalid arguments"):
            sw.align_long_coop_plan(*bad)


def test_value_errors(sw):
    a = np.frombuffer(b"ACDEFGHIKL" * 3, np.uint8)
    with sw.Matrix(b"ACDEFGHIKLMNPQRSTVWY", np.where(np.eye(20, dtype=bool), 2, -3)) as mx:
        with pytest.raises(ValueError, match="coop=True is not built without long=True"):
            sw.align_matrix_batch([(a, a)], mx, 5, 2, coop=True)
        with pytest.raises(ValueError, match="coop=True is not built without long=True"):
            sw.align_matrix(a, a, mx, 5, 2, coop=True, cpu=True)
        with pytest.raises(ValueError, match="not with cpu=True"):
            sw.align_matrix_batch([(a, a)], mx, 5, 2, long=True, coop=True, cpu=True)
        with pytest.raises(ValueError, match=r"band= is not built for coop=True \(the cooperative long path\)"):
            sw.align_matrix_batch([(a, a)], mx, 5, 2, long=True, coop=True, band=4)
        for mode in ("global", "semiglobal"):
            with pytest.raises(ValueError, match="mode=%r is not built for long=True" % mode):
                sw.align_matrix(a, a, mx, 5, 2, long=True, coop=True, mode=mode)
        with sw.Database.from_records([("r", a)]) as db:
            with pytest.raises(ValueError, match="coop=True is not built without long=True"):
                db.align(a, [0], mx, 5, 2, coop=True)
            with pytest.raises(ValueError, match="mode='global' is not built for long=True"):
                db.align(a, [0], mx, 5, 2, long=True, coop=True, mode="global")
    from concurrentproject_amd.align import main
    with pytest.raises(SystemExit):                           # --coop is a way of running --long
        main(["--query", "q.fa", "--db", "d.fa", "--alignments", "--coop"])


def test_header_declares_the_entry_points(sw):
    with open(os.path.join(ROOT, "include", "algoGPU.h")) as f:
        text = f.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("sw_align_matrix_long_coop", "sw_db_align_matrix_long_coop", "sw_align_long_coop_plan"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(sw.lib(), name), name
    m = re.search(r"typedef struct \{([^{}]*)\} sw_align_coop_plan;", code)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == ("int strips; long long ckpt_bytes; long long progress_bytes; "
                                                            "long long end_bytes; int window; long long window_trace_bytes;")
    assert "long_window" in text and "mode 12" in text


def test_option_long_window(sw):
    old = sw.get_option("long_window")
    try:
        assert old == 0
        for v in (1, 64, 17, 0):
            sw.set_option("long_window", v)
            assert sw.get_option("long_window") == v
        for bad in (-1, 65):
            with pytest.raises(sw.SwError):
                sw.set_option("long_window", bad)
            assert sw.get_option("long_window") == 0
    finally:
        sw.set_option("long_window", old)
    L = sw.lib()
    if hasattr(L, "sw_option_name"):                          # the listed keys are the header's "Tuning knobs"
        import ctypes
        L.sw_option_name.restype = ctypes.c_char_p
        L.sw_option_name.argtypes = [ctypes.c_int]
        names, k = [], 0
        while L.sw_option_name(k):
            names.append(L.sw_option_name(k).decode())
            k += 1
        assert "trace_mb" in names and "long_window" not in names and "coop_mb" not in names


def test_planner_window_and_merge_under_sanitizers():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "concurrentproject_amd", "csrc"), "asan-align-long-coop"], check=True)
    exe = os.path.join(ROOT, "build", "asan", "align_long_coop_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[1]) > 500 and int(words[2]) > 20000 and int(words[3]) > 10000

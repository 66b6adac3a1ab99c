"""Long pairs in a mode, host side (include/algoGPU.h sw_align_matrix_long_mode and its three namesakes;
csrc/sw_align_host.cpp), no GPU:

* include/algoGPU.h declares the four entry points and the library exports them; the Python calls exist;
* an unknown mode: ValueError from the Python calls, -1 with a message from the library;
* the range refusal, naming its pair or its record, from all four entry points before any device work
  (this machine has no device: a call that got as far as one would fail with another message);
* the plans take no mode;
* the keyword routes long=True with a mode, and `align --long --mode`, still raise, and name the new call;
* the end-record selection, the empty-sequence answers and the refusals under AddressSanitizer + UBSan in a
  stand-alone program (tests/asan/align_long_mode_driver.cpp,
  `make -C concurrentproject_amd/csrc asan-align-long-mode`)."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from test_matrix_cpu import random_table
from test_matrix import SYMBOLS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sw_align_matrix_long_mode", "sw_align_matrix_long_coop_mode", "sw_db_align_matrix_long_mode",
         "sw_db_align_matrix_long_coop_mode")
MODES = ("global", "semiglobal")


@pytest.fixture(scope="module")
def sw():
    import concurrentproject_amd as sw
    sw.lib()
    return sw


@pytest.fixture(scope="module")
def mx(sw):
    with sw.Matrix(SYMBOLS, random_table(np.random.default_rng(24), 24)) as m:
        yield m


def test_header_declares_the_entry_points(sw):
    with open(os.path.join(ROOT, "include", "algoGPU.h")) as f:
        text = f.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, code)
        assert m, name
        assert re.search(r"int gap_init, int gap_ext, int mode,\s*sw_alignment\* out", m.group(1)), name
        assert hasattr(sw.lib(), name), name
        assert getattr(sw.lib(), name).argtypes is not None
    assert "DESIGN.md section 18" in text and "do\n *   not depend on the mode" in text
    assert list(inspect.signature(sw.align_matrix_long).parameters)[-2:] == ["coop", "mode"]
    assert inspect.signature(sw.align_matrix_long).parameters["mode"].default == "local"
    par = inspect.signature(sw.Database.align_long).parameters
    assert list(par)[1:] == ["query", "indices", "matrix", "gap_init", "gap_ext", "mode", "coop"]
    assert (par["mode"].default, par["coop"].default) == ("local", False)


def test_unknown_mode(sw, mx):
    a = np.frombuffer(b"ARND", np.uint8)
    for coop in (False, True):
        with pytest.raises(ValueError, match="unknown alignment mode 'glocal'"):
            sw.align_matrix_long([(a, a)], mx, 12, 1, coop=coop, mode="glocal")
        with sw.Database.from_records([("r0", a)]) as db:
            with pytest.raises(ValueError, match="unknown alignment mode 'glocal'"):
                db.align_long(a, [0], mx, 12, 1, mode="glocal", coop=coop)
    L = sw.lib()
    for name in NAMES[:2]:
        with pytest.raises(sw.SwError, match="%s: unknown alignment mode 3" % name):
            sw._align_pairs(getattr(L, name), [(a, a)], mx, 12, 1, mode=3)
    with pytest.raises(ValueError, match="needs a substitution matrix"):
        sw.align_matrix_long([(a, a)], None, 12, 1, mode="global")


def test_range_refusal_before_any_device_work(sw, mx):
    a = np.frombuffer(b"ARND", np.uint8)
    long = np.full(1 << 22, SYMBOLS[0], np.uint8)
    for mode in MODES:
        for coop in (False, True):
            with pytest.raises(sw.SwError, match="pair 1: score range exceeds the int32 engine in this mode"):
                sw.align_matrix_long([(a, a), (long, a)], mx, 12, 1, coop=coop, mode=mode)
            with pytest.raises(sw.SwError, match="pair 0: score range exceeds the int32 engine in this mode"):
                sw.align_matrix_long([(a, a)], mx, 1 << 20, 1, coop=coop, mode=mode)
            with sw.Database.from_records([("r0", a), ("r1", long), ("r2", a)]) as db:
                with pytest.raises(sw.SwError, match="record 1: score range exceeds the int32 engine in this mode"):
                    db.align_long(a, [2, 0, 1], mx, 12, 1, mode=mode, coop=coop)
                with pytest.raises(sw.SwError, match="record 2: score range"):
                    db.align_long(a, [2], mx, 1, 1 << 20, mode=mode, coop=coop)
                with pytest.raises(sw.SwError, match="sw_db_align_matrix_long%s_mode: record index 3" % ("_coop" if coop else "")):
                    db.align_long(a, [0, 3], mx, 12, 1, mode=mode, coop=coop)
                assert db.align_long(a, [], mx, 12, 1, mode=mode, coop=coop) == []
            assert sw.align_matrix_long([], mx, 12, 1, coop=coop, mode=mode) == []


def test_the_plans_take_no_mode(sw):
    assert list(inspect.signature(sw.align_long_plan).parameters) == ["n", "m"]
    assert list(inspect.signature(sw.align_long_coop_plan).parameters) == ["n", "m"]
    assert sw.align_long_plan(65536, 65536)["ckpt_bytes"] == 127 * 65536 * 8


def test_the_keyword_routes_still_raise(sw, mx, capsys):
    a = np.frombuffer(b"ARND", np.uint8)
    for mode in MODES:
        for coop in (False, True):
            with pytest.raises(ValueError, match=r"mode=%r is not built for long=True .* local only; align_matrix_long\(" % mode):
                sw.align_matrix(a, a, mx, 12, 1, long=True, coop=coop, mode=mode)
            with pytest.raises(ValueError, match="mode=%r is not built for long=True" % mode):
                sw.align_matrix_batch([(a, a)], mx, 12, 1, long=True, coop=coop, mode=mode)
            with sw.Database.from_records([("r0", a)]) as db:
                with pytest.raises(ValueError, match=r"mode=%r is not built for long=True .* local only; Database.align_long\(" % mode):
                    db.align(a, [0], mx, 12, 1, long=True, coop=coop, mode=mode)
        with sw.Database.from_records([("r0", a)]) as db, sw.Database.from_records([("q0", a)]) as qs:
            with pytest.raises(ValueError, match="mode=%r is not built for search_db: it is local only$" % mode):
                db.search_db(qs, matrix=mx, gap_init=12, gap_ext=1, mode=mode)
    from concurrentproject_amd.align import main
    with pytest.raises(SystemExit) as e:
        main(["--query", "q.fa", "--db", "d.fa", "--matrix", "M.txt", "--gaps", "12,1", "--alignments", "--long", "--mode", "global"])
    err = capsys.readouterr().err
    assert e.value.code == 2 and "--long is local only" in err and "Database.align_long" in err


def test_end_record_empties_and_refusals_under_sanitizers():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "concurrentproject_amd", "csrc"), "asan-align-long-mode"], check=True,
                   timeout=300)
    exe = os.path.join(ROOT, "build", "asan", "align_long_mode_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[1]) > 4000 and int(words[2]) > 60000 and int(words[3]) == 100 and int(words[4]) > 20000

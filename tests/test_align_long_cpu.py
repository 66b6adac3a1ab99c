"""Long pairs by checkpointed traceback, host side (include/algoGPU.h sw_align_long_plan;
csrc/sw_align_host.cpp), no GPU: the arithmetic that decides what sw_align_matrix_long holds in
device memory and what it refuses.

* align_long_plan against the formulas restated here, over the grid of tests/test_align_long.py:
  strips = ceil(n / 512); checkpoints (strips - 1) columns of roundup(m, 64) rows, 8 B a row; one
  strip's trace ceil((m + 511) / 64) * 64 steps of 256 B; the whole pair's trace strips times that;
* the pinned values of the pairs that sw_align_matrix_batch refuses at trace_mb = 1;
* the two refusals, under trace_mb = 1 and SWMI_ALIGN_CKPT_MB = 1; n or m = 0; the longest
  sequence (2^27 - 1): no overflow;
* include/algoGPU.h declares the new entry points and the library exports them;
* the planner, the budget's environment variable and the greedy packer of groups and rounds under
  AddressSanitizer + UBSan in a stand-alone program (tests/asan/align_long_driver.cpp,
  `make -C concurrentproject_amd/csrc asan-align-long`)."""
import os
import re
import subprocess

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
    """Sets trace_mb and SWMI_ALIGN_CKPT_MB; both are restored afterwards."""
    old_env = os.environ.get("SWMI_ALIGN_CKPT_MB")
    old_opt = sw.get_option("trace_mb")

    def set_budgets(trace_mb=None, ckpt_mb=None):
        if trace_mb is not None:
            sw.set_option("trace_mb", trace_mb)
        if ckpt_mb is None:
            os.environ.pop("SWMI_ALIGN_CKPT_MB", None)
        else:
            os.environ["SWMI_ALIGN_CKPT_MB"] = str(ckpt_mb)
    yield set_budgets
    sw.set_option("trace_mb", old_opt)
    if old_env is None:
        os.environ.pop("SWMI_ALIGN_CKPT_MB", None)
    else:
        os.environ["SWMI_ALIGN_CKPT_MB"] = old_env


def plan(n, m):
    """The formulas of include/algoGPU.h, restated."""
    if n == 0 or m == 0:
        return {"strips": 0, "ckpt_bytes": 0, "strip_trace_bytes": 0, "full_trace_bytes": 0}
    strips = -(-n // 512)
    strip = -(-(m + 511) // 64) * 64 * 256
    return {"strips": strips, "ckpt_bytes": (strips - 1) * (-(-m // 64) * 64) * 8, "strip_trace_bytes": strip,
            "full_trace_bytes": strips * strip}


def test_plan_over_the_grid(sw, budgets):
    budgets(1024, None)
    for n in GRID_N + (0, 65536):
        for m in GRID_M + (0, 576, 5000, 65536):
            assert sw.align_long_plan(n, m) == plan(n, m), (n, m)
    big = sw.align_long_plan(65536, 65536)      # the headline pair: 2.1 GB of trace, or 67 MB + 17 MB
    assert big["full_trace_bytes"] == 2164260864 and big["ckpt_bytes"] == 127 * 65536 * 8 == 66584576
    assert big["strip_trace_bytes"] == 16908288


def test_pinned_values(sw, budgets):
    budgets(1, None)
    assert sw.align_long_plan(2600, 300) == {"strips": 6, "ckpt_bytes": 12800, "strip_trace_bytes": 212992,
                                             "full_trace_bytes": 1277952}
    assert sw.align_long_plan(1537, 700) == {"strips": 4, "ckpt_bytes": 16896, "strip_trace_bytes": 311296,
                                             "full_trace_bytes": 1245184}
    assert sw.align_long_plan(2600, 700)["ckpt_bytes"] == 28160
    for n, m in ((2600, 300), (1537, 700)):     # more than trace_mb = 1 as a whole, less a strip at a time
        p = sw.align_long_plan(n, m)
        assert p["full_trace_bytes"] > MIB > p["strip_trace_bytes"] + p["ckpt_bytes"]


def test_refusals(sw, budgets):
    budgets(1, None)
    with pytest.raises(sw.SwError, match=r"pair 0: a 600 x 5000 alignment needs 1425408 bytes of trace memory for one "
                                         r"strip, more than option trace_mb = 1 MiB"):
        sw.align_long_plan(600, 5000)
    assert sw.align_long_plan(131072, 576)["ckpt_bytes"] == 255 * 576 * 8      # fits the default 4096 MiB
    budgets(1, 1)
    with pytest.raises(sw.SwError, match=r"pair 0: a 131072 x 576 alignment needs 1175040 bytes of checkpoints, more "
                                         r"than SWMI_ALIGN_CKPT_MB = 1 MiB"):
        sw.align_long_plan(131072, 576)
    assert sw.align_long_plan(2600, 700)["ckpt_bytes"] == 28160                # read on every call
    budgets(1024, 2)
    assert sw.align_long_plan(131072, 576)["strips"] == 256
    for bad in ("0", "-1", "x", "1.5", ""):
        budgets(1024, bad)
        with pytest.raises(sw.SwError, match="SWMI_ALIGN_CKPT_MB"):
            sw.align_long_plan(100, 100)


def test_empty_and_longest(sw, budgets):
    budgets(3072, 1 << 30)
    zero = {"strips": 0, "ckpt_bytes": 0, "strip_trace_bytes": 0, "full_trace_bytes": 0}
    assert sw.align_long_plan(0, 700) == sw.align_long_plan(700, 0) == sw.align_long_plan(0, 0) == zero
    assert sw.align_long_plan(LONGEST, 0) == zero
    got = sw.align_long_plan(LONGEST, 64)
    assert got == plan(LONGEST, 64) and got["strips"] == 1 << 18 and got["ckpt_bytes"] == ((1 << 18) - 1) * 512
    got = sw.align_long_plan(LONGEST, 65536)
    assert got == plan(LONGEST, 65536) and got["full_trace_bytes"] == (1 << 18) * 16908288 > 1 << 42
    with pytest.raises(sw.SwError, match=r"a 64 x 134217727 alignment needs 34359869440 bytes of trace memory"):
        sw.align_long_plan(64, LONGEST)
    budgets(3072, None)
    with pytest.raises(sw.SwError, match=r"needs %d bytes of checkpoints" % (((1 << 18) - 1) << 30)):
        sw.align_long_plan(LONGEST, LONGEST)
    for bad in ((-1, 5), (5, -1), (LONGEST + 1, 5), (5, LONGEST + 1)):
        with pytest.raises(sw.SwError, match="invalid arguments"):
            sw.align_long_plan(*bad)


def test_header_declares_the_entry_points(sw):
    with open(os.path.join(ROOT, "include", "algoGPU.h")) as f:
        text = f.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("sw_align_matrix_long", "sw_db_align_matrix_long", "sw_align_long_plan"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(sw.lib(), name), name
    assert re.search(r"typedef struct \{ int strips; long long ckpt_bytes, strip_trace_bytes, full_trace_bytes; \} "
                     r"sw_align_plan;", code)
    assert "SWMI_ALIGN_CKPT_MB" in text and "mode 8" in text


def test_planner_under_sanitizers():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "concurrentproject_amd", "csrc"), "asan-align-long"], check=True)
    exe = os.path.join(ROOT, "build", "asan", "align_long_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[1]) > 100 and int(words[2]) > 400

"""The wedge planner's arithmetic and the join units of a launch that joins its chains in the staged kernel
(sw_internal.h join_unit_*), checked on the host: tools/wedge_bounds_check.cpp built stand-alone with
AddressSanitizer and UndefinedBehaviorSanitizer and run.  It sweeps the planned shapes and asserts that the units
visit exactly the index set of the combine kernels, that every entry a unit loads belongs to a strip that counts
into it, and that its full count is the number of those strips."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_wedge_bounds_and_join_units_under_host_sanitizers(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.fail("hipcc not found: the check includes sw_internal.h, which needs the HIP headers")
    exe = str(tmp_path / "wedge_bounds_check")
    cc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    subprocess.run([cc, "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", "--offload-arch=gfx950",
                    "-I", os.path.join(ROOT, "concurrentproject_amd", "csrc"),
                    os.path.join(ROOT, "tools", "wedge_bounds_check.cpp"), "-o", exe], check=True, cwd=str(tmp_path))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "wedge_bounds_check: 0 failures" in r.stdout, r.stdout[-2000:]

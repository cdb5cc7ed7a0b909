"""The window test of rcp_exact (cl2::rcp_window, clive2_amd/csrc/vecmath.hpp) decides as the exponent-field form it replaced, for
every one of the 2^32 bit patterns: tools/rcp_window_check.hip, built with hipcc and run on the host -- no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_test_of_rcp_exact_is_the_same_predicate_for_all_patterns(tmp_path):
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the library itself cannot be built without it")
    exe = str(tmp_path / "rcp_window_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O3", "-std=c++17", "-pthread", os.path.join(ROOT, "tools", "rcp_window_check.hip"),
                    "-o", exe], check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert res.stdout.startswith("0 of 4294967296 patterns differ")

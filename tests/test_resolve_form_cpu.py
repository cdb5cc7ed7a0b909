"""CPU test of the host-side rule that picks the resolve kernel of a pass (clive2_amd/csrc/scene_layout.hpp: resolve_runs_slim),
through tests/resolve_form_driver.cpp built with g++ -- no GPU.  The slim kernel keeps a light vertex's triangle index and material
byte in one word, {triangle << 8 | material}; a scene whose triangle indices do not fit runs k_connect_resolve.  A scene that
large is no seconds-long GPU test, so the triangle count is injected here, on either side of the limit."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("resolve_form") / "resolve_form_driver.so")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include",
                    os.path.join(ROOT, "tests", "resolve_form_driver.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.rf_runs_slim.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    return L


def test_triangle_count_limit_of_the_packed_word(lib):
    bits = lib.rf_tri_bits()
    limit = 1 << bits
    assert bits == 23                                     # 32 bits - the material byte - the sign
    # every index of a scene at the limit, and the -1 of "no triangle", survive the packed word with any material byte
    for tri in (-1, 0, 1, 36, limit - 2, limit - 1):
        for meta in (0, 7, 0xFF, 0x1FF, 0x3FF):          # the flag bits 8 and 9 of a vertex's meta word are not kept
            w = lib.rf_pack(tri, meta)
            assert lib.rf_packed_tri(w) == tri and lib.rf_packed_mat(w) == meta & 0xFF
    assert lib.rf_packed_tri(lib.rf_pack(limit, 0)) != limit          # the first index that does not
    for n, slim in ((36, 1), (328, 1), (limit - 1, 1), (limit, 1), (limit + 1, 0), (1 << 27, 0)):
        assert lib.rf_runs_slim(n, 8, 0, 0, 0, 0) == slim, n


def test_every_other_combination_runs_the_parent_kernel(lib):
    cap, bit = lib.rf_mat_cap(), 1 << lib.rf_parent_bit()
    assert bit == 1 << 27
    assert lib.rf_runs_slim(36, cap, 0, 0, 0, 0) == 1
    assert lib.rf_runs_slim(36, cap + 1, 0, 0, 0, 0) == 0             # material table in global memory
    assert lib.rf_runs_slim(36, 8, 1, 0, 0, 0) == 0                   # slot map (adaptive sampling)
    assert lib.rf_runs_slim(36, 8, 0, 1, 0, 0) == 0                   # partial strategy mask
    assert lib.rf_runs_slim(36, 8, 0, 0, 1, 0) == 0                   # layer table
    assert lib.rf_runs_slim(36, 8, 0, 0, 0, bit) == 0                 # the debug bit
    assert lib.rf_runs_slim(36, 8, 0, 0, 0, ~bit & 0x0EFF7FFF) == 1   # no other bit

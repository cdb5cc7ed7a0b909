"""The trees of the GPU BVH builder (cl2_build_bvh_gpu, csrc/bvh_builder_gpu.hip) box for box against their numpy statement
(tests/gpu_bvh_reference.py) on the inputs of tests/gpu_bvh_cases.py.  Render parity cannot see a bad tree (the oracle walks the same
Box[]), so every case here requires

    rc == 0, the independent checker passes (tight bounds, numbering, leaf ranges, smaller subtree at left + 1),
    boxes[:nb] (min, max as float values; left, right) and perm EQUAL the restatement's -- the tree, not just a valid tree,
    and a second call returns the same bytes.

The families: sizes across the PLOC radius, the wave, the workgroup and several blocks of the sort and the scan, at leaf sizes 1, 2, 3,
8 and >= n; the same through the radix tree (CLIVE2_GPU_BVH=lbvh, read on every call); exact area ties (lattices of equal boxes: the
pair rule picks among several candidates at the smallest area; on the 13 x 11 x 7 one any other rule gives another tree); equal
Morton keys (the stable sort, delta on equal keys, the cap of rounds); centroids without extent on one or two axes and boxes without
volume; PLOC given up in mid-build (its arrays must not leak into the radix tree); box_capacity."""
import ctypes as C

import numpy as np
import pytest

import gpu_bvh_cases as cases
import gpu_bvh_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from clive2_amd import _native
    L = _native.lib()
    L.cl2_build_bvh_gpu.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64,
                                    C.POINTER(C.c_int64), C.c_void_p]
    return L


def _build(L, lo, hi, members, cap=None):
    from clive2_amd import _native, struct_types as st
    n = len(lo)
    boxes = np.zeros(2 * n if cap is None else cap, st.Box)
    perm = np.full(n, -1, np.int64)
    nb = C.c_int64(-1)
    rc = L.cl2_build_bvh_gpu(0, _native.ptr(lo), _native.ptr(hi), n, members, _native.ptr(boxes), len(boxes), C.byref(nb), _native.ptr(perm))
    return rc, boxes, nb.value, perm


def _same_tree(got, perm, want, want_perm, what):
    assert len(got) == len(want), f"{what}: {len(got)} boxes, the restatement has {len(want)}"
    for f in ("left", "right"):
        bad = np.flatnonzero(got[f] != want[f])
        assert not len(bad), f"{what}: `{f}` differs first at box {bad[0]}: {got[f][bad[0]]}, the restatement has {want[f][bad[0]]}"
    bad = np.flatnonzero(perm != want_perm)
    assert not len(bad), f"{what}: perm differs first at {bad[0]}"
    for f in ("min", "max"):                               # float values: fminf(-0, +0) may return either zero
        bad = np.flatnonzero((got[f] != want[f]).any(axis=1))
        assert not len(bad), f"{what}: `{f}` differs first at box {bad[0]}: {got[f][bad[0]]}, the restatement has {want[f][bad[0]]}"
    assert not got["pad"].any()


def _check_case(L, case):
    case.guard(case.prepared())
    lo, hi = case.boxes()
    for mm in case.members:
        what = f"{case.name}, max_members {mm}"
        rc, boxes, nb, perm = _build(L, lo, hi, mm)
        assert rc == 0, (what, L.cl2_last_error(None))
        got = boxes[:nb]
        ref.check_tree(lo, hi, got, perm, mm)
        _same_tree(got, perm, *case.tree(mm), what)
        assert not boxes[nb:].view(np.uint8).any(), f"{what}: boxes behind the tree were written"
        rc2, boxes2, nb2, perm2 = _build(L, lo, hi, mm)
        assert rc2 == 0 and nb2 == nb and boxes2.tobytes() == boxes.tobytes() and perm2.tobytes() == perm.tobytes(), f"{what}: a second call differs"


def _named(family):
    return [c for c in cases.CASES if c.family == family]


@pytest.mark.parametrize("case", _named("sizes"), ids=repr)
def test_sizes(lib, monkeypatch, case):
    monkeypatch.delenv("CLIVE2_GPU_BVH", raising=False)
    _check_case(lib, case)


@pytest.mark.parametrize("case", _named("lbvh"), ids=repr)
def test_sizes_through_the_radix_tree(lib, monkeypatch, case):
    assert case.method == "lbvh" and 1 in case.members
    monkeypatch.setenv("CLIVE2_GPU_BVH", "lbvh")
    _check_case(lib, case)


@pytest.mark.parametrize("case", _named("ties") + _named("equal-keys") + _named("degenerate") + _named("fallback"), ids=repr)
def test_ties_equal_keys_degenerate_extents_and_fallbacks(lib, monkeypatch, case):
    if case.method == "lbvh":
        monkeypatch.setenv("CLIVE2_GPU_BVH", "lbvh")
    else:
        monkeypatch.delenv("CLIVE2_GPU_BVH", raising=False)
    _check_case(lib, case)


def test_the_method_is_read_on_every_call(lib, monkeypatch):
    """the two methods give different trees on the same input, and switching back gives the first one again"""
    a, b = cases.by_name("ploc-257"), cases.by_name("lbvh-257")
    assert a.tree(3)[0].tobytes() != b.tree(3)[0].tobytes()
    for case in (a, b, a):
        if case.method == "lbvh":
            monkeypatch.setenv("CLIVE2_GPU_BVH", "lbvh")
        else:
            monkeypatch.setenv("CLIVE2_GPU_BVH", "ploc")
        rc, boxes, nb, perm = _build(lib, *case.boxes(), 3)
        assert rc == 0
        _same_tree(boxes[:nb], perm, *case.tree(3), case.name)


@pytest.mark.parametrize("name, members", [("ploc-257", 1), ("ploc-257", 8), ("lbvh-257", 2), ("huge-partial", 3), ("ploc-9", 16)])
def test_box_capacity(lib, monkeypatch, name, members):
    """a capacity of exactly the box count succeeds and gives the tree; one less fails with the capacity error"""
    case = cases.by_name(name)
    if case.method == "lbvh":
        monkeypatch.setenv("CLIVE2_GPU_BVH", "lbvh")
    else:
        monkeypatch.delenv("CLIVE2_GPU_BVH", raising=False)
    want, want_perm = case.tree(members)
    rc, boxes, nb, perm = _build(lib, *case.boxes(), members, cap=len(want))
    assert rc == 0 and nb == len(want), lib.cl2_last_error(None)
    _same_tree(boxes, perm, want, want_perm, name)
    if len(want) > 1:
        rc, boxes, nb, perm = _build(lib, *case.boxes(), members, cap=len(want) - 1)
        assert rc < 0 and b"capacity" in lib.cl2_last_error(None)

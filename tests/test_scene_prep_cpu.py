"""CPU tests of the scene preparation behind cl2_upload_scene (clive2_amd/csrc/scene_prep.hpp): validation of the caller's
arrays and the device records built from them, through tests/scene_prep_driver.cpp built with g++ -- no GPU, and nothing of the
hipcc-built library.

The pinned digests (PINS) were recorded from the preparation moved out of cl2_upload_scene verbatim, before it was split into
stages; the staged module reproduces them, so every array the renderer uploads is byte-identical to what the one long function
built."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

from test_order_independence import visit_rank
from tree_reference import pending_depths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("nodes", "fast", "wide", "tris", "tris36", "shade", "ltris", "mats", "tri_rank", "cam_tris")
SCALARS = ("n_records", "n_top", "n_fast", "fast_flat", "n_wide", "max_pending", "order_depth")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("scene_prep") / "scene_prep_driver.so")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__",
                    f"-I{rocm}/include", os.path.join(ROOT, "tests", "scene_prep_driver.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.sp_prepare.restype = C.c_void_p
    L.sp_prepare.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]
    L.sp_array.restype = C.c_longlong
    L.sp_array.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p)]
    L.sp_scalar.argtypes = [C.c_void_p, C.c_char_p]
    L.sp_free.argtypes = [C.c_void_p]
    return L


class Input:
    """cl2_upload_scene's arguments, taken from a Scene; every field may be replaced before `prepare`."""
    def __init__(self, scene):
        self.boxes = np.array(scene.boxes, copy=True)
        self.tris = np.array(scene.triangles, copy=True)
        self.mats = np.array(scene.materials, copy=True)
        self.cam = np.array(scene.camera, copy=True).reshape(-1)
        self.ltris = np.array(scene.light_triangles, copy=True)
        self.areas = np.ascontiguousarray(scene.light_surface_areas, dtype=np.float32).reshape(-1)
        self.lidx = np.ascontiguousarray(scene.light_triangle_indices, dtype=np.int32).reshape(-1)
        self.W, self.H = int(self.cam["pixel_width"][0]), int(self.cam["pixel_height"][0])
        self.counts = None                         # (n_boxes, n_tris, n_mats, light_count) in place of the array lengths

    def prepare(self, L):
        """(None, {name: bytes or int}) or (refusal message, None)."""
        n = self.counts or tuple(0 if a is None else len(a) for a in (self.boxes, self.tris, self.mats, self.lidx))
        p = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data
        msg = C.create_string_buffer(512)
        h = L.sp_prepare(p(self.boxes), n[0], p(self.tris), n[1], p(self.mats), n[2], p(self.cam), p(self.ltris), p(self.areas),
                         p(self.lidx), n[3], self.W, self.H, msg, 512)
        if not h:
            return msg.value.decode(), None
        out = {}
        for name in ARRAYS:
            d = C.c_void_p()
            size = L.sp_array(h, name.encode(), C.byref(d))
            out[name] = C.string_at(d, size) if size > 0 else b""
        for name in SCALARS:
            out[name] = L.sp_scalar(h, name.encode())
        L.sp_free(h)
        return None, out


def set_bounds(inp, b, tris):
    """Box b of inp.boxes bounds triangles `tris` exactly (float32 min / max of their vertices)."""
    v = np.concatenate([inp.tris[k][tris, :3] for k in ("v0", "v1", "v2")])
    inp.boxes["min"][b, :3], inp.boxes["max"][b, :3] = v.min(axis=0), v.max(axis=0)


def chain(scene, depth):
    """`depth` inner boxes in a row, each the parent of a one-triangle leaf (left) and of the next inner box (left + 1, walked
    first), so the reference's stack holds one more pending box per level; the last inner box has two leaves."""
    inp = Input(scene)
    inp.boxes = np.zeros(2 * depth + 1, inp.boxes.dtype)
    for j in range(depth):
        inp.boxes["left"][2 * j] = 2 * j + 1
        set_bounds(inp, 2 * j, np.arange(j, depth + 1))
    for j in range(depth + 1):
        b = 2 * j + 1 if j < depth else 2 * depth
        inp.boxes["left"][b], inp.boxes["right"][b] = j, j + 1
        set_bounds(inp, b, [j])
    return inp


def big_leaf(scene):
    """A root over two leaves, the first of 20 triangles: an oversized leaf takes two records, so there is no 4-wide collapse."""
    inp = Input(scene)
    n = len(inp.tris)
    inp.boxes = np.zeros(3, inp.boxes.dtype)
    inp.boxes["left"] = [1, 0, 20]
    inp.boxes["right"] = [0, 20, n]
    set_bounds(inp, 0, np.arange(n)); set_bounds(inp, 1, np.arange(20)); set_bounds(inp, 2, np.arange(20, n))
    return inp


def not_nested(scene):
    """The scene's own tree with one leaf box reaching past its parent's."""
    inp = Input(scene)
    leaf = int(np.flatnonzero(inp.boxes["right"] != 0)[0])
    inp.boxes["max"][leaf, 0] += 1.0
    return inp


@pytest.fixture(scope="module")
def scenes(cornell_small, glass_scene):
    import clive2_amd as c2
    from clive2_amd.load import get_materials
    from clive2_amd.meshes import icosphere
    v, f = icosphere(3, radius=2.0, center=(0.0, 1.0, 0.0))
    mesh = c2.create_scene(64, 48, np.array([0, 1.5, 6]), np.array([0, 0, -1]), file_specs=[dict(mesh=(v, f), material=5)],
                           materials=get_materials(), bvh_builder="numpy", max_members=4)
    return {"cornell": cornell_small, "glass": glass_scene, "mesh": mesh}


@pytest.fixture(scope="module")
def inputs(scenes):
    return {"cornell": Input(scenes["cornell"]), "glass": Input(scenes["glass"]), "mesh": Input(scenes["mesh"]),
            "big_leaf": big_leaf(scenes["glass"]), "not_nested": not_nested(scenes["cornell"]), "chain": chain(scenes["glass"], 24)}


def digest(out):
    return {k: (hashlib.sha256(out[k]).hexdigest()[:16] if k in ARRAYS else out[k]) for k in ARRAYS + SCALARS}


# SHA-256 (first 16 hex digits) of each prepared array; the scalars as they are
PINS = {
    "cornell": {"nodes": "8038b7e1dc5a948a", "fast": "49a4cd6313e82a3e", "wide": "6124676fe21c674f", "tris": "b7f6e586fcb38296", "tris36": "e3b19db4e2683619",
        "shade": "3aff54db0c24b2ea", "ltris": "296bcada34d57497", "mats": "d2dbb3e27daba0c3", "tri_rank": "af53d6eaacd050da", "cam_tris": "bfce42ee6f1de630",
        "n_records": 5, "n_top": 0, "n_fast": 3, "fast_flat": 1, "n_wide": 1, "max_pending": 1, "order_depth": 2},
    "glass": {"nodes": "0aefc6b8adbbf810", "fast": "1c40ea03b23c8c1e", "wide": "eaab2425f6bd3b3a", "tris": "a59a769290f0ff25", "tris36": "4c781396304f2bb2",
        "shade": "e4aa70c826a02875", "ltris": "f273723a1f0621a5", "mats": "0c17a38b488ba004", "tri_rank": "83573ba26302b4a3", "cam_tris": "c7bd5e674ae7b286",
        "n_records": 121, "n_top": 0, "n_fast": 119, "fast_flat": 0, "n_wide": 34, "max_pending": 6, "order_depth": 13},
    "mesh": {"nodes": "75c8df3c6a76d303", "fast": "e3b0c44298fc1c14", "wide": "7a53536648ba86fd", "tris": "1f38df8d2b8c4c8e", "tris36": "63835a46c37f22e0",
        "shade": "4761c8910a96a8d6", "ltris": "f273723a1f0621a5", "mats": "d2dbb3e27daba0c3", "tri_rank": "ced3509026d1fe54", "cam_tris": "c7bd5e674ae7b286",
        "n_records": 839, "n_top": 512, "n_fast": 0, "fast_flat": 0, "n_wide": 207, "max_pending": 9, "order_depth": 18},
    "big_leaf": {"nodes": "4019f54a80f2c8ac", "fast": "e3b0c44298fc1c14", "wide": "e3b0c44298fc1c14", "tris": "a59a769290f0ff25", "tris36": "e3b0c44298fc1c14",
        "shade": "e4aa70c826a02875", "ltris": "f273723a1f0621a5", "mats": "0c17a38b488ba004", "tri_rank": "e3b0c44298fc1c14", "cam_tris": "c7bd5e674ae7b286",
        "n_records": 23, "n_top": 0, "n_fast": 0, "fast_flat": 0, "n_wide": 0, "max_pending": 1, "order_depth": 0},
    "not_nested": {"nodes": "5fc508789124f88b", "fast": "e3b0c44298fc1c14", "wide": "e3b0c44298fc1c14", "tris": "b7f6e586fcb38296", "tris36": "e3b0c44298fc1c14",
        "shade": "3aff54db0c24b2ea", "ltris": "296bcada34d57497", "mats": "d2dbb3e27daba0c3", "tri_rank": "e3b0c44298fc1c14", "cam_tris": "bfce42ee6f1de630",
        "n_records": 5, "n_top": 0, "n_fast": 0, "fast_flat": 0, "n_wide": 0, "max_pending": 1, "order_depth": 0},
    "chain": {"nodes": "7ebce829155c58c1", "fast": "c02f39eb7478d9e3", "wide": "df8e9b6f9b304e96", "tris": "a59a769290f0ff25", "tris36": "4c781396304f2bb2",
        "shade": "e4aa70c826a02875", "ltris": "f273723a1f0621a5", "mats": "0c17a38b488ba004", "tri_rank": "ea3548ec5a662bbd", "cam_tris": "c7bd5e674ae7b286",
        "n_records": 49, "n_top": 0, "n_fast": 30, "fast_flat": 0, "n_wide": 12, "max_pending": 24, "order_depth": 24},
}


def test_pinned_outputs(lib, inputs):
    for name, inp in inputs.items():
        err, out = inp.prepare(lib)
        assert err is None, (name, err)
        assert digest(out) == PINS[name], name


def test_records_of_the_pinned_scenes(inputs, lib):
    """What the pins stand for: the conditions each scene was chosen to reach."""
    got = {name: inp.prepare(lib)[1] for name, inp in inputs.items()}
    assert got["cornell"]["n_fast"] > 0 and got["cornell"]["fast_flat"] == 1       # pruned table, a flat list of leaves
    assert got["glass"]["n_fast"] > 0 and got["glass"]["fast_flat"] == 0
    assert got["mesh"]["n_records"] > 512 and got["mesh"]["n_top"] > 0              # top levels renumbered for the LDS window
    assert got["big_leaf"]["n_records"] == 1 + 2 + 20 and got["big_leaf"]["n_wide"] == 0 and got["big_leaf"]["tri_rank"] == b""
    assert got["not_nested"]["n_wide"] == 0 and got["not_nested"]["n_fast"] == 0
    assert got["chain"]["max_pending"] == 24 and got["chain"]["n_wide"] > 0


def test_rank_table_is_the_reference_visit_order(inputs, lib):
    """tri_rank[1 + t] is triangle t's place in the reference's visit order: visit_rank of test_order_independence.py."""
    for name in ("cornell", "glass", "mesh", "chain"):
        inp = inputs[name]
        rank = np.frombuffer(inp.prepare(lib)[1]["tri_rank"], np.int32)
        assert rank[0] == np.iinfo(np.int32).min and rank[-1] == np.iinfo(np.int32).max, name
        assert np.array_equal(rank[1:-1], visit_rank(inp.boxes, len(inp.tris))), name


def test_max_pending_is_the_reference_stack_depth(inputs, lib):
    for name, inp in inputs.items():
        assert inp.prepare(lib)[1]["max_pending"] == pending_depths(inp.boxes).max(), name



def refusals(cornell, glass):
    """(input, message) for every refusal of cl2_upload_scene, in the order its checks run."""
    n, n_mats = len(cornell.triangles), len(cornell.materials)

    def edit(scene, **change):
        inp = Input(scene)
        for k, v in change.items():
            setattr(inp, k, v)
        return inp

    def tree(*rows):                               # a Box[] of (left, right) rows, each box the whole room
        b = np.zeros(len(rows), cornell.boxes.dtype)
        b["min"], b["max"] = cornell.boxes["min"][0], cornell.boxes["max"][0]
        b["left"], b["right"] = np.array(rows).T
        return edit(cornell, boxes=b)

    def field(array, name, index, value):
        inp = Input(cornell)
        getattr(inp, array)[name][index] = value
        return inp

    counts = (len(cornell.boxes), n, n_mats, 2)
    out = [(edit(cornell, **{a: None}), "NULL scene array") for a in ("boxes", "tris", "mats", "cam", "ltris", "areas", "lidx")]
    out += [(edit(cornell, counts=counts[:k] + (0,) + counts[k + 1:]), "scene needs >=1 box, triangle and light") for k in (0, 1, 3)]
    # 2^27 triangles would take 16 GiB: the count alone, with the scene's small buffer (nothing is read before the check)
    out.append((edit(cornell, counts=(counts[0], 1 << 27) + counts[2:]), "at most 2^27 triangles (leaf records pack begin<<4 | count-1)"))
    out += [(edit(cornell, mats=np.resize(cornell.materials, m)), "material table must have 8..256 entries") for m in (7, 257)]
    out += [(edit(cornell, W=63), "camera resolution differs from the renderer's"),
            (edit(cornell, H=49), "camera resolution differs from the renderer's"),
            (tree((0, n), (0, n)), "box 1 is not reachable from the root"),
            (field("boxes", "left", 0, 9999), "inner box child index out of order/range"),
            (tree((1, 0), (1, 0), (0, n)), "inner box child index out of order/range"),             # a child not after its parent
            (tree((1, 0), (2, 0), (0, n), (0, n), (0, n)), "box has two parents"),
            (tree((1, 0), (0, n + 1), (0, n)), "leaf triangle range out of range"),
            (tree((1, 0), (-1, n), (0, n)), "leaf triangle range out of range"),
            (tree((1, 0), (3, 3), (0, n)), "leaf triangle range out of range"),
            # 63 inner boxes in a row: the last is entered with 62 entries pending
            (chain(glass, 63), "tree too deep: the reference's 64-entry traversal stack would overflow at box 124"),
            (field("tris", "material", 3, n_mats), "triangle material index out of range"),
            (field("tris", "material", 3, -1), "triangle material index out of range"),
            (edit(cornell, lidx=np.array([0, n], np.int32)), "light triangle index out of range"),
            (edit(cornell, lidx=np.array([-1, 0], np.int32)), "light triangle index out of range"),
            (field("ltris", "material", 1, n_mats), "light material index out of range")]
    return out


def test_every_refusal(lib, cornell_small, glass_scene):
    for inp, msg in refusals(cornell_small, glass_scene):
        assert inp.prepare(lib) == (msg, None)
    # one level less is accepted: its last inner box is entered with 61 entries pending and pushes to 63
    assert chain(glass_scene, 62).prepare(lib)[1]["max_pending"] == 62


def test_the_first_failing_check_is_reported(lib, cornell_small, glass_scene):
    """An input with two faults reports the one whose check runs first."""
    faults = refusals(cornell_small, glass_scene)
    first = {msg: k for k, (_, msg) in reversed(list(enumerate(faults)))}
    inp = chain(glass_scene, 63)                                        # too deep ...
    inp.tris["material"][0] = 99                                        # ... and a bad material index: the depth check runs first
    assert inp.prepare(lib)[0].startswith("tree too deep")
    inp.W = 1                                                           # a third fault, found before the tree is looked at
    assert inp.prepare(lib)[0] == "camera resolution differs from the renderer's"
    inp = Input(cornell_small)
    inp.boxes["left"][0] = 9999                                         # a bad child index ...
    inp.lidx = np.array([0, 99], np.int32)                             # ... and a bad light index
    assert inp.prepare(lib)[0] == "inner box child index out of order/range"
    inp.areas = None
    assert inp.prepare(lib)[0] == "NULL scene array"
    assert first["NULL scene array"] < first["box 1 is not reachable from the root"] < first["light material index out of range"]

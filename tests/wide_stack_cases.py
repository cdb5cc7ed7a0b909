"""Scenes, trees and rays of the wide-stack tests (tests/test_wide_stack_cpu.py, tests/test_gpu_wide_stack.py): trees on which the
stack of the 4-wide walk (csrc/bvh_wide.hpp) gets deep in the nearest-first child order while the reference's pending depth --
what the stack was sized from before -- stays small.

    plate_scene(n)      the Cornell room and n parallel one-triangle plates in a row along x; triangles [0, n) are the plates, far
                        to near as seen from plate_rays' origins (beyond the +x end), the room's 16 triangles follow
    left_chain(...)     inner boxes in a row, the deep child at `left` and a leaf at `left + 1`: one box pending on the reference's
                        stack, two more wide-stack entries per wide node for a ray that takes the deep child first
    plate_chain(scene)  the left chain over a plate scene: plate j hangs at chain level j, the room's two leaves of eight at the
                        deep end -- len(plates) + 1 inner boxes
    ploc_tree(scene)    the scene's triangles under the GPU builder's PLOC tree as tests/gpu_bvh_reference.py states it
    random_tree(...)    random uneven splits of a triangle permutation, boxes set exactly"""
import numpy as np

f32 = np.float32
ORIGINS = ([0.0, 1.5, 6.0], [3.5, 4.0, 3.0], [-3.0, 0.5, -3.5], [0.25, 8.5, 0.5])      # the four origins of test_gpu_round6.py
PLATE_X = (-8.0, 7.0)                  # the row of plates; the rays start at x = 8.5
PLATE_MATERIAL = 5


def reordered(scene, order, boxes):
    """The scene with triangle order[i] at place i and `boxes` as its tree; light and camera triangle indices follow."""
    from clive2_amd.scene import Scene
    order = np.asarray(order, np.int64)
    place = np.empty(len(order), np.int64)
    place[order] = np.arange(len(order))
    out = Scene(None, scene.pixel_width, scene.pixel_height, scene.camera, np.ascontiguousarray(scene.triangles[order]), boxes,
                scene.materials, scene.light_triangles, scene.light_counts, scene.light_surface_areas,
                place[np.asarray(scene.light_triangle_indices)].astype(np.int32),
                place[np.asarray(scene.camera_triangle_indices)].astype(np.int32))
    out.validate()
    assert out.triangles[out.light_triangle_indices].tobytes() == np.asarray(scene.light_triangles).tobytes()
    return out


def set_bounds(boxes, b, triangles, tris):
    """Box b bounds triangles `tris` exactly (float32 min / max of their vertices)."""
    v = np.concatenate([triangles[key][tris, :3] for key in ("v0", "v1", "v2")])
    boxes["min"][b, :3], boxes["max"][b, :3] = v.min(axis=0), v.max(axis=0)


def plate_scene(n_plates, width=32, height=18):
    import clive2_amd as c2
    from clive2_amd.load import get_materials
    x = np.linspace(PLATE_X[0], PLATE_X[1], n_plates)
    # slightly tilted, so that a plate's leaf box has a thickness and a hit lies inside it, not on its face
    v = np.stack([np.stack([x, np.full(n_plates, 0.5), np.full(n_plates, -2.0)], axis=1),
                  np.stack([x, np.full(n_plates, 0.5), np.full(n_plates, 2.0)], axis=1),
                  np.stack([x + 0.03, np.full(n_plates, 4.5), np.zeros(n_plates)], axis=1)], axis=1).reshape(-1, 3)
    faces = np.arange(3 * n_plates).reshape(-1, 3)
    scene = c2.create_scene(width, height, np.array([0, 1.5, 6]), np.array([0, 0, -1]),
                            file_specs=[dict(mesh=(v, faces), material=PLATE_MATERIAL)], materials=get_materials())
    t = scene.triangles
    plates = np.flatnonzero(t["material"] == PLATE_MATERIAL)
    assert len(plates) == n_plates and len(t) == n_plates + 16
    plates = plates[np.argsort(t["v0"][plates, 0], kind="stable")]                      # far (low x) to near
    return reordered(scene, np.concatenate([plates, np.flatnonzero(t["material"] != PLATE_MATERIAL)]), scene.boxes)


def left_chain(triangles, leaves):
    """Box[] of len(leaves) - 1 inner boxes in a row: inner box j has leaf j (a triangle range) at left + 1 and the next inner box at
    left; the last one has the last two leaves.  Every box bounds its triangles exactly."""
    from clive2_amd import struct_types as st
    n = len(leaves) - 1
    boxes = np.zeros(2 * n + 1, st.Box)
    inner = lambda j: 0 if j == 0 else 2 * j - 1
    for j in range(n):
        boxes["left"][inner(j)] = 2 * j + 1                                              # children at 2 j + 1 (deep) and 2 j + 2 (leaf j)
        set_bounds(boxes, inner(j), triangles, np.concatenate([np.arange(a, b) for a, b in leaves[j:]]))
    for j, (a, b) in enumerate(leaves):
        at = 2 * j + 2 if j < n else 2 * n - 1
        boxes["left"][at], boxes["right"][at] = a, b
        set_bounds(boxes, at, triangles, np.arange(a, b))
    return boxes


def plate_chain(scene):
    n = int((scene.triangles["material"] == PLATE_MATERIAL).sum())
    leaves = [(j, j + 1) for j in range(n)] + [(n, n + 8), (n + 8, n + 16)]
    return reordered(scene, np.arange(len(scene.triangles)), left_chain(scene.triangles, leaves))


def plate_rays(count, seed=3):
    """Rays from beyond the near end that pierce every plate, slightly tilted: all three direction components are non-zero."""
    rng = np.random.default_rng(seed)
    o = np.stack([np.full(count, 8.5), rng.uniform(1.2, 2.5, count), rng.uniform(-0.5, 0.5, count)], axis=1).astype(f32)
    to = np.stack([np.full(count, -8.5), rng.uniform(1.2, 2.5, count), rng.uniform(-0.5, 0.5, count)], axis=1).astype(f32)
    d = (to - o).astype(f32)
    d = (d / np.sqrt((d * d).sum(axis=1, dtype=f32))[:, None]).astype(f32)
    assert (d != 0).all()
    return o, d


def random_rays(count, seed, toward=None):
    """Origins anywhere in the room; directions uniform, or with toward = (centre, radius) at uniform points of that ball; rays with
    a zero direction component (no 4-wide walk) left out."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-9.5, 9.5, (count, 3)).astype(f32)
    o[:, 1] = rng.uniform(-1.5, 9.0, count).astype(f32)
    d = rng.normal(size=(count, 3)).astype(f32)
    if toward is not None:
        inside = d / np.sqrt((d * d).sum(axis=1))[:, None] * (toward[1] * rng.random(count) ** (1.0 / 3.0))[:, None]
        d = ((np.asarray(toward[0], f32) + inside).astype(f32) - o).astype(f32)
    d = (d / np.sqrt((d * d).sum(axis=1, dtype=f32))[:, None]).astype(f32)
    keep = (d != 0).all(axis=1)
    return np.ascontiguousarray(o[keep]), np.ascontiguousarray(d[keep])


def aimed_rays(scene, material=PLATE_MATERIAL):
    """From each of ORIGINS at every vertex and edge midpoint of the mesh: several triangles tie at one t, hits sit on box faces."""
    mesh = scene.triangles[scene.triangles["material"] == material]
    a, b, c = (mesh[key][:, :3].astype(f32) for key in ("v0", "v1", "v2"))
    targets = np.unique(np.concatenate([a, b, c, (a + b) / 2, (b + c) / 2, (c + a) / 2]).astype(f32), axis=0)
    os_, ds = [], []
    for origin in ORIGINS:
        o = np.broadcast_to(np.asarray(origin, f32), targets.shape).copy()
        d = (targets - o).astype(f32)
        d = (d / np.sqrt((d * d).sum(axis=1, dtype=f32))[:, None]).astype(f32)
        keep = (d != 0).all(axis=1)
        os_.append(o[keep]); ds.append(d[keep])
    return np.ascontiguousarray(np.concatenate(os_)), np.ascontiguousarray(np.concatenate(ds))


def glass_rays(scene):
    """The rays of the glass scenes' trees: aimed at the sphere's vertices and edge midpoints, 5,000 random ones through the sphere
    and 1,000 anywhere.  (Most rays go for the mesh, where these trees are deep -- and a tree with one-triangle leaves keeps each
    wall triangle in a flat box: every other ray that ends on a wall hits it in front of that box's entry distance, the case in which
    the two child orders may differ.)"""
    sets = [aimed_rays(scene), random_rays(5000, 12, toward=((0.0, 1.0, 0.0), 1.9)), random_rays(1000, 13)]
    return np.concatenate([s[0] for s in sets]), np.concatenate([s[1] for s in sets])


def glass(sub, width=32, height=18, **kw):
    """The glass scene of the suite (conftest.py) at another subdivision and frame."""
    import clive2_amd as c2
    from clive2_amd.load import get_materials
    from clive2_amd.meshes import icosphere
    mats = get_materials()
    mats["alpha"][5] = 0.1
    v, f = icosphere(sub, radius=2.0, center=(0.0, 1.0, 0.0))
    return c2.create_scene(width, height, np.array([0, 1.5, 6]), np.array([0, 0, -1]), file_specs=[dict(mesh=(v, f), material=5)],
                           materials=mats, **kw)


def ploc_tree(scene, max_members=1):
    import gpu_bvh_reference as ref
    t = scene.triangles
    v = np.stack([t[key][:, :3] for key in ("v0", "v1", "v2")]).astype(np.float64)
    boxes, perm, prepared = ref.build(v.min(axis=0), v.max(axis=0), max_members)
    assert prepared.path == "ploc"
    return reordered(scene, perm, boxes)


def random_tree(scene, seed, leaf_max=3, lean=0.85):
    """Splits of a random triangle permutation at random uneven places; with probability `lean` the smaller part goes to left + 1,
    so the reference's stack stays shallow while the tree gets deep.  Numbered breadth-first, children side by side."""
    from clive2_amd import struct_types as st
    rng = np.random.default_rng(seed)
    n = len(scene.triangles)
    order = rng.permutation(n)
    triangles = scene.triangles[order]
    rows, queue = [[0, n, 0]], [0]                                                    # [first, last, left child]
    while queue:
        at = queue.pop(0)
        a, b, _ = rows[at]
        if b - a <= leaf_max and (b - a == 1 or rng.random() < 0.5):
            continue
        small = 1 + int((b - a - 1) // 2 * rng.random() ** 3)
        cut = b - small if rng.random() < lean else a + small                          # [a, cut) at left, [cut, b) at left + 1
        rows[at][2] = len(rows)
        queue += [len(rows), len(rows) + 1]
        rows += [[a, cut, 0], [cut, b, 0]]
    boxes = np.zeros(len(rows), st.Box)
    for i, (a, b, left) in enumerate(rows):
        boxes["left"][i], boxes["right"][i] = (left, 0) if left else (a, b)
        set_bounds(boxes, i, triangles, np.arange(a, b))
    return reordered(scene, order, boxes)

"""Many-emitter scenes and other camera films (tests/test_emitter_scenes_cpu.py, tests/test_gpu_emitters.py): the two ends of every
path at values the Cornell box never gives them -- the box has two emitters of equal area and one material, side by side in the
triangle array, and a film of height 1 with square pixels.  Everything is deterministic; the helper holds no tests.

Material tables (table(40) moves the coloured emitter material to index 35, past LDS_MAT_CAP = 32 of csrc/scene_layout.hpp):

    index 8 / 35   coloured diffuse emitter, emission (4, 0.5, 0)
    9              a black emitter: diffuse, emission 0
    10             a glass emitter (type 1)
    11             a rough mirror emitter (type 3, alpha 0.2)
    0              a type-2 emitter (entry 0 of the reference's table, a dielectric nothing here uses otherwise)

Scenes (32 x 18, the Cornell walls; `ceiling` = the box's two emitter triangles of material 6):

    lamps_lds        ceiling, an icosphere(1) lamp of 80 emitters cycling through the five emitter materials, TINY (legs 1e-3, area
                     5e-7, a hair above the floor) and BACK (a wall-mounted emitter that faces the back wall: the camera sees its
                     back): 98 triangles, 84 lights, tree and triangles in LDS
    lamps_streamed   no ceiling; an icosphere(3) lamp (1280 emitters), TINY and a noisy_blob(3) of glass: 2575 triangles, 1281 lights,
                     the tree streams from memory
    one_light        ONE ceiling triangle: light_count == 1, the index clamp is the identity
    three_lights     ceiling and BACK: a count that is no power of two, unequal areas

Films (40 x 23: pixels are not square; the plain box): film_wide (phys 1.2 x 0.5), film_big (phys 3.0 x 2.5), film_rolled (an
oblique camera rolled 0.6 rad about its axis).

plant(seeds, entries) writes into seeds[k, 0] a state whose next xorshift state is >= 0xFFFFFF80: xorshift_random returns exactly
1.0 for it, the light index is count * 1.0 and only the clamp keeps it in the table."""
import functools

import numpy as np

f32 = np.float32
W, H = 32, 18
FILM_W, FILM_H = 40, 23
CAM_CENTER, CAM_DIRECTION = np.array([0, 1.5, 6.0]), np.array([0, 0, -1.0])
SCENES = ("lamps_lds", "lamps_streamed", "one_light", "three_lights")
FILMS = ("film_wide", "film_big", "film_rolled")
CASES = SCENES + FILMS
COLOURED, BLACK, GLASS, MIRROR, TYPE2 = "coloured", "black", "glass", "mirror", "type2"
CYCLE = (TYPE2, COLOURED, BLACK, GLASS, MIRROR)        # in this order lamps_lds shows the camera whole pixels of each kind
NON_DIFFUSE = (GLASS, MIRROR, TYPE2)
BLOB_MATERIAL = 5
# lamps_lds: near the camera (its field of view is 110 degrees), so that a face of the lamp is several pixels wide
LAMP_CENTER = {"lamps_lds": (-3.0, 2.0, 2.0), "lamps_streamed": (-3.0, 3.0, -2.0)}
LAMP_RADIUS = {"lamps_lds": 2.0, "lamps_streamed": 1.5}


def emitter_materials(n_mats):
    """{name: index} of the emitter materials in table(n_mats)"""
    return {COLOURED: 8 if n_mats <= 32 else 35, BLACK: 9, GLASS: 10, MIRROR: 11, TYPE2: 0}


def table(n_mats=12):
    """T12 (the resolve stage's slim kernel, materials in LDS) or T40 (more than LDS_MAT_CAP: the table stays in global memory)."""
    from clive2_amd import struct_types as st
    from clive2_amd.load import get_materials
    assert n_mats in (12, 40)
    m = np.zeros(n_mats, dtype=st.Material)
    m[:8] = get_materials()
    m[8:] = m[4]                                                       # the entries no triangle uses: white, diffuse
    m["alpha"][BLOB_MATERIAL] = 0.1
    e = emitter_materials(n_mats)
    for name, colour, emission, kind, alpha in ((COLOURED, (0.8, 0.8, 0.8), (4.0, 0.5, 0.0), 0, 0.0),
                                                (BLACK, (0.6, 0.7, 0.8), (0.0, 0.0, 0.0), 0, 0.0),
                                                (GLASS, (0.9, 0.9, 0.9), (0.5, 2.0, 1.0), 1, 0.0),
                                                (MIRROR, (0.9, 0.8, 0.7), (1.0, 1.0, 3.0), 3, 0.2),
                                                (TYPE2, (0.7, 0.9, 0.8), (2.0, 0.25, 0.75), 2, 0.1)):
        i = e[name]
        m["color"][i, :3], m["emission"][i, :3], m["type"][i], m["alpha"][i], m["ior"][i] = colour, emission, kind, alpha, 1.5
        m["color"][i, 3] = m["emission"][i, 3] = 0.0
    return m


def _emitter(v0, v1, v2, material):
    from clive2_amd.load import Triangle
    return Triangle(np.asarray(v0, np.float64), np.asarray(v1, np.float64), np.asarray(v2, np.float64), material=material, emitter=True)


def lamp(sub, center, radius, e):
    """The faces of an icosphere as emitters, face k of material CYCLE[(k + k // 20) % 5] (the four children of a face are 20 * 4^j
    apart: k % 5 alone would give them one material)"""
    from clive2_amd.meshes import icosphere
    v, f = icosphere(sub, radius=radius, center=center)
    return [_emitter(*v[face], e[CYCLE[(k + k // 20) % len(CYCLE)]]) for k, face in enumerate(f)]


def tiny(e):
    """Legs 1e-3, area 5e-7, 0.01 above the floor, facing up"""
    v0 = np.array([2.0, -1.99, 1.0])
    return _emitter(v0, v0 + [0, 0, 1e-3], v0 + [1e-3, 0, 0], e[COLOURED])


def back(e):
    """Half a unit in front of the back wall and facing it: area 3; the camera sees its back"""
    return _emitter([2.0, 1.0, -9.5], [2.0, 3.0, -9.5], [5.0, 1.0, -9.5], e[COLOURED])


def room(name, e):
    """The enclosure of scene `name` as load.Triangle objects"""
    from clive2_amd.load import triangles_for_box
    box = triangles_for_box()
    walls, ceiling = [t for t in box if not t.emitter], [t for t in box if t.emitter]
    if name == "lamps_lds":
        return walls + ceiling + lamp(1, LAMP_CENTER[name], LAMP_RADIUS[name], e) + [tiny(e), back(e)]
    if name == "lamps_streamed":
        return walls + lamp(3, LAMP_CENTER[name], LAMP_RADIUS[name], e) + [tiny(e)]
    if name == "one_light":
        return walls + ceiling[:1]
    if name == "three_lights":
        return walls + ceiling + [back(e)]
    raise ValueError(name)


def film_camera(name):
    from clive2_amd.camera import Camera
    if name == "film_wide":
        return Camera(center=CAM_CENTER, direction=CAM_DIRECTION, phys_width=1.2, phys_height=0.5, pixel_width=FILM_W, pixel_height=FILM_H)
    if name == "film_big":
        return Camera(center=CAM_CENTER, direction=CAM_DIRECTION, phys_width=3.0, phys_height=2.5, pixel_width=FILM_W, pixel_height=FILM_H)
    if name == "film_rolled":
        d = np.array([-0.3, -0.15, -1.0])
        cam = Camera(center=np.array([1.0, 2.0, 6.0]), direction=d / np.linalg.norm(d), phys_width=FILM_W / FILM_H, phys_height=1.0,
                     pixel_width=FILM_W, pixel_height=FILM_H)
        return rolled(cam, 0.6)
    raise ValueError(name)


def rolled(cam, angle):
    """`cam` turned by `angle` about its viewing direction: dx and dy rotated, and what Camera.__init__ derives from them again"""
    c, s = np.cos(angle), np.sin(angle)
    cam.dx, cam.dy = c * cam.dx + s * cam.dy, c * cam.dy - s * cam.dx
    cam.dx_dp = cam.dx * (cam.phys_width / cam.pixel_width)
    cam.dy_dp = cam.dy * (cam.phys_height / cam.pixel_height)
    cam.origin = cam.center - cam.dx * cam.phys_width / 2 - cam.dy * cam.phys_height / 2
    return cam


def scene_around(camera, enclosure, materials, builder="numpy", meshes=(), max_members=None):
    """create_scene's assembly around a given Camera (clive2_amd/scene.py: create_scene builds its own, of film W/H x 1).
    `meshes`: file specs with "mesh": (vertices, faces), "material" and "offset", as create_scene takes them."""
    from clive2_amd import struct_types as st
    from clive2_amd.bvh import FastTreeBox, construct_BVH, np_flatten_bvh
    from clive2_amd.load import camera_geometry, fast_load
    from clive2_amd.scene import Scene
    soups = [FastTreeBox.from_triangle_objects(camera_geometry(camera) + list(enclosure))]
    for spec in meshes:
        v, f = spec["mesh"]
        soups.append(fast_load(np.asarray(v) + spec.get("offset", np.zeros(3)), np.asarray(f), material=spec.get("material", 0)))
    soup = FastTreeBox.concat(soups) if len(soups) > 1 else soups[0]
    boxes, tris = np_flatten_bvh(construct_BVH(soup, builder=builder, max_members=max_members))
    light_ids = np.flatnonzero(tris["is_light"]).astype(np.int32)
    lt = tris[light_ids]
    areas = (np.linalg.norm(np.cross((lt["v1"] - lt["v0"])[:, :3], (lt["v2"] - lt["v0"])[:, :3]), axis=1) / 2).astype(f32)
    sc = Scene(device=None, pixel_width=camera.pixel_width, pixel_height=camera.pixel_height, camera=np.array([camera.to_struct()]),
               triangles=tris, boxes=boxes, materials=np.asarray(materials, dtype=st.Material), light_triangles=lt,
               light_counts=np.array(len(light_ids), dtype=np.int32), light_surface_areas=areas, light_triangle_indices=light_ids,
               camera_triangle_indices=np.flatnonzero(tris["is_camera"]).astype(np.int32))
    sc.validate()
    return sc


@functools.lru_cache(maxsize=None)
def scene(name, n_mats=12, builder="numpy", w=W, h=H):
    """Scene `name` of SCENES or FILMS (films: always FILM_W x FILM_H) with table(n_mats); never written by a test."""
    import clive2_amd as c2
    from clive2_amd.load import triangles_for_box
    from clive2_amd.meshes import noisy_blob
    mats = table(n_mats)
    if name in FILMS:
        return scene_around(film_camera(name), triangles_for_box(), mats, builder)
    specs = None
    if name == "lamps_streamed":
        specs = [dict(mesh=noisy_blob(3, radius=1.6, center=(3.0, 0.5, -1.0), seed=11), material=BLOB_MATERIAL)]
    return c2.create_scene(w, h, CAM_CENTER, CAM_DIRECTION, file_specs=specs, materials=mats, bvh_builder=builder,
                           room=room(name, emitter_materials(n_mats)))


# ---- seeds ----
def xorshift_step(x):
    x = int(x) & 0xFFFFFFFF
    x ^= (x << 13) & 0xFFFFFFFF
    x ^= x >> 17
    x ^= (x << 5) & 0xFFFFFFFF
    return x


def xorshift_before(y):
    """The state that steps to y: the step is a bijection of the 32-bit words (each of its three shifts-and-xors is undone by
    repeating it with doubled shifts until the shift leaves the word)."""
    x = target = int(y) & 0xFFFFFFFF
    for k in (5, 10, 20):
        x ^= (x << k) & 0xFFFFFFFF
    x ^= x >> 17
    for k in (13, 26):
        x ^= (x << k) & 0xFFFFFFFF
    assert xorshift_step(x) == target
    return x


# next states whose float32 quotient by 2^32 is exactly 1.0: the smallest one, the largest, and one between
PLANTED_NEXT = (0xFFFFFF80, 0xFFFFFFFF, 0xFFFFFFF0)


def planted_entries(batch):
    """The first and last entry of the first wave, of the second wave and of the frame, and one in the middle"""
    return sorted({0, 63, 64, 127, batch // 2 + 5, batch - 64, batch - 1})


def seeds(batch, planted=False):
    from clive2_amd.renderer import make_seeds
    s = make_seeds(batch)
    if planted:
        for j, k in enumerate(planted_entries(batch)):
            s[k, 0] = xorshift_before(PLANTED_NEXT[j % len(PLANTED_NEXT)])
    return s


# ---- pixels that see one kind of emitter only ----
def pixels_by_first_hit(sc, traverse):
    """(emitting, dark): bool [W*H] each.  `emitting`: every film point of the pixel sees the front of a diffuse emitting triangle.
    `dark`: every film point of the pixel AND of its eight neighbours sees the front of an emitter that gives a one-edge path
    nothing -- the black one, or one of a material of type > 0 (a directly seen specular emitter zeroes p_values[s] of the pair
    s = 0, t = 2, trace.metal:759-764, and the t = 1 projection leaves a specular vertex out, :577); the neighbours, because
    finalize_samples spreads a pixel's sample over the 3 x 3 pixels around it.

    Pixel (x, y) owns the film coordinates [x, x + 1] of its camera rays (the jitter's whole range) and [x - 0.5, x + 0.5) of the
    t = 1 splats, whose pixel index is ROUNDED (trace.metal:602): its film points are [x - 0.5, x + 1] x
    [y - 0.5, y + 1], cast on a grid of step 0.25 (the lamp's faces are pixels wide, and nothing stands between the camera and
    the lamp).  Column 0 is left out (a rounded x of W lands there, a row further on).  traverse(rays) -> (triangle, ...)."""
    from clive2_amd import struct_types as st
    c = sc.camera.reshape(-1)[0]
    Wp, Hp = int(c["pixel_width"]), int(c["pixel_height"])
    centre, focal = c["center"][:3].astype(np.float64), c["focal_point"][:3].astype(np.float64)
    dx, dy = c["dx"][:3].astype(np.float64), c["dy"][:3].astype(np.float64)
    # one ray per grid point of the whole film and a margin of two pixels: grid point (i, j) is the film coordinate (i, j) / 4 - 2
    gx, gy = np.meshgrid(np.arange(4 * (Wp + 4) + 1), np.arange(4 * (Hp + 4) + 1))
    fx, fy = gx.reshape(-1) / 4.0 - 2.0, gy.reshape(-1) / 4.0 - 2.0
    o = centre + ((fx - 0.5 * Wp) / Wp)[:, None] * dx * float(c["phys_width"]) + ((fy - 0.5 * Hp) / Hp)[:, None] * dy * float(c["phys_height"])
    d = focal - o
    rays = np.zeros(len(fx), st.Ray)
    rays["origin"][:, :3], rays["direction"][:, :3] = o, d / np.linalg.norm(d, axis=1)[:, None]
    with np.errstate(divide="ignore"):
        rays["inv_direction"][:, :3] = f32(1.0) / rays["direction"][:, :3]
    tri = traverse(rays)[0]
    T = sc.triangles[np.maximum(tri, 0)]
    front = (tri >= 0) & (T["is_light"] != 0) & ((rays["direction"][:, :3] * T["normal"][:, :3]).sum(axis=1) < 0)
    emits = (sc.materials["emission"][T["material"], :3] > 0).any(axis=1)
    diffuse = sc.materials["type"][T["material"]] == 0
    lit = (front & emits & diffuse).reshape(gx.shape)
    nothing = (front & ~(emits & diffuse)).reshape(gx.shape)

    def every(grid, lo, hi):
        """bool [Hp, Wp]: `grid` holds at every grid point of [x + lo, x + hi] x [y + lo, y + hi]"""
        out = np.ones((Hp, Wp), bool)
        for j in range(int(4 * (lo + 2)), int(4 * (hi + 2)) + 1):
            for i in range(int(4 * (lo + 2)), int(4 * (hi + 2)) + 1):
                out &= grid[j:j + 4 * Hp:4, i:i + 4 * Wp:4]
        return out
    emitting, dark = every(lit, -0.5, 1.0), every(nothing, -1.5, 2.0)
    emitting[:, 0] = dark[:, 0] = False
    return emitting.reshape(-1), dark.reshape(-1)


# ---- what a case exercises, counted on an oracle ----
def live(paths):
    return np.arange(paths["rays"].shape[1])[None, :] < paths["length"][:, None]


def emitter_vertices(sc, paths):
    """bool [B, 8]: the path's vertices >= 1 that lie on an emitter triangle"""
    tri = paths["rays"]["triangle"]
    on = live(paths) & (tri >= 0) & (sc.triangles["is_light"][np.maximum(tri, 0)] != 0)
    on[:, 0] = False
    return on


def tally(sc, o, counts=None):
    """Adds what the sample `o` (an OracleRenderer after run_sample) holds to `counts`: camera vertices on emitters, emitter vertices
    of either subpath met from the front (hit_light) and from the back, light-subpath vertices >= 1 by emitter material, NaN
    vertices."""
    from path_compare import nan_vertices
    c = counts or dict(camera_on_emitters=0, front=0, back=0, light_by_material={}, nan_vertices=0, vertices=0)
    for kind, paths in (("camera", o.out_camera_paths), ("light", o.out_light_paths)):
        on = emitter_vertices(sc, paths)
        front = paths["rays"]["hit_light"] >= 0
        c["front"] += int((on & front).sum())
        c["back"] += int((on & ~front).sum())
        assert not (front & live(paths) & ~on)[:, 1:].any()                  # hit_light only on emitters
        if kind == "camera":
            c["camera_on_emitters"] += int(on.sum())
        else:
            mat = sc.triangles["material"][np.maximum(paths["rays"]["triangle"], 0)][on]
            for m in np.unique(mat):
                c["light_by_material"][int(m)] = c["light_by_material"].get(int(m), 0) + int((mat == m).sum())
        bad, n = nan_vertices(paths)
        c["nan_vertices"] += bad
        c["vertices"] += n
    return c

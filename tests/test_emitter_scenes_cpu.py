"""CPU: the scenes and films of tests/emitter_scenes.py on the oracle -- held to something independent of it, and counted, so that
tests/test_gpu_emitters.py compares the device with a reference that is right and with cases that exercise what they claim to.

Vertex 0 of the light subpath (orc_generate_light_rays) against oracle/np_kernels.generate_light_rays bit for bit, and against a
float64 statement written here: the light index, the origin on that light's triangle, 1 / (n * area) of the SAME light, its own
material's emission, its own triangle index -- on every case, planted seeds included.  prepare_scene's light, shading and material
records row by row.  Floors on what the cases bring, at about half of what they measured, and the caps on NaN vertices and
non-finite addends.

Measured on the oracle, two samples, numpy builder, make_seeds(W * H) (T12 and T40 give the same counts):

    case             lights  chosen at vertex 0   camera vertices   emitter vertices   light-subpath vertices >= 1 on emitters of
                             (sample 1)           on emitters       front / back       glass / rough mirror / type 2
    lamps_lds        84      84                   814               721 / 395          34 / 30 / 33
    lamps_streamed   1281    471                  164               217 / 73           26 / 32 / 20
    one_light        1       1                    55                67 / 44            -
    three_lights     3       3                    121               321 / 62           -
    film_wide        2       2                    134               231 / 71           -
    film_big         2       2                    168               262 / 74           -
    film_rolled      2       2                    129               218 / 78           -

(Back: the vertex lies on an emitter and hit_light is -1.  On the box that is the gap between the ceiling and the light 0.5 below
it.)  Light-image pixels > 0 per sample, of 920: film_wide 706 and 685, film_big 683 and 673, film_rolled 616 and 625 (of 576:
lamps_lds 307 and 309, lamps_streamed 372 and 366).  NaN vertices: 0 of some 13,700 (scenes) and 22,080 (films) on every case.
Pixels with a non-finite addend: 0 on every case.  With the planted seeds the seven planted entries take the LAST light on every
case.  lamps_lds has 25 pixels that see only diffuse emitting faces of the lamp and 11 that, with their eight neighbours, see only
black and specular ones."""
import numpy as np
import pytest

import emitter_scenes as es
import masked_oracle as mo
from test_resolve_form_cpu import lib as resolve_form  # noqa: F401 (the g++ build of resolve_runs_slim: a fixture)
from test_scene_prep_cpu import Input, lib  # noqa: F401 (the g++ build of csrc/scene_prep.hpp: a fixture)

f32 = np.float32
DELTA = 0.0001                                                          # trace.metal:5
# floors, at about half of the measured values of the table above
CAMERA_ON_EMITTERS = {"lamps_lds": 400, "lamps_streamed": 75, "one_light": 25, "three_lights": 60, "film_wide": 60, "film_big": 80,
                      "film_rolled": 60}
CHOSEN = {"lamps_lds": 84, "lamps_streamed": 200, "one_light": 1, "three_lights": 3, "film_wide": 2, "film_big": 2, "film_rolled": 2}
LIGHT_PIXELS = 320                                                      # of 920, every film, each sample
EMITTING_PIXELS, DARK_PIXELS = 12, 5                                    # lamps_lds (es.pixels_by_first_hit): 25 and 11


@pytest.fixture(scope="module")
def samples(oracle_mod):
    """case -> two samples of the oracle: the tally, the lights chosen in sample 1, the light image's pixels > 0 per sample"""
    made = {}

    def get(name, n_mats=12):
        if (name, n_mats) not in made:
            sc = es.scene(name, n_mats)
            o = oracle_mod.OracleRenderer(sc, seeds=es.seeds(sc.pixel_width * sc.pixel_height))
            counts, chosen, pixels = None, None, []
            for k in range(2):
                o.run_sample()
                if k == 0:
                    chosen = len(np.unique(o.out_light_paths["rays"]["triangle"][:, 0]))
                counts = es.tally(sc, o, counts)
                pixels.append(int((o.out_light_image[:, :3] > 0).any(axis=1).sum()))
            made[name, n_mats] = dict(scene=sc, counts=counts, chosen=chosen, pixels=pixels, image=o.summed_image.copy())
        return made[name, n_mats]
    return get


def _draw(state):
    """xorshift_random of each state, as exact Python integers and one float32 rounding: (next states, draws)"""
    nxt = np.array([es.xorshift_step(s) for s in state], np.uint32)
    return nxt, (nxt.astype(np.float64).astype(f32).astype(np.float64) / 2.0 ** 32).astype(f32)


def test_planted_states_draw_exactly_one():
    assert es.xorshift_before(0xFFFFFFF0) == 0x2AC9AE73
    for y in es.PLANTED_NEXT:
        nxt, u = _draw([es.xorshift_before(y)])
        assert nxt[0] == y and u[0] == f32(1.0)
    assert _draw([es.xorshift_before(0xFFFFFF7F)])[1][0] < f32(1.0)      # the largest state that draws less than 1


@pytest.mark.parametrize("planted", [False, True])
@pytest.mark.parametrize("n_mats", [12, 40])
@pytest.mark.parametrize("name", es.CASES)
def test_vertex_0_of_the_light_subpath(name, n_mats, planted, oracle_mod):
    from oracle import np_kernels as npk
    sc = es.scene(name, n_mats)
    B = sc.pixel_width * sc.pixel_height
    seeds0 = es.seeds(B, planted)
    o = oracle_mod.OracleRenderer(sc, seeds=seeds0)
    o.make_light_rays()
    got = o.light_ray_buffer
    # the numpy restatement, bit for bit
    org, d, l_imp, li, seeds1 = npk.generate_light_rays(sc.light_triangles, sc.light_surface_areas, seeds0)
    assert got["origin"][:, :3].tobytes() == org.tobytes()
    assert got["direction"][:, :3].tobytes() == d.tobytes()
    assert got["l_importance"].tobytes() == l_imp.tobytes()
    assert np.array_equal(got["triangle"], sc.light_triangle_indices[li])
    assert np.array_equal(o.rand_buffer, seeds1)
    # the float64 statement
    n = int(sc.light_counts)
    _, u = _draw(seeds0[:, 0])
    index = np.minimum((u.astype(np.float64) * n).astype(f32).astype(np.int64), n - 1)      # the product of two float32, rounded once
    assert np.array_equal(index, li)
    rows = es.planted_entries(B)
    if planted:
        assert (u[rows] == f32(1.0)).all() and (index[rows] == n - 1).all()          # count * 1.0 = count: the clamp alone holds it
        assert (got["triangle"][rows] == sc.light_triangle_indices[-1]).all()
    else:
        assert (u < f32(1.0)).all()
    assert np.array_equal(got["triangle"], sc.light_triangle_indices[index])
    L = sc.light_triangles[index]
    area = sc.light_surface_areas[index].astype(np.float64)
    want = (1.0 / (f32(n) * area).astype(f32).astype(np.float64)).astype(f32)
    assert got["l_importance"].tobytes() == want.tobytes()
    own = sc.triangles[got["triangle"]]
    assert np.array_equal(own["material"], L["material"]) and np.array_equal(got["material"], own["material"])
    assert got["color"][:, :3].tobytes() == np.ascontiguousarray(sc.materials["emission"][own["material"], :3]).tobytes()
    assert got["normal"][:, :3].tobytes() == np.ascontiguousarray(own["normal"][:, :3]).tobytes()
    # the origin lies on that triangle, DELTA along its normal, within 1e-5
    v0, v1, v2 = (own[k][:, :3].astype(np.float64) for k in ("v0", "v1", "v2"))
    nrm = own["normal"][:, :3].astype(np.float64)
    p = got["origin"][:, :3].astype(np.float64) - DELTA * nrm
    e1, e2, r = v1 - v0, v2 - v0, p - v0
    a11, a12, a22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    b1, b2 = (r * e1).sum(1), (r * e2).sum(1)
    det = a11 * a22 - a12 * a12
    s, t = np.clip((b1 * a22 - b2 * a12) / det, 0, 1), np.clip((b2 * a11 - b1 * a12) / det, 0, 1)
    over = np.maximum(s + t, 1.0)
    q = v0 + (s / over)[:, None] * e1 + (t / over)[:, None] * e2                       # a point of the triangle near p
    assert np.linalg.norm(p - q, axis=1).max() <= 1e-5
    # the rays leave on the normal's side
    assert ((got["direction"][:, :3].astype(np.float64) * nrm).sum(1) >= -1e-6).all()


@pytest.mark.parametrize("n_mats", [12, 40])
@pytest.mark.parametrize("name", ["lamps_lds", "lamps_streamed"])
def test_prepared_light_shading_and_material_records(name, n_mats, lib):  # noqa: F811
    """prepare_scene: `ltris` row l = {v0, v1, v2, normal, material} of scene.light_triangles[l]; the is_light and material words of
    `shade`; `mats` = the table."""
    sc = es.scene(name, n_mats)
    err, out = Input(sc).prepare(lib)
    assert err is None, err
    n, nt = int(sc.light_counts), len(sc.triangles)
    lt = np.frombuffer(out["ltris"], f32).reshape(n, 5, 4)
    for row, field in enumerate(("v0", "v1", "v2", "normal")):
        assert lt[:, row, :3].tobytes() == np.ascontiguousarray(sc.light_triangles[field][:, :3]).tobytes(), field
        assert not lt[:, row, 3].any()
    assert np.array_equal(lt[:, 4, 0].copy().view(np.int32), sc.light_triangles["material"])
    assert not lt[:, 4, 1:].any()
    assert np.array_equal(sc.light_triangles["material"], sc.triangles["material"][sc.light_triangle_indices])
    assert len(np.unique(sc.light_triangles["material"])) >= 5                    # the rows differ: a wrong stride cannot hide
    shade = np.frombuffer(out["shade"], f32).reshape(nt, 4, 4)
    assert np.array_equal(shade[:, 0, 3].copy().view(np.int32), sc.triangles["material"])
    assert np.array_equal(shade[:, 1, 3].copy().view(np.int32), (sc.triangles["is_light"] != 0).astype(np.int32))
    assert np.array_equal(shade[:, 2, 3].copy().view(np.int32), (sc.triangles["is_camera"] != 0).astype(np.int32))
    assert shade[:, 3, :3].tobytes() == np.ascontiguousarray(sc.triangles["normal"][:, :3]).tobytes()
    mats = np.frombuffer(out["mats"], f32).reshape(n_mats, 12)
    M = sc.materials
    assert mats[:, 0:3].tobytes() == np.ascontiguousarray(M["color"][:, :3]).tobytes()
    assert np.array_equal(mats[:, 3].copy().view(np.int32), M["type"])
    assert mats[:, 4:7].tobytes() == np.ascontiguousarray(M["emission"][:, :3]).tobytes()
    assert mats[:, 7].tobytes() == M["alpha"].tobytes() and mats[:, 8].tobytes() == M["ior"].tobytes()
    # the lights are no single run of the triangle array and do not start it: light l is not triangle first + l
    idx = np.asarray(sc.light_triangle_indices)
    assert idx[0] > 0 and (np.diff(idx) > 1).any()


def test_the_scenes_are_what_the_header_says():
    counts = {name: (len(es.scene(name).triangles), int(es.scene(name).light_counts)) for name in es.SCENES}
    assert counts == {"lamps_lds": (98, 84), "lamps_streamed": (2575, 1281), "one_light": (15, 1), "three_lights": (17, 3)}
    a = es.scene("lamps_lds").light_surface_areas
    assert a.min() < 5.1e-7 and a.max() == 12.5
    assert np.allclose(np.sort(es.scene("three_lights").light_surface_areas), [3.0, 12.5, 12.5])
    for n_mats in (12, 40):
        e, m = es.emitter_materials(n_mats), es.table(n_mats)
        assert len(m) == n_mats and len(set(e.values())) == 5
        assert {k: int(m["type"][e[k]]) for k in es.CYCLE} == {es.COLOURED: 0, es.BLACK: 0, es.GLASS: 1, es.MIRROR: 3, es.TYPE2: 2}
        assert not m["emission"][e[es.BLACK]].any() and all(m["emission"][e[k]].any() for k in es.CYCLE if k != es.BLACK)
    assert es.emitter_materials(40)[es.COLOURED] >= 32
    for name, phys in (("film_wide", (1.2, 0.5)), ("film_big", (3.0, 2.5)), ("film_rolled", (40 / 23, 1.0))):
        c = es.scene(name).camera.reshape(-1)[0]
        assert (c["pixel_width"], c["pixel_height"]) == (40, 23)
        assert np.allclose([c["phys_width"], c["phys_height"]], phys)
        dx, dy, d = c["dx"][:3], c["dy"][:3], c["direction"][:3]
        assert np.allclose([dx @ dy, dx @ d, dy @ d, dx @ dx, dy @ dy], [0, 0, 0, 1, 1], atol=1e-6)
    c = es.scene("film_rolled").camera.reshape(-1)[0]
    assert abs(c["dx"][1]) > 0.3 and abs(c["dy"][0]) > 0.3                            # rolled: neither axis is level
    # the camera quad is the film: its corner is center - dx w / 2 - dy h / 2
    sc = es.scene("film_rolled")
    quad = sc.triangles[sc.camera_triangle_indices]
    corner = c["center"][:3] - c["dx"][:3] * c["phys_width"] / 2 - c["dy"][:3] * c["phys_height"] / 2
    assert np.allclose(quad["v0"][:, :3], corner, atol=1e-6)


@pytest.mark.parametrize("name", es.CASES)
def test_floors_on_what_the_cases_exercise(name, samples):
    s = samples(name)
    sc, c = s["scene"], s["counts"]
    print(name, s["chosen"], c, s["pixels"])
    assert s["chosen"] >= CHOSEN[name] and s["chosen"] <= int(sc.light_counts)
    assert c["camera_on_emitters"] >= CAMERA_ON_EMITTERS[name]
    assert c["front"] >= 30 and c["back"] >= 20                                     # met from both sides
    if name.startswith("lamps"):
        e = es.emitter_materials(12)
        for kind in es.NON_DIFFUSE:
            assert c["light_by_material"].get(e[kind], 0) >= 3, kind
    if name in es.FILMS:
        assert min(s["pixels"]) >= LIGHT_PIXELS
    else:
        assert min(s["pixels"]) > 0
    assert np.isfinite(s["image"]).all()
    # caps: conditions, not measurements
    assert c["nan_vertices"] < 0.01 * c["vertices"]
    B = sc.pixel_width * sc.pixel_height
    bad = int(mo.Render(sc, es.seeds(B), 2).render(None).nonfinite.sum())
    assert bad <= B // mo.NONFINITE_CAP, bad


def test_t40_walks_the_same_paths(samples):
    """The coloured emitter's material index is the only difference: the same counts, with 35 in place of 8."""
    for name in es.SCENES:
        a, b = samples(name, 12)["counts"], samples(name, 40)["counts"]
        swap = {8: 35}
        assert {swap.get(k, k): v for k, v in a["light_by_material"].items()} == b["light_by_material"]
        assert {k: v for k, v in a.items() if k != "light_by_material"} == {k: v for k, v in b.items() if k != "light_by_material"}
        assert samples(name, 12)["image"].tobytes() == samples(name, 40)["image"].tobytes()


def test_emission_layer_on_pixels_of_one_emitter(oracle_mod):
    """lamps_lds has pixels that see only diffuse emitting faces of the lamp, and pixels that -- with their eight neighbours -- see
    only black and specular ones; the masked oracle's emission layer (paths of one edge: s = 0, t = 2 and s = 1, t = 1) is
    non-zero on the first and zero on the second (es.pixels_by_first_hit says why)."""
    from clive2_amd import strategies as S
    sc = es.scene("lamps_lds")
    emitting, dark = es.pixels_by_first_hit(sc, lambda rays: oracle_mod.traverse(rays, sc.boxes, sc.triangles))
    print(int(emitting.sum()), int(dark.sum()))
    assert emitting.sum() >= EMITTING_PIXELS and dark.sum() >= DARK_PIXELS
    layer = mo.Render(sc, es.seeds(es.W * es.H), 2).layers(S.LAYERS)[0]              # (3, W*H)
    assert (layer[:, emitting] > 0).any(axis=0).all()
    assert not layer[:, dark].any()
    assert (layer > 0).any(axis=0).sum() > 4 * emitting.sum()                        # and the layer is no all-or-nothing picture


def test_which_resolve_kernel_the_tables_select(resolve_form):
    """csrc/scene_layout.hpp: resolve_runs_slim -- T12 runs the slim kernel (debug bit 27: its parent), T40 the two-wave form with the
    material table in global memory."""
    for name in es.SCENES:
        n = len(es.scene(name).triangles)
        assert resolve_form.rf_runs_slim(n, 12, 0, 0, 0, 0) == 1 and resolve_form.rf_runs_slim(n, 12, 0, 0, 0, 1 << 27) == 0
        assert resolve_form.rf_runs_slim(n, 40, 0, 0, 0, 0) == 0


def test_scene_around_restates_create_scene():
    """es.scene_around with create_scene's own Camera gives create_scene's arrays, byte for byte."""
    import clive2_amd as c2
    from clive2_amd.camera import Camera
    from clive2_amd.load import triangles_for_box
    from clive2_amd.meshes import icosphere
    specs = [dict(mesh=icosphere(1, radius=1.5), material=5, offset=np.array([0.5, 0.0, -1.0]))]
    for builder in ("numpy", "native"):
        a = c2.create_scene(40, 23, es.CAM_CENTER, es.CAM_DIRECTION, file_specs=specs, materials=es.table(12), bvh_builder=builder)
        cam = Camera(center=es.CAM_CENTER, direction=es.CAM_DIRECTION, pixel_width=40, pixel_height=23, phys_width=40 / 23, phys_height=1)
        b = es.scene_around(cam, triangles_for_box(), es.table(12), builder, meshes=specs)
        for f in ("camera", "triangles", "boxes", "materials", "light_triangles", "light_counts", "light_surface_areas",
                  "light_triangle_indices", "camera_triangle_indices"):
            assert np.asarray(getattr(a, f)).tobytes() == np.asarray(getattr(b, f)).tobytes(), (builder, f)

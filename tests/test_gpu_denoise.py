"""The denoiser on the device (csrc/denoise.hpp): the feature pass against the render's own first hits, the filter against
its numpy statement (tests/denoise_reference.py), the gain in picture quality, and that neither touches the render."""
import numpy as np
import pytest

import denoise_reference as dr

pytestmark = pytest.mark.gpu


def _open_scene(w, h, mesh=True):
    """Floor, back wall and the emitter of the box only (plus a 1,280-triangle ball: not LDS-resident, so the 4-wide walk is
    available): the top and the sides of the frame see nothing."""
    import clive2_amd as c2
    from clive2_amd.load import get_materials, triangles_for_box
    from clive2_amd.meshes import icosphere
    keep = [t for t in triangles_for_box() if t.emitter or t.n[1] > 0.5 or t.n[2] > 0.5]
    specs = [dict(mesh=icosphere(3, radius=1.5), material=5, offset=np.array([0.5, 0.0, -1.0]))] if mesh else None
    return c2.create_scene(w, h, np.array([0, 1.5, 6]), np.array([0, 0, -1]), room=keep, materials=get_materials(),
                           file_specs=specs)


def _glass(w, h):
    import clive2_amd as c2
    from clive2_amd.load import get_materials
    from clive2_amd.meshes import icosphere
    mats = get_materials()
    mats["alpha"][5] = 0.1
    v, f = icosphere(2, radius=2.0, center=(0.0, 1.0, 0.0))
    return c2.create_scene(w, h, np.array([0, 1.5, 6]), np.array([0, 0, -1]), file_specs=[dict(mesh=(v, f), material=5)],
                           materials=mats)


def _cornell(w, h):
    import clive2_amd as c2
    return c2.create_scene_from_preset("empty", w, h)


def _shading_normals(scene, tri, u, v, d):
    """sn of shade_and_bounce (csrc/kernels.hpp) in float32, turned to face the ray."""
    T = scene.triangles[tri]
    f = np.float32
    n0, n1, n2, tn = (np.asarray(T[k][:, :3], f) for k in ("n0", "n1", "n2", "normal"))
    u, v = u[:, None].astype(f), v[:, None].astype(f)
    s = (n0 * ((f(1) - u) - v) + n1 * u) + n2 * v
    length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    s = s * (f(1) / length)[:, None]
    facing = (d[:, 0] * tn[:, 0] + d[:, 1] * tn[:, 1]) + d[:, 2] * tn[:, 2]
    return np.where((facing > 0)[:, None], -s, s)


@pytest.mark.parametrize("name,mode", [("cornell", 0), ("glass", 0), ("open", 0), ("open", 5)])
def test_features_are_the_first_hits_of_the_camera_rays(name, mode):
    from clive2_amd.renderer import Renderer, make_seeds, CAMERA
    W, H = 72, 40
    scene = {"cornell": _cornell, "glass": _glass, "open": _open_scene}[name](W, H)
    S = make_seeds(W * H, seed=77)
    r = Renderer(scene, seeds=S)
    r.set_traversal_mode(mode)
    if mode == 5:
        assert r.organisation()["wide_nodes"] > 0
    r.make_camera_rays()
    rays = r.export_rays(CAMERA)
    bi, bt, u, v = r.probe_traverse(rays)
    r.render_features(1, seeds=S)
    f = r.features()
    hit = bi >= 0
    if name == "open":
        assert hit.any() and (~hit).any()
    else:
        assert hit.all()
    depth, cov = f["depth"].reshape(-1), f["coverage"].reshape(-1)
    normal, albedo = f["normal"].reshape(-1, 3), f["albedo"].reshape(-1, 3)
    assert np.array_equal(cov, hit.astype(np.float32))
    assert depth[hit].tobytes() == bt[hit].tobytes()
    mat_colour = np.asarray(scene.materials["color"][:, :3], np.float32)
    assert albedo[hit].tobytes() == mat_colour[scene.triangles["material"][bi[hit]]].tobytes()
    d = np.asarray(rays["direction"][:, :3], np.float32)
    want = _shading_normals(scene, bi[hit], u[hit], v[hit], d[hit])
    np.testing.assert_allclose(normal[hit], want, rtol=0, atol=1e-6)
    assert not normal[~hit].any() and not depth[~hit].any() and not albedo[~hit].any()
    # more samples: the coverage counts the hits, the normals stay unit length
    r.render_features(4, seeds=S)
    f4 = r.features()
    c4 = f4["coverage"]
    assert set(np.unique(c4)) <= {0.0, 0.25, 0.5, 0.75, 1.0}
    n4 = f4["normal"][c4 > 0]
    np.testing.assert_allclose(np.linalg.norm(n4, axis=-1), 1.0, atol=1e-5)


SIGMAS = [dict(sigma_color=0.6, sigma_depth=0.1, sigma_albedo=0.1), dict(sigma_color=0.2, sigma_depth=0.02, sigma_albedo=0.3),
          dict(sigma_color=4.0, sigma_depth=1.0, sigma_albedo=0.05)]


@pytest.mark.parametrize("name", ["cornell", "open"])
def test_kernel_equals_the_specification(name):
    from clive2_amd.renderer import Renderer
    W, H = 70, 45                               # partial 16 x 16 tiles on both edges
    scene = {"cornell": _cornell, "open": _open_scene}[name](W, H)
    r = Renderer(scene)
    r.run_samples(3)
    r.render_features(2)
    f = r.features()
    c = r.radiance
    if name == "open":
        assert (f["coverage"] == 0).any()
    for sig in SIGMAS:
        for it in (1, 5):
            got = r.denoised_radiance(iterations=it, **sig)
            want = dr.denoise(c, f["normal"], f["depth"], f["albedo"], f["coverage"], iterations=it, **sig)
            np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6, err_msg=f"{sig} iterations {it}")
    assert r.denoised_radiance(iterations=0).tobytes() == c.tobytes()


def _rmse(x, ref):
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 1e-2)))


@pytest.mark.parametrize("name", ["cornell", "glass"])
def test_it_denoises(name):
    from clive2_amd.renderer import Renderer, make_seeds
    W, H = 256, 192
    scene = {"cornell": _cornell, "glass": _glass}[name](W, H)
    ref_r = Renderer(scene, seeds=make_seeds(W * H, seed=4321))
    ref_r.run_samples(1024)
    ref = ref_r.radiance
    ref_r.close()
    r = Renderer(scene)
    r.run_samples(4)
    r.render_features(4)
    raw, den = r.radiance, r.denoised_radiance()
    ratio = _rmse(den, ref) / _rmse(raw, ref)
    print(f"{name}: rMSE raw {_rmse(raw, ref):.4g} denoised {_rmse(den, ref):.4g} ratio {ratio:.3f}")
    assert ratio <= 0.5
    img = r.denoised_image
    assert img.dtype == np.uint8 and img.shape == (H, W, 3)


@pytest.mark.parametrize("name,mode", [("cornell", 0), ("open", 5)])
def test_render_state_is_untouched(name, mode):
    from clive2_amd.renderer import Renderer, make_seeds
    W, H = 64, 48
    scene = {"cornell": _cornell, "open": _open_scene}[name](W, H)
    S = make_seeds(W * H, seed=5)
    a, b = Renderer(scene, seeds=S), Renderer(scene, seeds=S)
    for x in (a, b):
        x.set_reproducible(True)
        x.set_traversal_mode(mode)
        if mode == 5:
            x.set_counting(2)
    a.run_samples(2)
    b.run_samples(1)
    b.render_features(4)
    b.denoised_radiance()
    b.run_samples(1)
    assert a.packed_accumulators().tobytes() == b.packed_accumulators().tobytes()
    assert a.get_random_buffer().tobytes() == b.get_random_buffer().tobytes()
    assert a.counters() == b.counters()
    assert a.walk_tallies() == b.walk_tallies()


def test_denoise_needs_current_features():
    from clive2_amd.renderer import Renderer, RendererError
    scene = _cornell(32, 24)
    r = Renderer(scene)
    r.run_samples(1)
    with pytest.raises(RendererError, match=r"\(-3\)"):
        r.denoised_radiance()
    with pytest.raises(RendererError, match=r"\(-3\)"):
        r.features()
    r.render_features(1)
    r.denoised_radiance()
    r.upload_scene(scene)
    with pytest.raises(RendererError, match=r"\(-3\)"):
        r.denoised_radiance()
    with pytest.raises(RendererError, match=r"\(-1\)"):
        r.render_features(0)
    with pytest.raises(RendererError, match=r"\(-1\)"):
        r._check(r._L.cl2_denoise(r._h, 1, -1.0, 0.1, 0.1, None, 0), "cl2_denoise")

"""The filter over the layers of one render (cl2_denoise_layers, cl2_keep_layer_picture, csrc/denoise_layers.hpp) on
the device.  THE ORACLE IS THE EXISTING FILTER ON THE DEVICE: a twin handle with the same features whose accumulator rows 0..2 are
lacc[l] runs cl2_denoise(iterations, sigma_color[l], ...), and layer l of cl2_denoise_layers must hold its bytes -- no tolerance; where
the oracle holds a NaN the result must hold a NaN (payload and sign are free).  Frames of 64 x 48 (Cornell box, glass scene) and
50 x 37 with two sample streams (partial 16 x 16 tiles on both edges), 3 passes; injected states of feature_states at 7 x 5 and
41 x 25; 0, 1, 2, 3 and 5 passes of the filter: both staged step forms, the global form, and steps that reach beyond the frame."""
import ctypes as C
import glob

import numpy as np
import pytest

import denoise_reference as dr
import error_states as es
import feature_states as fs
import layers_denoise_reference as ldr
from denoise_scenes import cornell as _cornell, glass as _glass
from clive2_amd import strategies as S

pytestmark = pytest.mark.gpu

F = np.float32
PASSES, SEED = 3, 20240928
ITERATIONS = (0, 1, 2, 3, 5)
SD, SA = 0.1, 0.1
TABLES = {
    "layers": dict(S.LAYERS),
    "lengths": dict([(f"k{k}", S.path_length(k, k)) for k in range(1, 8)] + [("k8+", S.path_length(8))]),
    "partial": {"direct": S.path_length(2, 2), "nothing": 0, "two": S.bit(3, 1) | S.bit(2, 3)},
}
CASES = {"cornell": (_cornell, 64, 48, 1), "glass": (_glass, 64, 48, 1), "odd": (_cornell, 50, 37, 2)}


def _sigmas(n):
    """a colour sigma of its own for every layer: 0.6, 1.02, 1.73, ... (narrow to wide)"""
    return [float(F(0.6 * 1.7 ** l)) for l in range(n)]


def _same(got, want, what=""):
    assert ldr.same_bytes_or_both_nan(got, want), what


def _rendered(case, table):
    """a handle that holds 3 passes under `table` and the features of its scene"""
    from clive2_amd.renderer import Renderer, stream_seeds
    make, W, H, K = CASES[case]
    r = Renderer(make(W, H), streams=K)
    r.set_seeds(stream_seeds(r.batch_size, K, seed=SEED))
    r.set_reproducible(True)
    r.set_layers(table)
    r.run_samples(PASSES)
    r.render_features(2)
    return r


def _twin(r):
    """a second handle of the same frame with r's features: the oracle's"""
    from clive2_amd.renderer import Renderer
    t = Renderer(_cornell(r.pixel_width, r.pixel_height))
    t.load_features(**r.features())
    return t


def _oracle(t, acc, lacc, l, iterations, sigma_color):
    """cl2_denoise on the twin after cl2_write_accumulators_packed with rows 0..2 replaced by lacc[l], the other rows unchanged"""
    a = np.array(acc, dtype=F, copy=True).reshape(8, -1)
    a[:3] = lacc[l]
    t.load_packed_accumulators(a)
    return t.denoised_radiance(iterations=iterations, sigma_color=sigma_color, sigma_depth=SD, sigma_albedo=SA)


def _check_against_the_existing_filter(r, t, iterations=ITERATIONS, label=""):
    names = list(r.layers())
    sig = _sigmas(len(names))
    acc, lacc = r.packed_accumulators().reshape(8, -1), r.layer_accumulators()
    for it in iterations:
        layers, total = r.denoised_layers(iterations=it, sigma_color=dict(zip(names, sig)), sigma_depth=SD, sigma_albedo=SA)
        assert list(layers) == names
        for l, name in enumerate(names):
            _same(layers[name], _oracle(t, acc, lacc, l, it, sig[l]), f"{label} layer {name} iterations {it}")
        # the sum: float32 adds of the device's own layer pictures, in layer order
        _same(total, ldr.layer_sum([layers[n] for n in names]), f"{label} sum, iterations {it}")
    return acc, lacc


# ---------------------------------------------------------------- real renders
@pytest.mark.parametrize("table", list(TABLES))
@pytest.mark.parametrize("case", list(CASES))
def test_layers_equal_the_existing_filter_on_renders(case, table):
    r = _rendered(case, TABLES[table])
    t = _twin(r)
    acc, lacc = _check_against_the_existing_filter(r, t, label=f"{case} {table}")
    assert np.any(lacc != 0)
    # iterations = 0 is layer_radiance() on the device
    layers, _ = r.denoised_layers(iterations=0)
    for name, pic in r.layer_radiance().items():
        assert layers[name].tobytes() == pic.tobytes(), name
    if table == "partial":
        assert not layers["nothing"].any()
    r.close(); t.close()


# ---------------------------------------------------------------- injected states
@pytest.fixture(scope="module")
def pool():
    return es.pool()


def _injected(W, H, pool, L, wild=True):
    """a handle whose features, accumulators and L layer accumulators are states of feature_states: layer l takes the colour rows of
    the state with seed l + 1 (every class, the wild ones included) over the shared weight row"""
    from clive2_amd.renderer import Renderer
    r = Renderer(_cornell(W, H))
    cls, n, z, a, cov = fs.features(W, H)
    _, acc = fs.colours(cls, pool, wild=wild)
    lacc = np.stack([fs.colours(cls, pool, seed=l + 1, wild=wild)[1][:3] for l in range(L)]).astype(F)
    r.set_layers({f"l{l}": S.bit(l % 7, 2 + l // 7) for l in range(L)})
    r.load_packed_accumulators(acc)
    r.load_layer_accumulators(lacc)
    r.load_features(n, z, a, cov)
    return r, acc, lacc, (n, z, a, cov)


@pytest.mark.parametrize("W,H", [(7, 5), (41, 25)])
@pytest.mark.parametrize("L", [1, 3, 8])
def test_layers_equal_the_existing_filter_on_injected_states(W, H, L, pool):
    """coverage 0 (blocks, single pixels, a checker), zero normals, depth 0 and the wild colours: a skipped tap that was weighted 0
    instead would turn a NaN or inf colour behind it into a NaN sum"""
    r, acc, lacc, g = _injected(W, H, pool, L)
    cls = fs.features(W, H)[0]
    for k in (fs.COV0_BLOCK, fs.COV0_SINGLE, fs.COV0_CHECKER, fs.ZERO_NORMAL, fs.DEPTH_ZERO):
        assert fs.has(cls, k).any(), fs.NAMES[k]
    t = _twin(r)
    _check_against_the_existing_filter(r, t, label=f"{W} x {H}, {L} layers")
    # pixels that must pass through hold their input, in every layer
    keep = fs.pass_through(g[0], g[1], g[3])
    c = ldr.layer_radiance(lacc, acc, W, H)
    layers, total = r.denoised_layers(iterations=3, sigma_color=2.0, sigma_depth=SD, sigma_albedo=SA)
    for l, name in enumerate(layers):
        assert layers[name][keep].tobytes() == c[l][keep].tobytes(), name
    if L == 1:
        _same(total, layers["l0"], "the sum of one layer is that layer")
        assert total.tobytes() == layers["l0"].tobytes()
    r.close(); t.close()


def test_against_the_numpy_restatement_on_calm_colours(pool):
    W, H, L = 41, 25, 3
    r, acc, lacc, g = _injected(W, H, pool, L, wild=False)
    sig = _sigmas(L)
    layers, total = r.denoised_layers(iterations=3, sigma_color=dict(zip(r.layers(), sig)), sigma_depth=SD, sigma_albedo=SA)
    want, want_sum = ldr.denoise_layers(lacc, acc, *g, 3, sig, SD, SA)
    for l, name in enumerate(layers):
        np.testing.assert_allclose(layers[name], want[l], rtol=1e-4, atol=1e-6, err_msg=name)
    np.testing.assert_allclose(total, want_sum, rtol=1e-4, atol=1e-6)
    r.close()


# ---------------------------------------------------------------- kept pictures
def test_kept_layer_pictures_and_their_tone_map():
    from clive2_amd.camera import tone_map
    from clive2_amd.renderer import RendererError
    r = _rendered("odd", TABLES["layers"])
    names = list(r.layers())
    params = dict(iterations=3, sigma_color=dict(zip(names, _sigmas(3))), sigma_depth=SD, sigma_albedo=SA)
    layers, total = r.denoised_layers(**params)
    assert r.kept_kind is None
    r.keep_layer_picture(None, **params)
    assert r.kept_kind == "layer_sum" and r._L.cl2_kept_picture(r._h) == 7
    _same(r.kept_picture(), total, "kept sum")
    Lw = np.exp(np.float64(r.picture_log_sum()) / (r.pixel_height * r.pixel_width))
    assert np.isfinite(Lw) and Lw > 0
    assert r.tone_mapped_picture(log_average=Lw).tobytes() == tone_map(total, exposure=4.0, Lw=Lw).tobytes()
    for name in names:
        r.keep_layer_picture(name, **params)                          # only this layer is filtered
        assert r.kept_kind == "layer" and r._L.cl2_kept_picture(r._h) == 6
        _same(r.kept_picture(), layers[name], name)
        assert r.tone_mapped_picture(log_average=Lw).tobytes() == tone_map(layers[name], exposure=4.0, Lw=Lw).tobytes(), name
    # iterations = 0 through the same path
    r.keep_layer_picture("direct", iterations=0)
    assert r.kept_picture().tobytes() == r.layer_radiance()["direct"].tobytes()
    # a refused call leaves the previous kept picture
    before = r.kept_picture().tobytes()
    sig = (C.c_float * 3)(2.0, 2.0, 2.0)
    for layer, it, s in ((3, 1, sig), (-2, 1, sig), (0, 13, sig), (0, 1, (C.c_float * 3)(2.0, -1.0, 2.0)), (0, 1, None)):
        assert r._L.cl2_keep_layer_picture(r._h, layer, it, s, SD, SA) == -1, (layer, it)
        assert r.kept_kind == "layer" and r.kept_picture().tobytes() == before
    with pytest.raises(ValueError):
        r.keep_layer_picture("no such layer")
    # cl2_keep_picture takes 0..4 only, and 0 drops a layer's picture like any other
    for kind in (5, 6, 7):
        assert r._L.cl2_keep_picture(r._h, kind, 3, 2.0, SD, SA) == -1
        assert r.kept_kind == "layer" and r.kept_picture().tobytes() == before
    r.keep_picture(None)
    assert r.kept_kind is None
    with pytest.raises(RendererError, match=r"\(-3\)"):
        r.kept_picture()
    r.close()


# ---------------------------------------------------------------- nothing else moves
def test_render_state_and_the_plain_filter_are_untouched():
    r = _rendered("cornell", TABLES["layers"])

    def state():
        return (r.packed_accumulators().tobytes(), r.layer_accumulators().tobytes(), r.get_random_buffer().tobytes(),
                {k: v.tobytes() for k, v in r.features().items()}, r.counters(), r.walk_tallies(), r.denoised_radiance().tobytes())
    before = state()
    r.denoised_layers(iterations=3, sigma_color=1.0)
    r.denoised_layers(iterations=0)
    r.keep_layer_picture("indirect", iterations=5)
    r.keep_layer_picture(None, iterations=2)
    after = state()
    assert before == after
    # and the layered call does not read what cl2_denoise left in its own buffers
    a, _ = r.denoised_layers(iterations=3, sigma_color=1.0)
    r.denoised_radiance(iterations=5, sigma_color=7.0)
    b, _ = r.denoised_layers(iterations=3, sigma_color=1.0)
    for name in a:
        _same(a[name], b[name], name)
    # samples after the calls continue the render a handle without them makes
    twin = _rendered("cornell", TABLES["layers"])
    r.run_samples(1); twin.run_samples(1)
    assert r.packed_accumulators().tobytes() == twin.packed_accumulators().tobytes()
    assert r.layer_accumulators().tobytes() == twin.layer_accumulators().tobytes()
    r.close(); twin.close()


# ---------------------------------------------------------------- state and refusals
def test_state_and_refusals():
    from clive2_amd.renderer import Renderer, RendererError, stream_seeds
    from clive2_amd._native import ptr
    W, H = 32, 24
    scene = _cornell(W, H)
    r = Renderer(scene)
    r.set_seeds(stream_seeds(r.batch_size, 1, seed=SEED))
    r.set_reproducible(True)
    FB = W * H
    lay, tot = np.empty(3 * 3 * FB, F), np.empty(3 * FB, F)
    sig = (C.c_float * 8)(*[2.0] * 8)

    def call(it=1, s=sig, sd=SD, sa=SA, out=lay, n=None, out_sum=tot, m=None):
        return r._L.cl2_denoise_layers(r._h, it, s, sd, sa, ptr(out), C.c_size_t(out.size if n is None and out is not None else n or 0),
                                       ptr(out_sum), C.c_size_t(out_sum.size if m is None and out_sum is not None else m or 0))
    # no table
    r.run_samples(1)
    r.render_features(1)
    assert call() == -3
    assert r._L.cl2_keep_layer_picture(r._h, -1, 1, sig, SD, SA) == -3
    with pytest.raises(RendererError, match=r"no layer table is set"):
        r.denoised_layers()
    # a table set on a handle with samples: lacc is invalid until the accumulators are reset
    r.set_layers(TABLES["layers"])
    assert call() == -3
    with pytest.raises(RendererError, match=r"do not cover every sample"):
        r.denoised_layers()
    with pytest.raises(RendererError, match=r"do not cover every sample"):
        r.keep_layer_picture(None)
    r.reset_accumulators()
    r.run_samples(1)
    assert call() == 0
    # no features after cl2_upload_scene
    r.upload_scene(scene)
    assert call() == -3
    with pytest.raises(RendererError, match=r"no features for the current scene"):
        r.denoised_layers()
    r.render_features(1)
    assert call() == 0
    # arguments
    assert call(s=None) == -1
    assert call(out=None, out_sum=None) == -1
    assert call(n=lay.size - 1) == -1 and call(n=3 * FB) == -1 and call(m=tot.size + 1) == -1
    assert call(out=None) == 0 and call(out_sum=None) == 0                         # either output alone
    bad = lambda l, v: (C.c_float * 3)(*[v if k == l else 2.0 for k in range(3)])
    for l in range(3):                                                             # cl2_denoise's checks for every layer's sigma
        for v in (-1.0, 0.0, float("nan"), float("inf"), 1e-23, 1e-19):
            assert call(s=bad(l, v)) == -1, (l, v)
        assert call(it=12, s=bad(l, 2e-16)) == -1
        assert call(it=11, s=bad(l, 2e-16)) == 0
        assert call(it=0, s=bad(l, 1e-23)) == 0                                    # no pass divides by den_c
        assert call(s=bad(l, 1.1e-19)) == 0
    for args in (dict(it=-1), dict(it=13), dict(sd=0.0), dict(sd=float("nan")), dict(sa=-1.0), dict(sa=1e-23), dict(sa=1e-19),
                 dict(it=0, sa=1e-23)):
        assert call(**args) == -1, args
    assert call(it=12, sd=1e-30) == 0
    for layer in (-2, 3, 8):
        assert r._L.cl2_keep_layer_picture(r._h, layer, 1, sig, SD, SA) == -1
    assert r.kept_kind is None
    with pytest.raises(ValueError):
        r.denoised_layers(sigma_color={"no such layer": 1.0})
    r.close()


def test_working_buffers_follow_the_table():
    """3 layers, 8, and 3 again on one handle: the working buffers are made for the table that is set"""
    r = _rendered("odd", TABLES["layers"])
    t = _twin(r)
    from clive2_amd.renderer import stream_seeds
    first = {k: v.tobytes() for k, v in r.denoised_layers(iterations=3)[0].items()}
    for table in ("lengths", "layers"):
        r.set_layers(TABLES[table])
        r.reset_accumulators()
        r.set_seeds(stream_seeds(r.batch_size, 2, seed=SEED))
        r.run_samples(PASSES)
        _check_against_the_existing_filter(r, t, iterations=(0, 3), label=table)
    assert {k: v.tobytes() for k, v in r.denoised_layers(iterations=3)[0].items()} == first
    r.set_layers(None)                                                             # switched off: buffers released, calls refused
    assert r._L.cl2_keep_layer_picture(r._h, -1, 1, (C.c_float * 1)(2.0), SD, SA) == -3
    r.close(); t.close()


# ---------------------------------------------------------------- the command line
def test_render_denoise_layers_writes_the_files(tmp_path):
    from clive2_amd import render
    from clive2_amd.renderer import Renderer, stream_seeds
    from clive2_amd.scene import create_scene_from_preset
    W, H = 64, 48
    prefix = str(tmp_path / "box")
    argv = ["--scene", "empty", "--width", str(W), "--height", str(H), "--samples", "2", "--reproducible"]
    assert render.main(argv + ["--layers", prefix, "--single-pass", "--denoise-layers"]) == 0
    for name in ("emission", "direct", "indirect", "denoised"):
        assert glob.glob(f"{prefix}_{name}.png*"), name                   # .png, or .png.npy without PIL
    got = np.load(prefix + "_layers.npz")
    assert sorted(got.files) == ["denoised", "direct", "emission", "indirect"]
    r = Renderer(create_scene_from_preset("empty", pixel_width=W, pixel_height=H))
    r.set_reproducible(True)
    r.set_seeds(stream_seeds(W * H, 1))
    r.set_layers(S.LAYERS)
    r.run_samples(2)
    r.render_features(4)
    layers, total = r.denoised_layers()
    for name in layers:
        assert got[name].tobytes() == layers[name].tobytes(), name
        assert np.any(got[name] != 0)
    assert got["denoised"].tobytes() == total.tobytes()
    r.close()

"""The robust picture without a GPU: the formula of csrc/robust.hpp on cases worked by hand (through its numpy restatement,
tests/robust_reference.py), the state generator of the GPU tests, the exports, the refusals of the binding and of both CLIs, and
the estimator itself on synthetic addends."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import robust_reference as rr
import robust_states as rs_

F = np.float32
NEW_CALLS = ("cl2_set_robust_buckets", "cl2_get_robust_buckets", "cl2_read_buckets_packed", "cl2_write_buckets_packed",
             "cl2_robust_picture")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pixel(buckets):
    """one pixel from [(b, g, r, w), ...] -> bkt (M, 4, 1)"""
    return np.array(buckets, F).reshape(len(buckets), 4, 1)


def _grey(keys_w):
    """buckets whose three colour sums are key * w: the key is then luma(key, key, key)"""
    return _pixel([(k * w, k * w, k * w, w) for k, w in keys_w])


# ---------------------------------------------------------------- the formula by hand
def test_boundary_half_zero_half_equal_gives_g_one_half_and_trims_two_of_eight():
    """m = 8: four keys 0 and four keys v.  S = 4v, N = (1 + 3 + 5 + 7) v = 16v, G = 16v / (8 * 4v) = 0.5 exactly (every
    intermediate is a small multiple of a 24-bit value, exact in float64); c = floor(0.5 * 8 / 2) = 2.  Kept: ranks 3 .. 6 = the last
    two zero buckets (by index) and the first two bright ones, so the pixel is (2 * 0 + 2 * g) / (4 * w) = g / (2 w)."""
    b = np.zeros((8, 4, 1), F)
    b[:, 3] = 2.0
    b[[1, 2, 5, 7], 1] = 2.0 * 0.25                              # green mean 0.25 in buckets 1, 2, 5, 7
    valid, rank, m, G, c = rr.gini_trim(b)
    assert m[0] == 8 and G[0] == 0.5 and c[0] == 2
    assert rank[:, 0].tolist() == [0, 4, 5, 1, 2, 6, 3, 7]      # zeros 0, 3, 4, 6 first, in bucket order
    pic, st = rr.robust_picture(b)
    assert pic[0].tolist() == [0.0, 0.125, 0.0] and st[0].tolist() == [0.5, 2.0]
    # either side: one bright sum a float32 ulp up raises G; one zero key at 2^-50 of the bright ones lowers it by float64 ulps
    up, dn = b.copy(), b.copy()
    up[7, 1] = np.nextafter(up[7, 1], F(np.inf))
    dn[0, 1] = 0.5 * 2.0 ** -50
    Gu, cu = rr.gini_trim(up)[3:]
    Gd, cd = rr.gini_trim(dn)[3:]
    assert Gu[0] > 0.5 and cu[0] == 2
    assert 0.5 - 1e-15 < Gd[0] < 0.5 and cd[0] == 1


def test_fewer_than_three_valid_buckets_are_never_trimmed():
    # m = 0: black.  m = 1: that bucket.  m = 2: keys 0 and 1, G = 0.5, c = min(floor(0.5), 0) = 0: the plain ratio
    empty = np.zeros((4, 4, 1), F)
    pic, st = rr.robust_picture(empty)
    assert pic[0].tolist() == [0, 0, 0] and st[0].tolist() == [0, 0]
    one = empty.copy(); one[2, :, 0] = (1.0, 2.0, 3.0, 2.0)
    pic, st = rr.robust_picture(one)
    assert pic[0].tolist() == [0.5, 1.0, 1.5] and st[0].tolist() == [0, 0]
    two = one.copy(); two[0, :, 0] = (0.0, 0.0, 0.0, 2.0)
    valid, rank, m, G, c = rr.gini_trim(two)
    assert m[0] == 2 and G[0] == 0.5 and c[0] == 0
    assert rr.robust_picture(two)[0][0].tolist() == [0.25, 0.5, 0.75]
    # weights that are not > 0 and finite do not count, whatever the colour holds
    bad = two.copy()
    bad[1, :, 0] = (np.nan, 5.0, 5.0, -1.0); bad[3, :, 0] = (np.inf, 5.0, 5.0, np.inf)
    assert rr.gini_trim(bad)[2][0] == 2
    assert rr.robust_picture(bad)[0].tobytes() == rr.robust_picture(two)[0].tobytes()


def test_ties_keep_bucket_order():
    """keys 1, 1, 1, 40, 1 (the weights differ, so which tied bucket is dropped shows in the sums).  Ranks: buckets 0, 1, 2, 4 in
    bucket order, then 3.  S = 44, N = -4 - 2 + 0 + 2 + 160 = 156, G = 156 / 220, c = floor(G 5 / 2) = 1: rank 1 = bucket 0 (the first
    of the ties) and rank 5 = bucket 3 are dropped."""
    b = _grey([(1.0, 1.0), (1.0, 2.0), (1.0, 4.0), (40.0, 1.0), (1.0, 8.0)])
    valid, rank, m, G, c = rr.gini_trim(b)
    assert rank[:, 0].tolist() == [0, 1, 2, 4, 3]
    S, N = 44.0, (-4 * 1.0) + (-2 * 1.0) + 0.0 + 2 * 1.0 + 4 * 40.0
    assert G[0] == N / (5 * S) and c[0] == 1
    pic = rr.robust_picture(b)[0]
    assert pic[0].tolist() == [1.0, 1.0, 1.0]                    # buckets 1, 2, 4: (2 + 4 + 8) / (2 + 4 + 8)
    # all equal: G = 0, nothing trimmed, the plain ratio
    e = _grey([(0.5, w) for w in (1.0, 2.0, 4.0, 8.0)])
    valid, rank, m, G, c = rr.gini_trim(e)
    assert rank[:, 0].tolist() == [0, 1, 2, 3] and G[0] == 0.0 and c[0] == 0


def test_a_nan_key_sorts_last_and_counts_as_infinite():
    b = _grey([(3.0, 1.0), (1.0, 1.0), (2.0, 1.0), (5.0, 1.0), (4.0, 1.0)])
    b[1, 0, 0] = np.nan                                          # bucket 1: NaN key
    valid, rank, m, G, c = rr.gini_trim(b)
    assert rank[:, 0].tolist() == [1, 4, 0, 3, 2]
    assert G[0] == 1.0 and c[0] == 2                             # S = +inf: G = 1, c = min(floor(2.5), 2)
    assert rr.robust_picture(b)[0][0].tolist() == [4.0, 4.0, 4.0]   # the median bucket
    # +inf and NaN keys tie at +inf: bucket order
    b[3, 1, 0] = np.inf
    assert rr.gini_trim(b)[1][:, 0].tolist() == [1, 3, 0, 4, 2]


def test_negative_keys_count_as_zero_in_the_gini_sums_but_rank_by_value():
    b = _grey([(-2.0, 1.0), (1.0, 1.0), (-1.0, 1.0), (3.0, 1.0)])
    valid, rank, m, G, c = rr.gini_trim(b)
    assert rank[:, 0].tolist() == [0, 2, 1, 3]
    assert G[0] == (1 * 1.0 + 3 * 3.0) / (4 * 4.0)               # v = 0, 0, 1, 3
    allneg = _grey([(-2.0, 1.0), (-1.0, 1.0), (-3.0, 1.0)])
    assert rr.gini_trim(allneg)[3][0] == 0.0                     # S = 0: G = 0


def test_the_hook_puts_addend_i_into_bucket_i_mod_m():
    n, M = 11, 4
    xs = [np.full((1, 3), 2.0 ** i, F) for i in range(n)]
    ws = [np.ones(1, F) for _ in range(n)]
    a7, bkt = rr.accumulate(xs, ws, M)
    assert a7[0] == n
    for k in range(M):
        assert bkt[k, 0, 0] == sum(2.0 ** i for i in range(k, n, M)) and bkt[k, 3, 0] == len(range(k, n, M))
    # continuing from a count: the next addend goes to bucket 11 % 4
    rr.add_bucket(bkt, a7, np.full((1, 3), 0.5, F), np.ones(1, F))
    assert bkt[3, 3, 0] == 3 and bkt[3, 0, 0] == 2.0 ** 3 + 2.0 ** 7 + 0.5


@pytest.mark.parametrize("M", [3, 8, 16])
def test_synthetic_states_hold_every_class_where_the_docstring_says(M):
    """The state generator of the GPU tests does what its classes are named for -- checked here so that a GPU test that passes
    has met them."""
    pl = rs_.pool(M)
    pcls, pa7, pbkt = pl
    assert pbkt.shape == (M, 4, rs_.POOL)
    valid, rank, m, G, c = rr.gini_trim(pbkt)
    assert set(np.unique(m[pcls == rs_.PARTIAL])) == {0, 1, 2, 3}
    assert (m[pcls == rs_.UNCOVERED] == 0).all()
    assert (m[pcls == rs_.ORDINARY] == M).all()
    z = pcls == rs_.ZERO
    assert (G[z] == 0).all() and (c[z] == 0).all() and (m[z] == M).all()
    f = pcls == rs_.FIREFLY
    # G <= (m - 1) / m, so G m / 2 < 1 at m = 3: three buckets never trim a finite firefly (the formula's own limit)
    assert (c[f] == 0).all() if M == 3 else (c[f] >= 1).all()
    key = rr.keys(pbkt)[1]
    t = pcls == rs_.TIES
    most = np.array([np.unique(key[:, p], return_counts=True)[1].max() for p in np.flatnonzero(t)])
    assert set(most) == set(range(2, M + 1))
    assert (key[:, pcls == rs_.NEGATIVE] < 0).any(0).all()
    assert np.isinf(key[:, pcls == rs_.NONFINITE]).any(0).all()
    b = pcls == rs_.BOUNDARY
    if M % 2 == 0:
        assert (G[b] == 0.5).sum() >= b.sum() // 3 and (G[b] > 0.5).any() and (G[b] < 0.5).any()
    if M == 8:
        assert set(c[b]) == {1, 2} and (c[b][G[b] == 0.5] == 2).all()
    cls, a7, bkt = rs_.state(pl, 41 * 25)
    assert (np.bincount(cls[:64], minlength=9) >= 7).all() and (cls[64:128] == rs_.ORDINARY).all()


# ---------------------------------------------------------------- exports
@pytest.fixture(scope="module")
def native_lib():
    from clive2_amd import _native
    _native.build()
    return _native.lib()


def test_library_exports_and_header_declares_the_robust_calls(native_lib):
    from clive2_amd import _native
    header = open(os.path.join(ROOT, "include", "clive2_amd.h")).read()
    for name in NEW_CALLS:
        assert name in _native.EXPORTS
        assert hasattr(native_lib, name)
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert native_lib.cl2_abi_version() == 6


def test_robust_calls_refuse_a_null_handle(native_lib):
    L = native_lib
    buf = np.zeros(64, F)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.cl2_set_robust_buckets(None, 8) == -1
    assert L.cl2_get_robust_buckets(None) == -1
    assert L.cl2_read_buckets_packed(None, p, 64) == -1
    assert L.cl2_write_buckets_packed(None, p, 64) == -1
    assert L.cl2_robust_picture(None, p, 48, None, 0) == -1


# ---------------------------------------------------------------- refusals of the binding
class _NoDevice:
    """stands in for the library: the size of the buckets is known, nothing else may be called"""
    def cl2_get_robust_buckets(self, h):
        return 8

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called although the argument should have been refused before")


def _bare_renderer():
    from clive2_amd.renderer import Renderer
    r = Renderer.__new__(Renderer)
    r._L, r._h, r.batch_size = _NoDevice(), None, 12
    return r


@pytest.mark.parametrize("M", [-1, 1, 2, 17, 100])
def test_binding_refuses_a_bucket_count_outside_0_and_3_to_16(M):
    with pytest.raises(ValueError, match="3..16"):
        _bare_renderer().set_robust_buckets(M)


@pytest.mark.parametrize("size", [0, 4 * 8 * 12 - 1, 4 * 8 * 12 + 1, 8 * 12])
def test_binding_refuses_buckets_of_the_wrong_size(size):
    with pytest.raises(ValueError, match="4\\*M\\*W\\*H"):
        _bare_renderer().load_buckets(np.zeros(size, F))


# ---------------------------------------------------------------- CLI
@pytest.mark.parametrize("argv", [["--robust", "--denoise"], ["--robust", "4", "--denoise", "--variance-guided"],
                                  ["--robust", "2"], ["--robust", "17"]])
@pytest.mark.parametrize("cli", ["render", "movie"])
def test_cli_refuses_robust_with_denoise(cli, argv, monkeypatch):
    import importlib
    mod = importlib.import_module("clive2_amd." + cli)

    def no_renderer(*a, **k):
        raise AssertionError("a renderer was made before the arguments were checked")
    monkeypatch.setattr(mod, "Renderer", no_renderer)
    monkeypatch.setattr(mod, "rank_info", no_renderer)
    with pytest.raises(SystemExit) as e:
        mod.main(argv + ["--width", "16", "--height", "16"])
    assert e.value.code == 2


# ---------------------------------------------------------------- the estimator, on the restatement alone
def _mse_ratio(draw, mean, n, P=20000, M=8, seed=7):
    rs = np.random.RandomState(seed)
    xs, ws = [], []
    for _ in range(n):
        v = draw(rs, P).astype(F)
        xs.append(np.repeat(v[:, None], 3, 1))
        ws.append(np.ones(P, F))
    _, bkt = rr.accumulate(xs, ws, M)
    robust = rr.robust_picture(bkt)[0].astype(np.float64)
    plain = rr.plain_picture(bkt)
    return np.mean((robust - mean) ** 2) / np.mean((plain - mean) ** 2)


def test_fireflies_are_trimmed_and_clean_pixels_are_left_alone():
    """20,000 pixels, M = 8.  64 addends gamma(0.5, 2) * 0.5 of which one in a thousand is replaced by 500: the mean squared error
    of the robust picture about the addends' mean (0.5 * 0.999 + 500 * 0.001) is at most 0.2 of the plain picture's (measured 0.078:
    the robust picture pays a bias of the fireflies' share of the mean for not carrying their variance).  256 addends gamma(0.5, 2)
    alone: at most 1.05 of the plain one (measured 1.000)."""
    def fire(rs, P):
        return np.where(rs.uniform(size=P) < 1e-3, 500.0, rs.gamma(0.5, 2.0, P) * 0.5)
    r1 = _mse_ratio(fire, 0.5 * 0.999 + 500.0 * 1e-3, 64)
    r2 = _mse_ratio(lambda rs, P: rs.gamma(0.5, 2.0, P), 1.0, 256)
    print(f"robust / plain MSE: fireflies {r1:.3f}, clean {r2:.3f}")
    assert r1 <= 0.2
    assert r2 <= 1.05

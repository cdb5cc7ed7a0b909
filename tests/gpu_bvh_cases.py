"""Inputs of the GPU BVH builder's tree tests (tests/test_gpu_bvh_trees.py, tests/test_gpu_bvh_reference_cpu.py): float64 boxes by
family, the leaf sizes each is flattened at, and what the restatement must report about the path the input takes (the guards).
No NaN and no infinite input: their behaviour is undefined in the builder."""
import functools

import numpy as np

import gpu_bvh_reference as ref

SIZES = (2, 3, 8, 9, 10, 16, 17, 18, 63, 64, 65, 255, 256, 257, 511, 513, 4097, 70001)
LBVH_SIZES = tuple(n for n in SIZES if n <= 4097)
MEMBERS = (1, 2, 3, 8)


def random_boxes(n):
    """boxes inside [-5, 5]^3, coordinates of both signs"""
    rng = np.random.RandomState(1000 + n)
    size = rng.rand(n, 3) * 0.5
    lo = -5.0 + rng.rand(n, 3) * (10.0 - size)
    return lo, lo + size


def grid(dup):
    """16^3 equal boxes on a lattice (every union area of two neighbours along an axis is the same number), each `dup` times"""
    g = np.arange(16, dtype=np.float64)
    lo = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    lo = np.repeat(lo, dup, axis=0)
    return lo, lo + 0.5


def lattice():
    """13 x 11 x 7 equal boxes: no power of two, so the Morton order has no symmetry that makes the tie-break rule moot (on the
    16^3 grid "the first candidate at the smallest area wins" happens to build the same tree as the stated pair rule)"""
    lo = np.stack(np.meshgrid(np.arange(13.0), np.arange(11.0), np.arange(7.0), indexing="ij"), axis=-1).reshape(-1, 3)
    return lo, lo + 0.5


def repeated():
    """300 distinct boxes, 7 copies each, the copies scattered over the index range"""
    rng = np.random.RandomState(7)
    lo = rng.rand(300, 3) * 4.0 - 2.0
    hi = lo + rng.rand(300, 3) * 0.3
    at = rng.permutation(np.tile(np.arange(300), 7))
    return lo[at], hi[at]


def coincident(n):
    lo = np.tile(np.array([[0.25, 0.5, 0.75]]), (n, 1))
    return lo, lo + 0.5


def plane():
    rng = np.random.RandomState(21)
    lo = rng.rand(1000, 3) * 6.0 - 3.0
    hi = lo + rng.rand(1000, 3) * 0.2
    lo[:, 2] = hi[:, 2] = 0.0
    return lo, hi


def line_axis():
    """centroids on a line along x: two axes without extent"""
    rng = np.random.RandomState(22)
    lo = np.zeros((600, 3)); lo[:, 0] = rng.rand(600) * 8.0 - 4.0; lo[:, 1] = 0.5; lo[:, 2] = -1.25
    return lo, lo + 0.125


def line_diagonal():
    """points on a diagonal line"""
    rng = np.random.RandomState(23)
    p = (rng.rand(600, 1) * 2.0 - 1.0) * np.array([[1.0, 2.0, 3.0]])
    return p, p.copy()


def one_flat_axis():
    """boxes of different widths in x, symmetric about x = 1: one distinct centroid on that axis (the halves are exact in float64)"""
    rng = np.random.RandomState(24)
    lo = rng.rand(700, 3) * 4.0 - 2.0
    hi = lo + rng.rand(700, 3) * 0.25
    s = rng.randint(1, 100, 700) / 1024.0
    lo[:, 0], hi[:, 0] = 1.0 - s, 1.0 + s
    return lo, hi


def points():
    rng = np.random.RandomState(25)
    p = rng.rand(777, 3) * 2.0 - 1.0
    return p, p.copy()


def huge_partial():
    """areas of near neighbours are finite, of far ones +inf: PLOC merges for some rounds, then no cluster finds a neighbour"""
    rng = np.random.RandomState(31)
    lo = rng.rand(2000, 3) * 1e20
    return lo, lo + rng.rand(2000, 3) * 1e18


def huge_all():
    """every union area overflows float32 (tests/test_gpu_bvh.py)"""
    rng = np.random.RandomState(11)
    lo = rng.rand(500, 3) * 1e25
    return lo, lo + rng.rand(500, 3) * 1e24


class Case:
    def __init__(self, family, name, make, members, method="ploc", guard=None):
        self.family, self.name, self.make, self.members, self.method, self.guard = family, name, make, tuple(members), method, guard

    def __repr__(self):
        return self.name

    @functools.lru_cache(maxsize=None)
    def boxes(self):
        lo, hi = self.make()
        lo, hi = np.ascontiguousarray(lo, np.float64), np.ascontiguousarray(hi, np.float64)
        lo.setflags(write=False); hi.setflags(write=False)
        return lo, hi

    @functools.lru_cache(maxsize=None)
    def prepared(self):
        """the restatement up to the flattening: computed once, shared by the CPU and the GPU tests"""
        return ref.Prepared(*self.boxes(), self.method)

    @functools.lru_cache(maxsize=None)
    def tree(self, max_members):
        boxes, perm = self.prepared().flatten(max_members)
        boxes.setflags(write=False); perm.setflags(write=False)
        return boxes, perm


def _ploc_done(rounds=None):
    def guard(p):
        assert p.path == "ploc" and p.clusters_left == 1 and (rounds is None or p.rounds == rounds), (p.path, p.rounds, p.clusters_left)
    return guard


def _radix(rounds, left):
    def guard(p):
        assert p.path == "radix" and p.rounds == rounds and p.clusters_left == left, (p.path, p.rounds, p.clusters_left)
    return guard


def _mid_build(p):
    assert p.path == "radix" and p.rounds >= 1 and p.merges[0] >= 1 and p.clusters_left > 1, (p.path, p.rounds, p.clusters_left)


def _size_members(n):
    return (MEMBERS if n <= 4097 else (8,)) + (n, n + 5)          # max_members >= n: a single leaf


def _size_guard(n):
    return _radix(0, n) if n <= 2 else _ploc_done()


CASES = (
    [Case("sizes", f"ploc-{n}", functools.partial(random_boxes, n), _size_members(n), guard=_size_guard(n)) for n in SIZES] +
    [Case("lbvh", f"lbvh-{n}", functools.partial(random_boxes, n), _size_members(n), "lbvh", _radix(0, n)) for n in LBVH_SIZES] +
    [Case("ties", "grid", functools.partial(grid, 1), MEMBERS, guard=_ploc_done()),
     Case("ties", "grid-doubled", functools.partial(grid, 2), MEMBERS, guard=_ploc_done()),
     Case("ties", "lattice", lattice, MEMBERS, guard=_ploc_done()),
     Case("ties", "grid-lbvh", functools.partial(grid, 2), (1, 8), "lbvh", _radix(0, 8192)),
     Case("equal-keys", "repeated", repeated, MEMBERS, guard=_ploc_done()),
     Case("equal-keys", "repeated-lbvh", repeated, MEMBERS, "lbvh", _radix(0, 2100)),
     Case("equal-keys", "coincident-40", functools.partial(coincident, 40), MEMBERS, guard=_ploc_done(39)),
     Case("equal-keys", "coincident-3000", functools.partial(coincident, 3000), MEMBERS, guard=_radix(400, 2600)),
     Case("degenerate", "plane", plane, MEMBERS, guard=_ploc_done()),
     Case("degenerate", "line-axis", line_axis, MEMBERS, guard=_ploc_done()),
     Case("degenerate", "line-diagonal", line_diagonal, MEMBERS, guard=_ploc_done()),
     Case("degenerate", "one-flat-axis", one_flat_axis, MEMBERS, guard=_ploc_done()),
     Case("degenerate", "points", points, MEMBERS, guard=_ploc_done()),
     Case("degenerate", "plane-lbvh", plane, (1, 8), "lbvh", _radix(0, 1000)),
     Case("degenerate", "line-axis-lbvh", line_axis, (1, 8), "lbvh", _radix(0, 600)),
     Case("fallback", "huge-partial", huge_partial, MEMBERS, guard=_mid_build),
     Case("fallback", "huge-all", huge_all, MEMBERS, guard=_radix(0, 500))])

def by_name(name):
    return next(c for c in CASES if c.name == name)

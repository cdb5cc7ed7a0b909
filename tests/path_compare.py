"""Comparing Path[] arrays of the device with the oracle's -- TEST INFRASTRUCTURE (tests/test_gpu_walk_cases.py, tools/fuzz_parity.py)."""
import numpy as np

_FLOAT_FIELDS = ("origin", "direction", "inv_direction", "color", "normal", "c_importance", "l_importance", "tot_importance")


def canonical_nans(paths):
    """A copy of a Path[] array with every NaN of its float fields in ONE bit pattern.  A NaN that both sides compute in the same
    place (a reverse pdf of 0 / 0 at a grazing vertex: 3 scenes in 9,000, round 6) is the same result; its sign and payload are the
    hardware's default for an invalid operation -- 0x7fc00000 on the GPU, 0xffc00000 ("real indefinite") on the x86 host of the oracle,
    whatever Metal's is on the reference's GPU -- and say nothing about the computation."""
    out = paths.copy()
    rays = out["rays"]
    for f in _FLOAT_FIELDS:
        a = rays[f]
        a[np.isnan(a)] = np.float32(np.nan)
    return out


def nan_vertices(paths):
    """(vertices with a NaN in a float field, vertices) over the vertices the paths have (index < length)."""
    rays = paths["rays"]
    live = np.arange(rays.shape[1])[None, :] < paths["length"][:, None]
    bad = np.zeros(rays.shape, bool)
    for f in _FLOAT_FIELDS:
        a = np.isnan(rays[f])
        bad |= a.reshape(a.shape[0], a.shape[1], -1).any(axis=2)
    return int((bad & live).sum()), int(live.sum())


def same_paths(got, want):
    """'bytes' where the arrays have the same bytes, 'nans' where they have after canonical_nans, else None."""
    if got.tobytes() == want.tobytes():
        return "bytes"
    if canonical_nans(got).tobytes() == canonical_nans(want).tobytes():
        return "nans"
    return None

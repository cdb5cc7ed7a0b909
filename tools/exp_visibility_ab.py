"""Seeded visibility walk of the t >= 2 connection rays (cl2_set_connection_query(1); csrc/bvh_wide.hpp VIS) against the closest-hit walk.

    python tools/exp_visibility_ab.py [scene=glass,blob,interior] [samples=1] [W=1920] [H=1080] [parity_W=W] [parity_H=H]
    python tools/exp_visibility_ab.py baseline <libclive2_amd.so> [scene=...] [W] [H]      # mode-0 timing of ANOTHER build (the parent's)

Per scene, on ONE box:
  (i)   verdict parity over the t >= 2 connection rays of `samples` samples of the pipeline (light vertex s-1 -> camera vertex t-1 of
        every pair, rebuilt on the host from the exact render's exported Path[], each with its target: the camera vertex's triangle):
        `closest hit == T` of cl2_probe_traverse (traversal mode 5, the exact walk) against `stored triangle == T` of
        cl2_probe_visibility.  Every differing ray is classified: one of {the target T, the exact closest hit, the reported blocker}
        must lie in front of its own leaf box's entry distance -- the one case in which the two queries may differ;
  (ii)  what a connection ray costs in either mode: wide-node visits, triangle records, own bytes (device tallies, cl2_set_counting(2));
  (iii) ms per sample with 8 sample streams (pipelined) and the serial stage breakdown, modes 0, 1, 0, 1 of this build.
`baseline` times mode 0 of another build of the library the same way (one library per process), to confirm that the default path
costs what it cost before.  Functions are imported by nothing else; tests/test_gpu_visibility.py has the assertions of the suite."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from exp_order_ab import leaf_entry_distance, pipeline_ray_chunks      # noqa: E402


def connection_ray_chunks(scene, samples=1, seed=0):
    """pipeline_ray_chunks' connection rays with their targets: yields (s, t, origins, directions, target triangles) per strategy
    pair.  The rays are rebuilt exactly as exp_order_ab.pipeline_ray_chunks rebuilds them (checked chunk by chunk against it: same
    seeds, same samples), plus the `triangle` field of camera vertex t-1."""
    from clive2_amd.renderer import Renderer, make_seeds, LIGHT, CAMERA
    W, H = scene.pixel_width, scene.pixel_height
    twin = (c for c in pipeline_ray_chunks(scene, samples, seed) if c[0] == "connection")
    r = Renderer(scene, seeds=make_seeds(W * H, seed=seed) if seed else make_seeds(W * H))
    try:
        for _ in range(samples):
            r.run_sample()
            p = r.export_paths(LIGHT)
            len_l, o_l = p["length"].astype(np.int32), np.ascontiguousarray(p["rays"]["origin"][:, :6, :3])
            p = r.export_paths(CAMERA)
            len_c, o_c = p["length"].astype(np.int32), np.ascontiguousarray(p["rays"]["origin"][:, :6, :3])
            tri_c = np.ascontiguousarray(p["rays"]["triangle"][:, :6]).astype(np.int32)
            del p
            for s in range(1, 7):
                for t in range(2, 7):
                    m = (len_l >= s) & (len_c >= t)
                    if not m.any():
                        continue
                    a, b = o_l[m, s - 1], o_c[m, t - 1]
                    v = (b - a).astype(np.float32)
                    n = np.sqrt((v * v).sum(axis=1, dtype=np.float32)).astype(np.float32)
                    ok = n > 0
                    o, d = a[ok], (v[ok] / n[ok, None]).astype(np.float32)
                    _, o2, d2 = next(twin)
                    assert o.tobytes() == o2.tobytes() and d.tobytes() == d2.tobytes(), (s, t)
                    yield (s, t, o, d, tri_c[m, t - 1][ok])
    finally:
        r.close()
        twin.close()


def compare_queries(scene, chunks, log=None):
    """(i): every chunk through the exact closest-hit walk and through the seeded walk; every differing verdict is explained."""
    from clive2_amd import struct_types as st
    from clive2_amd.renderer import Renderer
    r = Renderer(scene)
    out = {"rays": 0, "visible_exact": 0, "visible_seeded": 0, "differ": 0, "in_front_of_own_leaf": 0, "unseeded": 0, "examples": []}
    try:
        r.set_traversal_mode(5)
        for s, t, o, d, T in chunks:
            n = len(o)
            rays = np.zeros(n, dtype=st.Ray)
            rays["origin"][:, :3] = o
            rays["direction"][:, :3] = d
            with np.errstate(divide="ignore"):
                seeded = np.isfinite(np.float32(1.0) / d).all(axis=1) & (T >= 0)      # the others are closest-hit queries in either mode
            i0, t0, _, _ = r.probe_traverse(rays)
            i1, t1 = r.probe_visibility(rays, T)
            same_unseeded = (i0[~seeded] == i1[~seeded]).all() and t0[~seeded].tobytes() == t1[~seeded].tobytes()
            assert same_unseeded, "an unseeded ray is a closest-hit query"
            v0, v1 = i0 == T, i1 == T
            diff = np.flatnonzero(v0 != v1)
            out["rays"] += n; out["unseeded"] += int((~seeded).sum())
            out["visible_exact"] += int(v0.sum()); out["visible_seeded"] += int(v1.sum()); out["differ"] += len(diff)
            for j in diff:
                # T's distance: what the walk that saw T reports
                t_T = float(t1[j]) if v1[j] else (float(t0[j]) if v0[j] else None)
                cands = {"target": (int(T[j]), t_T), "closest_hit": (int(i0[j]), float(t0[j])), "blocker": (int(i1[j]), float(t1[j]))}
                front = {k: (tri >= 0 and tt is not None and tt < leaf_entry_distance(scene, tri, o[j], d[j])) for k, (tri, tt) in cands.items()}
                out["in_front_of_own_leaf"] += int(any(front.values()))
                if len(out["examples"]) < 16:
                    out["examples"].append({"s": s, "t": t, "target": int(T[j]), "exact": [int(i0[j]), float(t0[j])], "seeded": [int(i1[j]), float(t1[j])], "in_front": front})
            if log:
                log(f"  s={s} t={t} {n:9d} rays  visible {int(v0.sum())}  verdicts differ {len(diff)}")
    finally:
        r.close()
    return out


def walk_cost(scene, mode, K=8, passes=3, set_mode=True):
    """(ii) + (iii): device tallies of the walk that runs, ms per sample (pipelined, K sample streams), the serial stage breakdown."""
    from clive2_amd.renderer import Renderer, stream_seeds
    W, H = scene.pixel_width, scene.pixel_height
    r = Renderer(scene, seeds=stream_seeds(W * H, K), streams=K)
    try:
        if set_mode:
            r.set_connection_query(mode)
        active = r.connection_query_active() if set_mode else 0
        r.tune()
        r.set_counting(2); r.reset_counters(); r.run_samples(1)
        t = r.walk_tallies()
        r.set_counting(False)
        r.run_samples(1); r.synchronize()
        t0 = time.perf_counter(); r.run_samples(passes); r.synchronize(); dt = time.perf_counter() - t0
        r.reset_counters(); r.set_profiling(2); r.set_pipelining(0); r.run_samples(1)
        c = r.counters()
        stages = {k[3:]: round(c[k] / K, 3) for k in c if k.startswith("ms_") and c[k] > 0}

        def per_ray(x):
            n = max(x["rays"], 1)
            return {"wide_visits": round(x["wide_visits"] / n, 3), "tri_records": round(x["tri_records"] / n, 3),
                    "own_bytes": round((112.0 * x["wide_visits"] + 36.0 * x["tri_records"] + 32.0 * x["binary_records"] + 16.0 * x["stack_spills"]) / n + 48.0, 1)}
        rays = c["rays"] // K
        ms = dt / (passes * K) * 1e3
        return {"mode": mode, "active": active, "ms_per_sample": round(ms, 3), "grays_per_s": round(rays / ms / 1e6, 3),
                "serial_stage_ms_per_sample": stages, "connection": per_ray(t["connection"]), "subpath": per_ray(t["subpath"]),
                "rays_per_sample": rays, "connection_rays_per_sample": t["connection"]["rays"] // K, "paths_share": r.organisation()["paths_share"]}
    finally:
        r.close()


def main():
    import json
    argv = sys.argv[1:]
    baseline = None
    if argv and argv[0] == "baseline":
        import ctypes
        import types
        import clive2_amd._native as native
        baseline = native.LIB_PATH = os.path.abspath(argv[1])
        new = ("cl2_set_connection_query", "cl2_get_connection_query", "cl2_connection_query_active", "cl2_probe_visibility")

        class OlderLibrary(ctypes.CDLL):
            """a build from before the connection query lacks its four entry points: the binding may still describe them (this
            process never calls them); any other missing symbol stays an error"""
            def __getattr__(self, name):
                if name in new:
                    try:
                        return super().__getattr__(name)
                    except AttributeError:
                        return types.SimpleNamespace()
                return super().__getattr__(name)
        native.C.CDLL = OlderLibrary
        argv = argv[2:]
    import bench
    names = (argv[0] if len(argv) > 0 else "glass,blob,interior").split(",")
    if baseline:
        W, H = (int(argv[1]), int(argv[2])) if len(argv) > 2 else (1920, 1080)
        for name in names:
            scene, desc = bench.build_scene(name, W, H)
            print(f"== {desc} {W}x{H}  library {os.path.relpath(baseline)}", flush=True)
            for _ in range(2):
                print("cost:", json.dumps(walk_cost(scene, 0, set_mode=False)), flush=True)
            bench._SCENES.clear()
        return
    samples = int(argv[1]) if len(argv) > 1 else 1
    W = int(argv[2]) if len(argv) > 2 else 1920
    H = int(argv[3]) if len(argv) > 3 else 1080
    PW = int(argv[4]) if len(argv) > 4 else W
    PH = int(argv[5]) if len(argv) > 5 else H
    for name in names:
        scene, desc = bench.build_scene(name, PW, PH)
        print(f"== {desc}  verdict parity at {PW}x{PH}, {samples} sample(s)", flush=True)
        res = compare_queries(scene, connection_ray_chunks(scene, samples), log=lambda s: print(s, flush=True))
        print("verdict parity:", json.dumps(res), flush=True)
        if (PW, PH) != (W, H):
            bench._SCENES.clear()
            scene, desc = bench.build_scene(name, W, H)
        print(f"== {desc}  cost at {W}x{H}", flush=True)
        for mode in (0, 1, 0, 1):
            print("cost:", json.dumps(walk_cost(scene, mode)), flush=True)
        bench._SCENES.clear()


if __name__ == "__main__":
    main()

"""Same-box A/B of two builds of the library: python tools/exp_ab_libs.py <lib_a.so> <lib_b.so> [scene=empty] [pairs=3] [samples=192]
Each library runs in its own child process (one library per process), alternating, 1080p, ms per sample."""
import os, subprocess, sys

CHILD = r'''
import sys, time, os
sys.path.insert(0, os.getcwd())
import clive2_amd._native as n
n.LIB_PATH = sys.argv[1]
import clive2_amd as c2
from clive2_amd.renderer import Renderer, make_seeds
scene = c2.create_scene_from_preset(sys.argv[2], 1920, 1080)
r = Renderer(scene, seeds=make_seeds(1920 * 1080))
r.run_samples(32); r.synchronize()
n = int(sys.argv[3])
t = time.perf_counter(); r.run_samples(n); r.synchronize(); dt = time.perf_counter() - t
print("%s  ms/sample %.3f" % (os.path.relpath(sys.argv[1]), dt / n * 1e3), flush=True)
'''

if __name__ == "__main__":
    a, b = sys.argv[1], sys.argv[2]
    scene = sys.argv[3] if len(sys.argv) > 3 else "empty"
    pairs = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    samples = sys.argv[5] if len(sys.argv) > 5 else "192"
    for lib in (a, b) * pairs:
        subprocess.run([sys.executable, "-c", CHILD, os.path.abspath(lib), scene, samples], check=True)

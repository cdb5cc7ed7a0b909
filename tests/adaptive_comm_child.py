"""Child process of test_gpu_adaptive.test_density_calls_refused_with_a_communicator: a one-rank RCCL communicator on device 0,
then every density call must return CL2_E_STATE.  Prints `STEP <name>` lines; exits 0 when every refusal came."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def step(name):
    print("STEP", name, flush=True)


def refused(fn):
    from clive2_amd.renderer import RendererError
    try:
        fn()
    except RendererError as e:
        return "(-3)" in str(e)
    return False


def main():
    from clive2_amd.renderer import Renderer, make_seeds
    from clive2_amd.scene import create_scene_from_preset
    from clive2_amd.distributed import join_communicator
    scene = create_scene_from_preset("empty", pixel_width=32, pixel_height=24)
    r = Renderer(scene, seeds=make_seeds(32 * 24))
    r.set_error_tracking(True)
    r.run_samples(2)
    join_communicator(r, 0, 1)
    step("comm-up")
    assert refused(lambda: r.set_sample_density(np.ones(32 * 24))), "set_sample_density"
    assert refused(lambda: r.update_sample_density()), "update_sample_density"
    assert refused(lambda: r.render_until(0.01, 4, adaptive=True)), "render_until(adaptive=True)"
    step("refused")
    r.comm_destroy()
    r.close()
    step("closed")


if __name__ == "__main__":
    main()

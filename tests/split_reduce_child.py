"""Child process of test_gpu_error_split.test_reduce_leaves_the_split_rows_invalid (the pattern of tests/rccl_one_rank_child.py): a
one-rank RCCL communicator on device 0, split tracking on, cl2_reduce_accumulators.  The accumulators and the moments come through
the reduce as they are; the split rows are not reduced and are invalid afterwards (-3 from every call that needs them) until
reset_accumulators().  Prints `STEP <name>` lines so that the parent can tell where a hang happened."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def step(name):
    print("STEP", name, flush=True)


def main():
    from clive2_amd.renderer import Renderer, RendererError, make_seeds
    from clive2_amd.scene import create_scene_from_preset
    from clive2_amd.distributed import join_communicator
    scene = create_scene_from_preset("empty", pixel_width=41, pixel_height=25)
    r = Renderer(scene, seeds=make_seeds(41 * 25))
    r.set_split_tracking(True)
    r.run_samples(2)
    acc, mom, rows = r.packed_accumulators().copy(), r.moments().copy(), r.split_moments().copy()
    share = r.light_share()
    step("rendered")
    join_communicator(r, 0, 1)
    step("comm-up")
    r.reduce_accumulators()
    assert r.packed_accumulators().tobytes() == acc.tobytes() and r.moments().tobytes() == mom.tobytes()
    step("reduced")
    for call in (r.split_moments, r.light_share):
        try:
            call()
        except RendererError as e:
            assert "(-3)" in str(e), e
        else:
            raise AssertionError("the split rows are still valid after the reduce")
    assert r.split_tracking
    step("rows-invalid")
    r.load_split_moments(rows)                         # the caller brings them: valid again
    assert r.light_share() == share
    r.reset_accumulators()
    assert not r.split_moments().any()
    step("rows-valid-again")
    r.comm_destroy()
    r.close()
    step("closed")


if __name__ == "__main__":
    main()

"""Child process of test_reduce_on_one_rank_keeps_the_buckets: a one-rank RCCL communicator on device 0, robust buckets on, the
accumulators and the buckets reduced in place by cl2_reduce_accumulators.  Prints `STEP <name>` lines so that the parent can
tell where a hang happened.  Modelled on tests/rccl_one_rank_child.py."""
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
    scene = create_scene_from_preset("empty", pixel_width=64, pixel_height=48)
    r = Renderer(scene, seeds=make_seeds(64 * 48))
    r.set_robust_buckets(8)
    r.run_samples(11)
    acc, bkt, pic = r.packed_accumulators().copy(), r.buckets().copy(), r.robust_radiance().copy()
    assert bkt.any()
    step("rendered")
    join_communicator(r, 0, 1)
    step("comm-up")
    r.reduce_accumulators()
    assert r.packed_accumulators().tobytes() == acc.tobytes(), "sum over one rank changed the accumulators"
    assert r.buckets().tobytes() == bkt.tobytes(), "sum over one rank changed the buckets"
    step("reduced-same-bytes")
    assert r.robust_radiance().tobytes() == pic.tobytes()          # still valid
    step("picture-same-bytes")
    r.load_packed_accumulators(acc)                                # invalid buckets stay invalid through the sum
    r.reduce_accumulators()
    try:
        r.robust_radiance()
        raise AssertionError("the reduce made invalid buckets valid")
    except RendererError as e:
        assert "(-3)" in str(e), e
    assert r.buckets().tobytes() == bkt.tobytes()
    step("invalid-stays-invalid")
    r.comm_destroy()
    step("comm-down")
    r.close()
    step("closed")


if __name__ == "__main__":
    main()

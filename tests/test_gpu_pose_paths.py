"""coeb_pose_optimization on every directed problem of tests/pose_ref.py (MI355X only): each
k_pose template (the id's ept5 / ept9 / ept0 is what launch_pose picks for the problem's keypoint
count), the template boundaries, full and partly filled 32-lane runs and register slots, all
three largest-diagonal quaternion branches, points at and behind the camera, qmax == 10 rounds
and long rejection runs.  Every result is compared twice: bit for bit with the oracle, and,
independently, with the float64 model under the bound measured on the CPU."""
import numpy as np
import pytest

import pose_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(R.PROBLEMS), ids=R.problem_id)
def test_pose_paths(ctx, oracle_mod, name):
    P, model = R.problem(name)
    assert np.array_equal(ctx.tables().inv_sigma2[:8], R.inv_sigma2())
    res = R.run_kernel(ctx, P)
    R.pose_both(ctx, oracle_mod, P, result=res)
    d = R.compare_with_model(P, *res, model)
    print("%s: nin %d max|T_gpu - T_model| %.3g" % (R.problem_id(name), res[0], d))


def test_pose_scratch_regrowth_ept0(oracle_mod):
    """k_pose<0> keeps its edges and active flags in the context's global scratch.  On a fresh
    context: 600 keypoints (small scratch), 2600 (the scratch regrows), 600 again, 2600 again;
    both 2600 runs must give the oracle's bits, whatever the runs between left behind."""
    from coeb_front import Context
    big, small = R.problem("n2600")[0], R.problem("base-seed0")[0]
    assert R.ept_of(len(big["kps"])) == 0 and R.ept_of(len(small["kps"])) == 5
    c = Context(max_width=640, max_height=480, max_batch=1)
    try:
        R.pose_both(c, oracle_mod, small)
        first = R.run_kernel(c, big)
        R.pose_both(c, oracle_mod, small)
        second = R.run_kernel(c, big)
        R.pose_both(c, oracle_mod, big, result=second)
    finally:
        c.close()
    assert first[0] == second[0] and np.array_equal(first[1].view(np.uint32), second[1].view(np.uint32))
    assert np.array_equal(first[2], second[2])

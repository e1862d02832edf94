"""Non-finite rows through gmr_motion_self_collision_repair: a NaN, an infinity or a zero root quaternion in one row changes that
frame's outputs and its own clip's statistics, and no other byte (the values are those of tests/nonfinite_cases.py)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import nonfinite_cases as nf  # noqa: E402
from tests import self_collision_repair_inputs as ri  # noqa: E402
from tests import self_collision_repair_reference as RR  # noqa: E402
from tests.test_gpu_self_collision_repair import FRAME, STATS, busy_rows, run, same  # noqa: E402

ROBOT = "unitree_g1"
OFFS = np.array([0, 12, 26, 40], np.int64)
ROW = 20          # a colliding frame of the middle clip (rows 16 .. 39 of busy_rows collide)


def _clean():
    from tests import self_collision_inputs as ci
    caps, pairs = ci.tables(ROBOT)
    q = np.array(busy_rows()[0])
    return q, caps, pairs, run(ROBOT, q, OFFS, caps, pairs)


@pytest.mark.parametrize("value", nf.VALUES)
def test_a_non_finite_entry_reaches_its_own_frame_and_its_own_clip_only(value):
    q0, caps, pairs, clean = _clean()
    nq = q0.shape[1]
    assert clean["move"][ROW] > 0.0 and clean["repaired_frames"].tolist() == [0, 10, 14]
    for col in (0, 2, 3, 6, 7, 7 + 12, nq - 1):
        q1 = q0.copy()
        q1[ROW, col] = nf.value64(value)
        got = run(ROBOT, q1, OFFS, caps, pairs)
        check_one(got, clean, q1, (value, col))


def test_a_zero_root_quaternion_gives_a_nan_frame_that_is_copied():
    q0, caps, pairs, clean = _clean()
    q1 = q0.copy()
    q1[ROW, 3:7] = 0.0
    check_one(run(ROBOT, q1, OFFS, caps, pairs), clean, q1, "zero quaternion")


def check_one(got, clean, q1, what):
    assert same(got["qpos"][ROW], q1[ROW]), what                                        # copied bit for bit, the payload of a NaN included
    assert np.isnan(got["clearance_before"][ROW]) and np.isnan(got["clearance_after"][ROW]) and got["move"][ROW] == 0.0, what
    keep = np.arange(q1.shape[0]) != ROW
    for k in FRAME:
        assert same(got[k][keep], clean[k][keep]), (what, k)                            # no other frame changes
    for k in STATS:
        assert same(got[k][[0, 2]], clean[k][[0, 2]]), (what, k)                        # no byte of another clip changes
    own = RR.statistics(got["clearance_after"], got["move"], OFFS, 0.0, RR.RESOLVE_TOL)
    for k in STATS:
        assert same(got[k], own[k]), (what, k)
    assert got["nonfinite_frames"].tolist() == [0, 1, 0] and got["repaired_frames"].tolist() == [0, clean["repaired_frames"][1] - 1, 14], what


def test_the_reference_treats_such_rows_alike():
    from tests import self_collision_inputs as ci
    q0, caps, pairs, clean = _clean()
    q1 = q0.copy()
    q1[ROW, 9] = np.nan
    q1[ROW + 2, 3:7] = 0.0
    ref = RR.repair(ci.robot_model(ROBOT), caps, pairs, q1, OFFS)
    got = run(ROBOT, q1, OFFS, caps, pairs)
    assert same(ref["qpos"][[ROW, ROW + 2]], q1[[ROW, ROW + 2]]) and same(got["qpos"][[ROW, ROW + 2]], q1[[ROW, ROW + 2]])
    for k in ("clearance_before", "clearance_after"):
        assert np.array_equal(np.isnan(ref[k]), np.isnan(got[k])) and np.isnan(ref[k]).sum() == 2
    for k in ("repaired_frames", "unresolved_frames", "nonfinite_frames"):
        assert np.array_equal(ref[k], got[k]), k
    assert ri.N == 332

"""Host side of the per-joint velocity limit (``use_velocity_limit`` / ``gmr_model_set_step_cap``): no GPU, no native library.

1. The reference the GPU tests compare with (tests/step_cap_reference.py) is the oracle's own frame loop when the cap is +inf.
2. How the constructor arguments resolve to the per-solve cap table.
"""
import inspect

import numpy as np
import pytest

from gmr_amd import synth
from gmr_amd.model import DEFAULT_VELOCITY_LIMIT, compile_model, resolve_velocity_limits, step_cap
from gmr_amd.schedule import make_items
from oracle.oracle import IKParams, Oracle
from tests.step_cap_reference import retarget_clips
from tests.util import compiled


@pytest.mark.parametrize("robot", ["unitree_g1", "booster_t1", "galaxea_r1pro"])
@pytest.mark.parametrize("dtype,otg", [(np.float32, 0), (np.float64, 1)])
def test_helper_without_cap_is_the_oracle(robot, dtype, otg):
    """Cap all +inf: the Python frame loop equals Oracle.ik_solve / retarget_frame on the same frames, values and solve counts.
    Observed maximum difference on these inputs: 0.0 exactly (the helper calls the very functions the oracle's loop calls, in its
    order); the assert leaves room for one rounding."""
    cm = compiled("smplx", robot)
    orc = Oracle(cm.blob)
    pos, quat, names, offs, _ = synth.synth_clips(cm, 3, 6, seed=32, hard=True, dtype=dtype)
    sc = cm.slot_columns(names)
    prm = IKParams(offset_to_ground=otg)
    got = retarget_clips(cm, pos, quat, sc, offs, cap=None, params=prm, orc=orc)
    q_ref, it_ref, _ = orc.ik_solve(pos, quat, sc, make_items(offs), params=prm)
    print(f"{robot}: max |helper - oracle| = {np.abs(got.qpos - q_ref).max():.3e}")
    assert np.abs(got.qpos - q_ref).max() <= 1e-12
    assert np.array_equal(got.solves, it_ref)
    assert got.cap_active_solves() == 0
    # ... and frame by frame through retarget_frame, clip 0
    q = np.array(cm.robot.qpos0)
    for f in range(int(offs[1])):
        q, s, _ = orc.retarget_frame(q, pos[f][sc].astype(np.float64), quat[f][sc].astype(np.float64), prm)
        assert np.abs(q - got.qpos[f]).max() <= 1e-12 and s == got.solves[f]


def _hinges(robot):
    return [robot.jnt_names[b] for b in robot.hinge_bodies()]


@pytest.mark.parametrize("name", ["unitree_g1", "galaxea_r1pro"])
def test_default_table_is_the_limited_hinges(name):
    robot = compiled("smplx", name).robot
    assert resolve_velocity_limits(robot) is None and resolve_velocity_limits(robot, False, None) is None
    table = resolve_velocity_limits(robot, True)
    limited = [robot.jnt_names[b] for b in robot.hinge_bodies() if robot.jnt_limited[b]]
    assert list(table) == limited and len(limited) > 0
    assert all(v == DEFAULT_VELOCITY_LIMIT == 3 * np.pi for v in table.values())
    cap = step_cap(robot, table)
    assert cap.shape == (robot.nv,) and np.isinf(cap[:6]).all()  # never the root: free joint, planar base and its null dofs alike
    for b in robot.hinge_bodies():
        expect = robot.timestep * 3 * np.pi if robot.jnt_limited[b] else np.inf
        assert cap[robot.dof_adr[b]] == expect
    assert step_cap(robot, None) is None


def test_r1pro_has_unlimited_hinges_the_default_leaves_alone():
    robot = compiled("smplx", "galaxea_r1pro").robot
    free = [robot.jnt_names[b] for b in robot.hinge_bodies() if not robot.jnt_limited[b]]
    assert free, "the wheels are unlimited hinges"
    table = resolve_velocity_limits(robot, True)
    assert not set(free) & set(table)
    assert set(resolve_velocity_limits(robot, False, 2.0)) == set(_hinges(robot))  # one number: every hinge


def test_overrides():
    robot = compiled("smplx", "unitree_g1").robot
    h = _hinges(robot)
    # one number for all hinges; implies the switch
    t = resolve_velocity_limits(robot, False, 7.5)
    assert t == {n: 7.5 for n in h}
    assert np.array_equal(step_cap(robot, t)[6:], np.full(len(h), robot.timestep * 7.5))
    # a dict alone: the joints it names and nothing else
    t = resolve_velocity_limits(robot, False, {h[0]: 1.0, h[3]: np.inf})
    assert t == {h[0]: 1.0, h[3]: np.inf}
    cap = step_cap(robot, t)
    assert cap[6] == robot.timestep * 1.0 and np.isinf(np.delete(cap, 6)).all()
    # a dict on top of the switch: the default table with those entries replaced
    t = resolve_velocity_limits(robot, True, {h[0]: 1.0})
    assert t[h[0]] == 1.0 and all(t[n] == DEFAULT_VELOCITY_LIMIT for n in h[1:] if n in t) and len(t) == len(resolve_velocity_limits(robot, True))
    with pytest.raises(KeyError):
        resolve_velocity_limits(robot, True, {"no_such_joint": 1.0})
    with pytest.raises(KeyError):
        resolve_velocity_limits(robot, False, {robot.body_names[0]: 1.0})  # a body, not a hinge
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            resolve_velocity_limits(robot, False, bad)
        with pytest.raises(ValueError):
            resolve_velocity_limits(robot, True, {h[1]: bad})


def test_the_cap_travels_with_the_compiled_model_not_in_the_blob():
    base = compiled("smplx", "unitree_g1")
    table = resolve_velocity_limits(base.robot, True)
    cm = compile_model(base.robot, base.config, None, velocity_limits=table)
    assert cm.blob == base.blob and base.step_cap is None and base.velocity_limits is None
    assert cm.velocity_limits == table and np.array_equal(cm.step_cap, step_cap(base.robot, table))


def test_constructors_take_the_two_arguments():
    from gmr_amd import GeneralMotionRetargeting
    from gmr_amd.multi_robot import MultiRobotRetargeting
    for cls in (GeneralMotionRetargeting, MultiRobotRetargeting):
        p = inspect.signature(cls.__init__).parameters
        assert p["use_velocity_limit"].default is False and p["velocity_limits"].default is None, cls


def test_broadcast_step_cap_single_process():
    from gmr_amd import distributed as gdist
    cap = np.array([np.inf] * 6 + [0.01, 0.02])
    assert gdist.broadcast_step_cap(None) is None
    assert np.array_equal(gdist.broadcast_step_cap(cap), cap)

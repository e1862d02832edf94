"""The inputs of the self-collision repair tests and their reference answers, each computed once
(tests/self_collision_repair_reference.py).

The rows are those of tests/self_collision_inputs.py: the 332-row `explicit` clips of 0, 1, 2, 3, 4, 63, 64, 65 and 130 frames, and
`reach_pose()`.  The cases are the five of the issue (six with both margins of booster_k1), at the call's defaults (16 passes,
damping 1e-6 m^2, step cap 0.2 rad, resolve_tol 1e-4 m: conventions, not measured on a robot).

`unitree_g1_with_hands` and the thin synthetic chains of tests/synthetic_trees.py are NOT agreement cases: their random finger and
chain poses cross segment axes (nw of an active pair down to 5.7e-6 m, where the normal w / nw amplifies every rounding and the
contract has no normal at nw = 0), and 28 of the 167 colliding frames of the hands model stay unresolved.  The algorithm is not
tuned for them."""
import functools

import numpy as np

from gmr_amd import collision
from tests import self_collision_inputs as ci
from tests import self_collision_repair_reference as RR

LENS, OFFS, N, S = ci.LENS, ci.OFFS, ci.N, ci.S
ALL = (1 << 64) - 1
# case: (robot, margin, rest_margin of default_pairs, frozen joint-name fragments, rows)
CASES = {"g1": ("unitree_g1", 0.0, 0.0, (), "explicit"), "g1_margin": ("unitree_g1", 0.005, 0.005, (), "explicit"),
         "g1_frozen": ("unitree_g1", 0.005, 0.005, ("hip", "knee", "ankle"), "explicit"),
         "k1": ("booster_k1", 0.0, 0.0, (), "explicit"), "k1_margin": ("booster_k1", 0.005, 0.005, (), "explicit"),
         "reach": ("unitree_g1", 0.0, 0.0, (), "reach")}
NW_MIN = 1e-4     # m: every active pair of every pass of the reference keeps its segments at least this far apart


def robot_of(case):
    return CASES[case][0]


def margin(case):
    return CASES[case][1]


@functools.lru_cache(maxsize=None)
def tables(case):
    """(CapsuleTable, PairTable): the skeleton's proxies at the robot's radius and `default_pairs(rest_margin=margin)`."""
    robot, _, rest, _, _ = CASES[case]
    if rest == 0.0:
        return ci.tables(robot)
    caps = ci.tables(robot)[0]
    return caps, collision.default_pairs(ci.robot_model(robot), caps, rest_margin=rest)[0]


@functools.lru_cache(maxsize=None)
def hinge_mask(case):
    robot, frozen = CASES[case][0], CASES[case][3]
    rob = ci.robot_model(robot)
    names = [rob.jnt_names[b] for b in rob.hinge_bodies() if any(f in rob.jnt_names[b] for f in frozen)]
    return collision.movable_mask(rob, freeze_joints=names)


@functools.lru_cache(maxsize=None)
def rows(case):
    """(qpos [N, nq], seq_offsets)."""
    if CASES[case][4] == "reach":
        q = ci.reach_pose()
        q.setflags(write=False)
        return q, np.array([0, q.shape[0]], np.int64)
    return ci.qpos(CASES[case][0]), OFFS


@functools.lru_cache(maxsize=None)
def reference(case, iterations=RR.ITERATIONS, dtype=np.float64):
    """The numpy reference's answer to the case, every output by name."""
    caps, pairs = tables(case)
    q, offs = rows(case)
    ref = RR.repair(ci.robot_model(robot_of(case)), caps, pairs, q, offs, margin(case), iterations=iterations,
                    hinge_mask=hinge_mask(case), dtype=dtype)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def measure_floor(case):
    """{"qpos", "clearance"}: worst |float64 - longdouble| of the reference over every row of the case."""
    a, b = reference(case), reference(case, dtype=np.longdouble)
    return {"qpos": float(np.abs(a["qpos"] - b["qpos"]).max()),
            "clearance": float(max(np.abs(a[k] - b[k]).max() for k in ("clearance_before", "clearance_after")))}

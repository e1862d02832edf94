"""The inputs of the self-collision GPU tests and their reference answers, each computed once (tests/self_collision_reference.py).

The trajectories are tests/dynamics_inputs.explicit: clips of 0, 1, 2, 3, 4, 63, 64, 65 and 130 frames (332 rows) -- the empty clip,
the short ones and the 64-frame edges of the per-clip kernel's tiles.  The proxies are the skeleton's (gmr_amd.collision) at a
radius per robot chosen so that colliding and free frames both occur (asserted below).  ROBOTS is the registry list; a name
``tree/<shape>/<nbody>`` (tests/synthetic_trees.py) is accepted by every function here as well."""
import functools

import numpy as np

from gmr_amd import collision
from tests import dynamics_inputs as di
from tests import dynamics_reference as R
from tests import self_collision_reference as SR
from tests import synthetic_trees as ST

LENS, OFFS, N, S, FPS = di.LENS, di.OFFS, di.N, di.S, di.FPS
RADIUS = {"unitree_g1": 0.03, "booster_k1": 0.05, "unitree_g1_with_hands": 0.01}
ROBOTS = list(RADIUS)
MARGIN = 0.0


def case_radius(robot):
    """The capsule radius of a model's case: RADIUS for a registry robot, tests/synthetic_trees.radius for a synthetic tree."""
    return ST.radius(robot) if ST.is_tree(robot) else RADIUS[robot]


def robot_model(robot):
    return R.model(robot)[0]


@functools.lru_cache(maxsize=None)
def tables(robot, radius=None):
    """(CapsuleTable, PairTable): the skeleton's proxies at the case's radius and their default pairs."""
    rob = robot_model(robot)
    caps = collision.skeleton_capsules(rob, case_radius(robot) if radius is None else radius)
    return caps, collision.default_pairs(rob, caps)[0]


def qpos(robot):
    return di.explicit(robot)[0]


@functools.lru_cache(maxsize=None)
def reference(robot):
    """The numpy reference's answer to the robot's case, every output by name plus `pair_clearance` [N, P]."""
    caps, pairs = tables(robot)
    ref = SR.self_collision(robot_model(robot), caps, pairs, qpos(robot), OFFS, MARGIN)
    hit = ref["hits"] > 0
    both = hit.any() and not hit.all()
    # (a synthetic star never collides and a tree of fewer than 9 bodies has too few pairs: synthetic_trees.collides drops it there)
    assert both or (ST.is_tree(robot) and not ST.collides(robot)), f"{robot}: the case needs colliding and free frames, got {int(hit.sum())} of {N}"
    assert not np.isnan(ref["clearance"]).any()
    for v in ref.values():
        v.setflags(write=False)
    return ref


def margin_distance(robot):
    """The smallest |pair clearance - margin| over every pair and frame of the reference: equal hit counts can only be asked for
    when it is far above the bound."""
    return float(np.abs(reference(robot)["pair_clearance"] - MARGIN).min())


def second_gap(cl):
    """Per frame the gap between the smallest and the second-smallest pair clearance [N]."""
    part = np.partition(cl, 1, axis=1)
    return part[:, 1] - part[:, 0]


def floor_rows(robot, per_kind=6):
    """The rows at which the numpy reference is measured against 50 digits: every clip's first row and, per kind, the `per_kind` rows
    with the smallest |clearance - margin|, the smallest clearance, and the smallest gap between the best and the second-best pair."""
    ref = reference(robot)
    keys = [np.abs(ref["clearance"] - MARGIN), ref["clearance"]]
    if ref["pair_clearance"].shape[1] > 1:                 # (a table of one pair has no second-best)
        keys.append(second_gap(ref["pair_clearance"]))
    rows = set(int(OFFS[s]) for s, T in enumerate(LENS) if T)
    for key in keys:
        rows.update(int(i) for i in np.argsort(key)[:per_kind])
    return sorted(rows)


def measure_floor(robot, rows=None):
    """Worst |numpy reference - 50-digit evaluator| of a pair clearance over all pairs of `rows` (None: floor_rows)."""
    rob = robot_model(robot)
    caps, pairs = tables(robot)
    cl = reference(robot)["pair_clearance"]
    worst, trajs = 0.0, {}
    for row in (floor_rows(robot) if rows is None else rows):
        s = int(np.searchsorted(OFFS, row, side="right")) - 1
        tr = trajs.setdefault(s, R.Trajectory(rob, s))
        want = SR.mp_pair_clearance(tr, caps, pairs, R.mpf(row - int(OFFS[s])) / R.mpf(FPS))
        worst = max(worst, float(np.abs(cl[row] - want).max()))
    return worst


def measure_origin_floor(robot, rows=None):
    """Worst |numpy FK - 50-digit evaluator| of a body origin over `rows` (None: all of them).  The floor of a model without a
    capsule pair (a tree of two bodies), whose points the transition search's test still compares."""
    rob = robot_model(robot)
    zero = np.zeros((rob.nbody, 3))
    caps = collision.CapsuleTable(np.arange(rob.nbody, dtype=np.int32), zero, zero, np.zeros(rob.nbody), list(rob.body_names))
    X = R.fk(rob, np.asarray(qpos(robot)))[0]
    worst, trajs = 0.0, {}
    for row in (range(N) if rows is None else rows):
        s = int(np.searchsorted(OFFS, row, side="right")) - 1
        tr = trajs.setdefault(s, R.Trajectory(rob, s))
        want = SR.mp_ends(tr, caps, R.mpf(row - int(OFFS[s])) / R.mpf(FPS))[0]
        worst = max(worst, float(np.abs(X[row] - np.array([[float(c) for c in p] for p in want])).max()))
    return worst


def reach_pose(frames=9, hit_frame=5):
    """A hand-built G1 clip: standing, and from frame 2 on the right arm swings up and the elbow folds so that in `hit_frame` the
    right hand is at the head.  Returns qpos [frames, nq].  (shoulder pitch, elbow) are scaled linearly; the pose of the hit frame
    was found by a coarse search of the numpy reference for the smallest hand-head clearance.)"""
    rob = robot_model("unitree_g1")
    q = di.standing("unitree_g1", frames).copy()
    col = {rob.jnt_names[b]: int(rob.qpos_adr[b]) for b in range(rob.nbody) if rob.jnt_type[b] == R.JNT_HINGE}
    target = reach_target()
    for k in range(frames):
        w = 1.0 - abs(k - hit_frame) / float(hit_frame)
        for name, v in target.items():
            q[k, col[name]] = w * v
    return q


@functools.lru_cache(maxsize=None)
def _reach_target_cached():
    rob = robot_model("unitree_g1")
    caps, _ = tables("unitree_g1")
    hand, head = caps.names.index("right_rubber_hand"), caps.names.index("head_mocap")
    pr = collision.PairTable(np.array([[min(hand, head), max(hand, head)]], np.int32))
    col = {rob.jnt_names[b]: int(rob.qpos_adr[b]) for b in range(rob.nbody) if rob.jnt_type[b] == R.JNT_HINGE}
    names = ("right_shoulder_pitch_joint", "right_shoulder_roll_joint", "right_elbow_joint")
    grid = [np.linspace(-3.0, 0.0, 13), np.linspace(-1.0, 1.0, 9), np.linspace(-1.0, 2.0, 13)]
    A, B, E = np.meshgrid(*grid, indexing="ij")
    q = np.repeat(di.standing("unitree_g1", 1), A.size, axis=0)
    for n, v in zip(names, (A, B, E)):
        lo, hi = rob.jnt_range[rob.qpos_adr.tolist().index(col[n])]
        q[:, col[n]] = np.clip(v.ravel(), lo, hi)
    cl = SR.pair_clearance(rob, caps, pr, q)[:, 0]
    i = int(np.argmin(cl))
    return tuple((n, float(q[i, col[n]])) for n in names), float(cl[i])


def reach_target():
    """{joint: angle} of the right arm that brings G1's right hand nearest its head on a coarse grid inside the joint ranges."""
    return dict(_reach_target_cached()[0])

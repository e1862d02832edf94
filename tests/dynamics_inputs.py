"""The inputs of the inverse-dynamics GPU tests and their reference answers, each computed once (tests/dynamics_reference.py).

Clips of 0, 1, 2, 3, 4, 63, 64, 65 and 130 frames at 64 Hz in one call: every length at which the differences take another path
(nothing, zero velocity, zero acceleration, one interior frame, two) and the 64-frame edges of the per-clip walk.  Clip s follows
the analytic trajectory of seed s (dynamics_reference.Trajectory), so its velocities and accelerations are known in closed form.

  explicit   qpos with the analytic qvel and qacc
  diff       the same qpos rounded to multiples of 2^-16 with qvel = qacc = None: differences of such rows over 1/64 s are exact in
             float64, so the linear and hinge parts of the contract's differences have one correct value, bit for bit

ROBOTS is the registry list.  Every function here takes a model by name, and dynamics_reference.model resolves a name of the form
``tree/<shape>/<nbody>`` to a synthetic tree of tests/synthetic_trees.py, so tests/test_gpu_tree_packing.py runs the same cases on
trees of every wavefront packing.
"""
import dataclasses
import functools

import numpy as np

from tests import dynamics_reference as R

LENS = [0, 1, 2, 3, 4, 63, 64, 65, 130]
OFFS = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
N, S = int(OFFS[-1]), len(LENS)
FPS = 64.0
ROBOTS = ["unitree_g1", "booster_k1", "unitree_g1_with_hands"]   # 38 bodies; 23, the fewest of the registry: two frames side by side; 52
QUANTUM = 2.0 ** -16


@functools.lru_cache(maxsize=None)
def explicit(robot, seed0=0):
    """(q, v, a) [N, .] float64, read-only."""
    rob, _ = R.model(robot)
    parts = [R.Trajectory(rob, seed0 + s).state([k / FPS for k in range(T)]) for s, T in enumerate(LENS) if T]
    out = tuple(np.concatenate([p[i] for p in parts]) for i in range(3))
    for t in out:
        t.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def quantised(robot, seed0=0):
    q = np.round(explicit(robot, seed0)[0] / QUANTUM) * QUANTUM
    q.setflags(write=False)
    return q


def with_statistics(robot, q, v, a, offs=OFFS, table=None):
    rob, tab = R.model(robot)
    tab = tab if table is None else table
    ref = R.dynamics(rob, tab, q, v, a)
    ref.update(R.statistics(tab, ref["tau"], ref["root_wrench"], offs))
    ref["qvel"], ref["qacc"] = v, a
    return ref


@functools.lru_cache(maxsize=None)
def reference(robot, case):
    """The numpy reference's answer to a named case, every output of the call by name."""
    if case == "explicit":
        return with_statistics(robot, *explicit(robot))
    q = quantised(robot)
    return with_statistics(robot, q, *R.differences(q, OFFS, FPS))


def margins(robot, ref, table=None):
    """How far the reference's own values are from the thresholds of the counted statistics, relative: (|tau| against the limits,
    F_z against the unloaded threshold).  A case whose margin is not far above rounding cannot ask for equal counts."""
    tab = R.model(robot)[1] if table is None else table
    ok = np.all(np.isfinite(ref["tau"]), axis=1) & np.all(np.isfinite(ref["root_wrench"]), axis=1)
    lim = np.where(np.isfinite(tab.torque_limit), tab.torque_limit, np.inf)
    with np.errstate(all="ignore"):
        m_tau = np.min(np.abs(np.abs(ref["tau"][ok]) / lim - 1.0)) if ok.any() and lim.size else np.inf   # (a model without a hinge has no torque)
    weight = tab.total_mass * 9.81
    m_fz = np.min(np.abs(ref["root_wrench"][ok, 2] / weight - R.FZ_MIN)) if ok.any() else np.inf
    return float(m_tau), float(m_fz)


def standing(robot, frames):
    """qpos [frames, nq] of the robot at rest: zero hinges, upright, the root 1 m up."""
    rob, _ = R.model(robot)
    q = np.zeros((frames, rob.nq))
    q[:, 2], q[:, 3] = 1.0, 1.0
    return q


@functools.lru_cache(maxsize=None)
def push_case(robot="unitree_g1"):
    """Three clips of 5 frames at rest with explicit zero velocity and acceleration, except that in frame 2 of clip 1 one distal hinge
    (the last of the model) is accelerated.  Only that hinge has a limit -- 1.5 times its largest static torque in the reference, at
    least 1 N m -- and the push is sized to take it to twice that limit.  Returns (q, v, a, offsets, table, (clip, row, hinge))."""
    rob, tab = R.model(robot)
    offs = np.array([0, 5, 10, 15], np.int64)
    q = standing(robot, 15)
    v, a = np.zeros((15, rob.nv)), np.zeros((15, rob.nv))
    rest = R.dynamics(rob, tab, q, v, a)["tau"]
    j = rob.nq - 8
    limit = np.full(rob.nq - 7, np.inf)
    limit[j] = max(1.5 * np.abs(rest[:, j]).max(), 1.0)
    table = dataclasses.replace(tab, torque_limit=limit)
    a1 = a.copy()
    a1[7, 6 + j] = 1.0
    slope = R.dynamics(rob, tab, q[7:8], v[7:8], a1[7:8])["tau"][0, j] - rest[7, j]     # tau is linear in the acceleration
    a = a.copy()
    a[7, 6 + j] = (2.0 * limit[j] - rest[7, j]) / slope
    return q, v, a, offs, table, (1, 7, j)


def free_fall(robot="unitree_g1", frames=12, z0=3.0):
    """One clip: the robot at rest falls freely, root z = z0 - 9.81 t^2 / 2, hinges fixed."""
    q = standing(robot, frames)
    t = np.arange(frames) / FPS
    q[:, 2] = z0 - 0.5 * 9.81 * t * t
    return q, np.array([0, frames], np.int64)


def floor_rows(robot, per_kind=4):
    """The rows of the explicit case at which tests/test_dynamics_host.py re-measures the numpy reference against 50 digits: per kind
    the `per_kind` rows with the largest |tau|, the largest |root_wrench|, the smallest loaded F_z (where the ZMP, a quotient by F_z,
    is worst conditioned) and the largest |zmp|, plus every clip's first row."""
    ref = reference(robot, "explicit")
    loaded = ~np.isnan(ref["zmp"]).any(axis=1)
    keys = [np.abs(ref["tau"]).max(axis=1, initial=0.0), np.abs(ref["root_wrench"]).max(axis=1), np.where(loaded, -ref["root_wrench"][:, 2], -np.inf),
            np.where(loaded, np.abs(np.nan_to_num(ref["zmp"])).max(axis=1), -np.inf)]
    rows = set(int(OFFS[s]) for s, T in enumerate(LENS) if T)
    for key in keys:
        rows.update(int(i) for i in np.argsort(key)[-per_kind:])
    return sorted(rows)


def measure_floor(robot, rows=None):
    """Worst |numpy reference - 50-digit evaluator| per output over `rows` of the explicit case (None: all of them), on the very
    frames the GPU is compared at.  Unloaded frames have no ZMP and are left out of its figure."""
    rob, tab = R.model(robot)
    ref = reference(robot, "explicit")
    worst = {k: 0.0 for k in ("tau", "root_wrench", "com", "zmp")}
    trajs = {}
    for row in (range(N) if rows is None else rows):
        s = int(np.searchsorted(OFFS, row, side="right")) - 1
        tr = trajs.setdefault(s, R.Trajectory(rob, s))
        want = R.mp_dynamics(tr, tab, R.mpf(row - int(OFFS[s])) / R.mpf(FPS))
        for k in worst:
            if k == "zmp" and np.isnan(ref[k][row]).any():
                continue
            worst[k] = max(worst[k], float(np.abs(ref[k][row] - want[k]).max(initial=0.0)))   # (no tau without a hinge)
    return worst

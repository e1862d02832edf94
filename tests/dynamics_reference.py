"""Inverse dynamics: the contract above gmr_dynamics_input (include/gmr_amd.h) restated twice, without a GPU and without native code.

(1) numpy float64, vectorised over frames (`differences`, `dynamics`, `statistics`).  The kinematics are written as SUMS OVER
    ANCESTORS -- a body's angular velocity is the root's plus its ancestors' hinge rates, a point's velocity and acceleration are
    the root's plus one term per ancestor hinge -- and W(p, set) is summed over explicit subtree sets.  Nothing here carries a
    velocity or a wrench from a parent to a child or back: no recursion is shared with the kernel's two sweeps.
(2) mpmath at 50 digits (`mp_dynamics`), along an analytic trajectory (`Trajectory`): root position a cubic in time, root rotation
    exp(t a) (x) q0, hinges sinusoids inside their ranges.  Only poses and angular velocities are evaluated; c_i'' and
    d/dt(R_i I_i R_i^T w_i) are central differences in 50 digits (step 1e-12: truncation 1e-24, rounding 1e-26), so this evaluator
    shares no velocity or acceleration algebra with (1) either.  `mp_energy_rate` is d/dt of kinetic plus potential energy.

Quaternions are wxyz.  FK is the IK side's: MuJoCo's convention, the root quaternion divided by its norm, unit body quaternions.
"""
import functools
import os

import mpmath
import numpy as np

from gmr_amd.inertial import InertialTable, load_inertial
from gmr_amd.mjcf import JNT_HINGE, load_mjcf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "tests", "golden", "gmr_root", "assets")
XML = {"unitree_g1": "unitree_g1/g1_mocap_29dof.xml", "unitree_g1_with_hands": "unitree_g1/g1_mocap_29dof_with_hands.xml",
       "booster_k1": "booster_k1/K1_serial.xml", "booster_t1": "booster_t1/t1_mocap.xml", "galaxea_r1pro": "galaxea_r1pro/r1_pro.xml"}
GRAVITY = (0.0, 0.0, -9.81)
FZ_MIN = 0.05

mp = mpmath.MPContext()   # a context of this module's own
mp.dps = 50
mpf = mp.mpf

# |numpy reference - 50-digit evaluator| per robot, measured on the very frames the GPU tests compare at: every frame of the explicit case
# of tests/dynamics_inputs.py (332 frames per robot, the lightly loaded ones included, where the ZMP -- a quotient by F_z -- is worst
# conditioned), by dynamics_inputs.measure_floor(robot) (x86-64, numpy float64; 76 s for the three), rounded up to one digit:
#     unitree_g1             tau 1.92e-13   root_wrench 3.98e-13   com 3.55e-15   zmp 5.97e-13
#     booster_k1             tau 9.59e-14   root_wrench 2.84e-13   com 3.55e-15   zmp 1.85e-13
#     unitree_g1_with_hands  tau 4.69e-13   root_wrench 1.48e-12   com 5.33e-15   zmp 7.92e-13
# tests/test_dynamics_host.py re-measures the rows of dynamics_inputs.floor_rows (the extremes of every output, which hold the ZMP's
# worst) and fails if a recorded figure is smaller than what it measures.  Nothing here was measured on a kernel.  The GPU tests allow
# GPU_FACTOR times these, as absolute bounds, with no other factor.
FLOAT_WORST = {"unitree_g1": {"tau": 2e-13, "root_wrench": 4e-13, "com": 4e-15, "zmp": 6e-13},
               "booster_k1": {"tau": 1e-13, "root_wrench": 3e-13, "com": 4e-15, "zmp": 2e-13},
               "unitree_g1_with_hands": {"tau": 5e-13, "root_wrench": 2e-12, "com": 6e-15, "zmp": 8e-13}}
# The same for the synthetic trees of tests/synthetic_trees.py (TREES), measured the same way over all 332 frames of each tree's
# explicit case (x86-64, numpy float64; 86 s for the slowest, the chain of 64 bodies) and rounded up to one digit; re-measured on
# dynamics_inputs.floor_rows by tests/test_synthetic_trees_host.py.  A chain's figures grow with its depth: the reference sums one
# term per ancestor hinge, and the 64-body chain's last body has 48.  tree/chain/1 has no hinge and so no tau.
#     tree/chain/1   tau 0.00e+00   root_wrench 1.70e-15   com 1.78e-15   zmp 2.70e-13
#     tree/chain/2   tau 8.53e-16   root_wrench 1.98e-14   com 1.78e-15   zmp 4.83e-13
#     tree/chain/3   tau 6.00e-15   root_wrench 2.13e-14   com 1.78e-15   zmp 4.26e-13
#     tree/chain/4   tau 1.17e-14   root_wrench 1.15e-13   com 1.78e-15   zmp 1.79e-12
#     tree/chain/5   tau 1.75e-14   root_wrench 1.24e-13   com 3.55e-15   zmp 4.69e-13
#     tree/chain/8   tau 6.39e-14   root_wrench 1.88e-13   com 3.55e-15   zmp 6.11e-13
#     tree/chain/9   tau 1.74e-13   root_wrench 2.98e-13   com 3.55e-15   zmp 8.38e-13
#     tree/chain/16  tau 3.87e-13   root_wrench 6.25e-13   com 3.55e-15   zmp 3.34e-13
#     tree/chain/17  tau 3.41e-13   root_wrench 5.74e-13   com 7.11e-15   zmp 2.88e-13
#     tree/chain/32  tau 1.39e-12   root_wrench 4.18e-12   com 7.11e-15   zmp 3.58e-12
#     tree/chain/33  tau 2.10e-12   root_wrench 4.32e-12   com 5.33e-15   zmp 2.27e-12
#     tree/chain/64  tau 3.91e-11   root_wrench 6.37e-11   com 7.11e-15   zmp 9.56e-11
#     tree/star/5    tau 4.62e-15   root_wrench 3.64e-14   com 1.78e-15   zmp 5.12e-13
#     tree/star/9    tau 9.60e-15   root_wrench 6.13e-14   com 2.66e-15   zmp 4.26e-13
#     tree/star/17   tau 8.62e-15   root_wrench 1.03e-13   com 1.78e-15   zmp 4.41e-13
#     tree/star/33   tau 9.05e-15   root_wrench 2.27e-13   com 3.55e-15   zmp 1.56e-13
#     tree/star/64   tau 9.64e-15   root_wrench 4.55e-13   com 5.33e-15   zmp 3.13e-13
#     tree/comb/5    tau 4.58e-15   root_wrench 2.66e-14   com 1.78e-15   zmp 3.27e-13
#     tree/comb/9    tau 9.46e-15   root_wrench 7.46e-14   com 3.55e-15   zmp 4.97e-13
#     tree/comb/17   tau 6.75e-14   root_wrench 2.84e-13   com 3.55e-15   zmp 1.15e-12
#     tree/comb/33   tau 2.13e-13   root_wrench 4.55e-13   com 3.55e-15   zmp 3.41e-13
#     tree/comb/64   tau 6.22e-13   root_wrench 4.87e-12   com 8.88e-15   zmp 9.66e-13
FLOAT_WORST.update({
    "tree/chain/1": {"tau": 0.0, "root_wrench": 2e-15, "com": 2e-15, "zmp": 3e-13},
    "tree/chain/2": {"tau": 9e-16, "root_wrench": 2e-14, "com": 2e-15, "zmp": 5e-13},
    "tree/chain/3": {"tau": 6e-15, "root_wrench": 3e-14, "com": 2e-15, "zmp": 5e-13},
    "tree/chain/4": {"tau": 2e-14, "root_wrench": 2e-13, "com": 2e-15, "zmp": 2e-12},
    "tree/chain/5": {"tau": 2e-14, "root_wrench": 2e-13, "com": 4e-15, "zmp": 5e-13},
    "tree/chain/8": {"tau": 7e-14, "root_wrench": 2e-13, "com": 4e-15, "zmp": 7e-13},
    "tree/chain/9": {"tau": 2e-13, "root_wrench": 3e-13, "com": 4e-15, "zmp": 9e-13},
    "tree/chain/16": {"tau": 4e-13, "root_wrench": 7e-13, "com": 4e-15, "zmp": 4e-13},
    "tree/chain/17": {"tau": 4e-13, "root_wrench": 6e-13, "com": 8e-15, "zmp": 3e-13},
    "tree/chain/32": {"tau": 2e-12, "root_wrench": 5e-12, "com": 8e-15, "zmp": 4e-12},
    "tree/chain/33": {"tau": 3e-12, "root_wrench": 5e-12, "com": 6e-15, "zmp": 3e-12},
    "tree/chain/64": {"tau": 4e-11, "root_wrench": 7e-11, "com": 8e-15, "zmp": 1e-10},
    "tree/star/5": {"tau": 5e-15, "root_wrench": 4e-14, "com": 2e-15, "zmp": 6e-13},
    "tree/star/9": {"tau": 1e-14, "root_wrench": 7e-14, "com": 3e-15, "zmp": 5e-13},
    "tree/star/17": {"tau": 9e-15, "root_wrench": 2e-13, "com": 2e-15, "zmp": 5e-13},
    "tree/star/33": {"tau": 1e-14, "root_wrench": 3e-13, "com": 4e-15, "zmp": 2e-13},
    "tree/star/64": {"tau": 1e-14, "root_wrench": 5e-13, "com": 6e-15, "zmp": 4e-13},
    "tree/comb/5": {"tau": 5e-15, "root_wrench": 3e-14, "com": 2e-15, "zmp": 4e-13},
    "tree/comb/9": {"tau": 1e-14, "root_wrench": 8e-14, "com": 4e-15, "zmp": 5e-13},
    "tree/comb/17": {"tau": 7e-14, "root_wrench": 3e-13, "com": 4e-15, "zmp": 2e-12},
    "tree/comb/33": {"tau": 3e-13, "root_wrench": 5e-13, "com": 4e-15, "zmp": 4e-13},
    "tree/comb/64": {"tau": 7e-13, "root_wrench": 5e-12, "com": 9e-15, "zmp": 1e-12}})
GPU_FACTOR = 10.0


def bound(robot, output):
    """The largest admissible |kernel - numpy reference| of an output: ten times the numpy reference's own measured distance to 50
    digits on the same frames."""
    return GPU_FACTOR * FLOAT_WORST[robot][output]


@functools.lru_cache(maxsize=None)
def model(robot):
    """(RobotModel, InertialTable) of a registry robot, from the MJCF files under tests/golden; a name ``tree/<shape>/<nbody>`` is a
    synthetic tree of tests/synthetic_trees.py."""
    if robot.startswith("tree/"):
        from tests import synthetic_trees
        return synthetic_trees.model(robot)
    path = os.path.join(ASSETS, XML[robot])
    return load_mjcf(path, name=robot), load_inertial(path)


def ancestors(rob):
    """Per body the hinge bodies on its path from the root, the body itself included, root side first."""
    out = []
    for b in range(rob.nbody):
        path, j = [], b
        while j >= 0:
            if rob.jnt_type[j] == JNT_HINGE:
                path.append(j)
            j = int(rob.parent[j])
        out.append(path[::-1])
    return out


def subtrees(rob):
    """Per body the explicit set of bodies of its subtree (itself included), ascending."""
    sets = [[b] for b in range(rob.nbody)]
    for b in range(rob.nbody - 1, 0, -1):
        j = int(rob.parent[b])
        while j >= 0:
            sets[j].append(b)
            j = int(rob.parent[j])
    return [sorted(set(s)) for s in sets]


# ------------------------------------------------------------------ numpy float64
def _qmul(a, b):
    aw, ax, ay, az = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bw, bx, by, bz = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def _rot(q, v):
    t = 2.0 * np.cross(q[..., 1:], v)
    return v + q[..., :1] * t + np.cross(q[..., 1:], t)


def _mat(q):
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def fk(rob, q):
    """World positions [N, nb, 3] and unit quaternions [N, nb, 4] of every body."""
    N = q.shape[0]
    X, Q = np.zeros((N, rob.nbody, 3)), np.zeros((N, rob.nbody, 4))
    X[:, 0] = q[:, 0:3]
    Q[:, 0] = q[:, 3:7] / np.sqrt(np.sum(q[:, 3:7] * q[:, 3:7], axis=1, keepdims=True))
    for b in range(1, rob.nbody):
        p = int(rob.parent[b])
        X[:, b] = X[:, p] + _rot(Q[:, p], rob.body_pos[b])
        r = _qmul(Q[:, p], np.broadcast_to(rob.body_quat[b], (N, 4)))
        if rob.jnt_type[b] == JNT_HINGE:
            h = 0.5 * q[:, rob.qpos_adr[b]]
            r = _qmul(r, np.concatenate([np.cos(h)[:, None], np.sin(h)[:, None] * rob.jnt_axis[b]], 1))
        Q[:, b] = r
    return X, Q


def dynamics(rob, tab: InertialTable, q, v, a, gravity=GRAVITY, ground_z=0.0, fz_min=FZ_MIN):
    """tau [N, nh], root_wrench [N, 6], com [N, 3], zmp [N, 2] of explicit (q, v, a); v and a with the root's angular part in the
    world frame."""
    q, v, a = (np.asarray(t, dtype=np.float64) for t in (q, v, a))
    N, nb = q.shape[0], rob.nbody
    g = np.asarray(gravity, dtype=np.float64)
    X, Q = fk(rob, q)
    anc, sub = ancestors(rob), subtrees(rob)
    hinges = [b for b in range(nb) if rob.jnt_type[b] == JNT_HINGE]
    ax = {j: _rot(Q[:, j], rob.jnt_axis[j]) for j in hinges}
    qd = {j: v[:, rob.dof_adr[j]][:, None] for j in hinges}
    qdd = {j: a[:, rob.dof_adr[j]][:, None] for j in hinges}
    x0, v0, w0, a0, wd0 = X[:, 0], v[:, 0:3], v[:, 3:6], a[:, 0:3], a[:, 3:6]
    w = [w0 + sum((ax[l] * qd[l] for l in anc[b]), np.zeros((N, 3))) for b in range(nb)]
    dax = {j: np.cross(w[j], ax[j]) for j in hinges}                 # d/dt of the world axis
    spin = {j: dax[j] * qd[j] + ax[j] * qdd[j] for j in hinges}      # d/dt of (axis rate)

    def vel(pt, b):
        return v0 + np.cross(w0, pt - x0) + sum((np.cross(ax[l] * qd[l], pt - X[:, l]) for l in anc[b]), np.zeros((N, 3)))

    pd = {j: vel(X[:, j], j) for j in hinges}
    F_i, L_i, C = [], [], []
    for b in range(nb):
        c = X[:, b] + _rot(Q[:, b], tab.com[b])
        cd = vel(c, b)
        cdd = a0 + np.cross(wd0, c - x0) + np.cross(w0, cd - v0)
        for l in anc[b]:
            cdd = cdd + np.cross(spin[l], c - X[:, l]) + np.cross(ax[l] * qd[l], cd - pd[l])
        wd = wd0 + sum((spin[l] for l in anc[b]), np.zeros((N, 3)))
        R = _mat(Q[:, b])
        Iw = R @ tab.inertia[b] @ np.swapaxes(R, -1, -2)
        Iom = np.einsum("nij,nj->ni", Iw, w[b])
        L_i.append(np.einsum("nij,nj->ni", Iw, wd) + np.cross(w[b], Iom))
        F_i.append(tab.mass[b] * (cdd - g))
        C.append(c)

    def W(p, bodies):
        s = np.zeros((N, 3))
        for i in bodies:
            s = s + (np.cross(C[i] - p, F_i[i]) + L_i[i])
        return s

    tau = np.zeros((N, len(hinges)))
    for j in hinges:
        k = rob.qpos_adr[j] - 7
        tau[:, k] = np.sum(ax[j] * W(X[:, j], sub[j]), axis=1) + tab.armature[k] * qdd[j][:, 0]
    F = np.zeros((N, 3))
    mc = np.zeros((N, 3))
    mtot = 0.0
    for i in range(nb):
        F = F + F_i[i]
        mc = mc + tab.mass[i] * C[i]
        mtot = mtot + float(tab.mass[i])
    M = W(x0, range(nb))
    Mo = M + np.cross(x0, F)
    with np.errstate(all="ignore"):
        zmp = np.stack([(ground_z * F[:, 0] - Mo[:, 1]) / F[:, 2], (Mo[:, 0] + ground_z * F[:, 1]) / F[:, 2]], -1)
    zmp[F[:, 2] < fz_min * (mtot * np.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]))] = np.nan
    return {"tau": tau, "root_wrench": np.concatenate([F, M], 1), "com": mc / mtot, "zmp": zmp}


def _rotvec_rate(p, q, h):
    """rotvec(p (x) conj(q)) / h, gmr_motion_track's formula in its operation order (rows of wxyz quaternions)."""
    w = p[:, 0] * q[:, 0] + (p[:, 1] * q[:, 1] + p[:, 2] * q[:, 2] + p[:, 3] * q[:, 3])
    vx = q[:, 0] * p[:, 1] - p[:, 0] * q[:, 1] - (p[:, 2] * q[:, 3] - p[:, 3] * q[:, 2])
    vy = q[:, 0] * p[:, 2] - p[:, 0] * q[:, 2] - (p[:, 3] * q[:, 1] - p[:, 1] * q[:, 3])
    vz = q[:, 0] * p[:, 3] - p[:, 0] * q[:, 3] - (p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1])
    v = np.stack([vx, vy, vz], -1)
    neg = w < 0.0
    w = np.where(neg, -w, w)
    v = np.where(neg[:, None], -v, v)
    n = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    with np.errstate(all="ignore"):
        f = np.where(n > 1e-12, 2.0 * np.arctan2(n, w) / n, 2.0)
    return v * f[:, None] / h


def differences(qpos, seq_offsets, fps):
    """qvel, qacc [N, nv] of the contract's differences (velocity as the tracking export, second differences, ends copied)."""
    qpos = np.asarray(qpos, dtype=np.float64)
    N, nq = qpos.shape
    dt = 1.0 / float(fps)
    lin = [0, 1, 2] + list(range(7, nq))
    vcol = [0, 1, 2] + list(range(6, nq - 1))
    qvel, qacc = np.zeros((N, nq - 1)), np.zeros((N, nq - 1))
    with np.errstate(all="ignore"):
        for s in range(len(seq_offsets) - 1):
            a, b = int(seq_offsets[s]), int(seq_offsets[s + 1])
            T = b - a
            if T < 2:
                continue
            q = qpos[a:b]
            k = np.arange(T)
            km, kp = np.maximum(k - 1, 0), np.minimum(k + 1, T - 1)
            hv = (kp - km).astype(np.float64) * dt
            qvel[a:b][:, vcol] = (q[kp][:, lin] - q[km][:, lin]) / hv[:, None]
            qvel[a:b, 3:6] = _rotvec_rate(q[kp][:, 3:7], q[km][:, 3:7], hv[:, None])
            if T < 3:
                continue
            kc = np.clip(k, 1, T - 2)
            qacc[a:b][:, vcol] = ((q[kc + 1][:, lin] - 2.0 * q[kc][:, lin]) + q[kc - 1][:, lin]) / (dt * dt)
            wp = _rotvec_rate(q[kc + 1][:, 3:7], q[kc][:, 3:7], dt)
            wm = _rotvec_rate(q[kc][:, 3:7], q[kc - 1][:, 3:7], dt)
            qacc[a:b, 3:6] = (wp - wm) / dt
    return qvel, qacc


def statistics(tab: InertialTable, tau, wrench, seq_offsets, gravity=GRAVITY, fz_min=FZ_MIN):
    """The per-clip statistics of the contract from tau [N, nh] and root_wrench [N, 6], frame by frame."""
    S, nh = len(seq_offsets) - 1, tau.shape[1]
    g = np.asarray(gravity, dtype=np.float64)
    weight = tab.total_mass * np.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2])
    thr = fz_min * weight
    f64, i32 = np.float64, np.int32
    out = {"tau_abs_max": np.zeros((S, nh), f64), "tau_rms": np.zeros((S, nh), f64), "tau_ratio_max": np.zeros((S, nh), f64),
           "frames_over_limit": np.zeros((S, nh), i32), "frames_any_over_limit": np.zeros(S, i32), "fz_ratio_max": np.zeros(S, f64),
           "fz_ratio_min": np.zeros(S, f64), "unloaded_frames": np.zeros(S, i32), "nonfinite_frames": np.zeros(S, i32)}
    for s in range(S):
        ss, n = np.zeros(nh), 0
        for k in range(int(seq_offsets[s]), int(seq_offsets[s + 1])):
            if not (np.all(np.isfinite(tau[k])) and np.all(np.isfinite(wrench[k]))):
                out["nonfinite_frames"][s] += 1
                continue
            at = np.abs(tau[k])
            over = at > tab.torque_limit
            out["tau_abs_max"][s] = np.maximum(out["tau_abs_max"][s], at)
            out["tau_ratio_max"][s] = np.maximum(out["tau_ratio_max"][s], at / tab.torque_limit)
            ss = ss + tau[k] * tau[k]
            out["frames_over_limit"][s] += over
            out["frames_any_over_limit"][s] += bool(over.any())
            fzr = wrench[k, 2] / weight
            out["fz_ratio_max"][s] = fzr if n == 0 else max(out["fz_ratio_max"][s], fzr)
            out["fz_ratio_min"][s] = fzr if n == 0 else min(out["fz_ratio_min"][s], fzr)
            out["unloaded_frames"][s] += bool(wrench[k, 2] < thr)
            n += 1
        if n:
            out["tau_rms"][s] = np.sqrt(ss / float(n))
    return out


# ------------------------------------------------------------------ the analytic trajectory and the 50-digit evaluator
class Trajectory:
    """Root position p0 + p1 t + p2 t^2 + p3 t^3, root rotation exp(t a) (x) q0, hinge j at mid_j + amp_j sin(om_j t + ph_j) inside
    its range (+-1 rad for an unlimited hinge).  All parameters are float64 values taken exactly."""

    def __init__(self, rob, seed):
        rng = np.random.default_rng(seed)
        self.rob = rob
        self.p = [rng.uniform(-1, 1, 3) * s + o for s, o in ((0.5, (0, 0, 0.9)), (1.0, 0), (2.0, 0), (1.0, 0))]
        self.a = rng.uniform(-2.0, 2.0, 3)
        q0 = rng.normal(size=4)
        self.q0 = q0 / np.linalg.norm(q0)
        self.hinges = [b for b in range(rob.nbody) if rob.jnt_type[b] == JNT_HINGE]
        lo = np.array([rob.jnt_range[b, 0] if rob.jnt_limited[b] else -1.0 for b in self.hinges])
        hi = np.array([rob.jnt_range[b, 1] if rob.jnt_limited[b] else 1.0 for b in self.hinges])
        self.mid, self.amp = 0.5 * (lo + hi), 0.45 * (hi - lo) * rng.uniform(0.3, 1.0, len(self.hinges))
        self.om, self.ph = rng.uniform(2.0, 9.0, len(self.hinges)), rng.uniform(0, 6.28, len(self.hinges))

    def mp_q(self, t):
        """qpos at the mpf time t, as a list of mpf."""
        t = mpf(t)
        pos = [mpf(self.p[0][c]) + mpf(self.p[1][c]) * t + mpf(self.p[2][c]) * t * t + mpf(self.p[3][c]) * t * t * t for c in range(3)]
        a = [mpf(x) for x in self.a]
        na = mp.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
        e = (mp.cos(na * t / 2),) + tuple(mp.sin(na * t / 2) * x / na for x in a)
        q0 = [mpf(x) for x in self.q0]
        n0 = mp.sqrt(sum(x * x for x in q0))
        quat = _mp_qmul(e, tuple(x / n0 for x in q0))
        th = [mpf(self.mid[i]) + mpf(self.amp[i]) * mp.sin(mpf(self.om[i]) * t + mpf(self.ph[i])) for i in range(len(self.hinges))]
        return pos + list(quat) + th

    def mp_rates(self, t):
        """(root linear velocity, root angular velocity (world), hinge rates) and the same for accelerations, mpf."""
        t = mpf(t)
        v = [mpf(self.p[1][c]) + 2 * mpf(self.p[2][c]) * t + 3 * mpf(self.p[3][c]) * t * t for c in range(3)]
        acc = [2 * mpf(self.p[2][c]) + 6 * mpf(self.p[3][c]) * t for c in range(3)]
        w = [mpf(x) for x in self.a]
        thd = [mpf(self.amp[i]) * mpf(self.om[i]) * mp.cos(mpf(self.om[i]) * t + mpf(self.ph[i])) for i in range(len(self.hinges))]
        thdd = [-mpf(self.amp[i]) * mpf(self.om[i]) ** 2 * mp.sin(mpf(self.om[i]) * t + mpf(self.ph[i])) for i in range(len(self.hinges))]
        return v + w + thd, acc + [mpf(0)] * 3 + thdd

    def state(self, times):
        """(q, v, a) as float64 arrays [len(times), .], each entry rounded once from 50 digits."""
        q = np.array([[float(x) for x in self.mp_q(t)] for t in times])
        va = [self.mp_rates(t) for t in times]
        return q, np.array([[float(x) for x in r[0]] for r in va]), np.array([[float(x) for x in r[1]] for r in va])


def _mp_qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return (aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
            aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw)


def _mp_cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _mp_matvec(R, v):
    return tuple(R[i][0] * v[0] + R[i][1] * v[1] + R[i][2] * v[2] for i in range(3))


def _mp_mat(q):
    w, x, y, z = q
    return ((1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)),
            (2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)),
            (2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)))


def _mp_pose(traj, tab, t):
    """Per body at time t: origin x, rotation matrix R, centre of mass c, angular velocity w, angular momentum about c; and the world
    hinge axes.  Angular velocities are sums of the root's and the ancestors' hinge rates."""
    rob = traj.rob
    q = traj.mp_q(t)
    rates, _ = traj.mp_rates(t)
    n = mp.sqrt(sum(x * x for x in q[3:7]))
    X, Q = [tuple(q[0:3])], [tuple(x / n for x in q[3:7])]
    for b in range(1, rob.nbody):
        p = int(rob.parent[b])
        Rp = _mp_mat(Q[p])
        d = _mp_matvec(Rp, [mpf(float(x)) for x in rob.body_pos[b]])
        X.append(tuple(X[p][c] + d[c] for c in range(3)))
        r = _mp_qmul(Q[p], tuple(mpf(float(x)) for x in rob.body_quat[b]))
        if rob.jnt_type[b] == JNT_HINGE:
            h = q[rob.qpos_adr[b]] / 2
            axv = [mpf(float(x)) for x in rob.jnt_axis[b]]
            r = _mp_qmul(r, (mp.cos(h),) + tuple(mp.sin(h) * x for x in axv))
        Q.append(r)
    anc = ancestors(rob)
    out, axes = [], {}
    for b in range(rob.nbody):
        R = _mp_mat(Q[b])
        if rob.jnt_type[b] == JNT_HINGE:
            axes[b] = _mp_matvec(R, [mpf(float(x)) for x in rob.jnt_axis[b]])
    for b in range(rob.nbody):
        R = _mp_mat(Q[b])
        s = _mp_matvec(R, [mpf(float(x)) for x in tab.com[b]])
        c = tuple(X[b][k] + s[k] for k in range(3))
        w = list(rates[3:6])
        for l in anc[b]:
            for k in range(3):
                w[k] = w[k] + axes[l][k] * rates[rob.dof_adr[l]]
        Rt = tuple(zip(*R))
        I = [[mpf(float(x)) for x in row] for row in tab.inertia[b]]
        L = _mp_matvec(R, _mp_matvec(I, _mp_matvec(Rt, w)))
        out.append({"x": X[b], "c": c, "w": tuple(w), "L": L})
    return out, axes


def mp_dynamics(traj, tab, t, gravity=GRAVITY, ground_z=0.0, step="1e-12"):
    """The contract's outputs at time t in 50 digits (floats, rounded once): c'' and dL/dt by central differences of step `step`."""
    rob, d = traj.rob, mpf(step)
    t = mpf(t)
    g = [mpf(float(x)) for x in gravity]
    (Pm, _), (P0, axes), (Pp, _) = _mp_pose(traj, tab, t - d), _mp_pose(traj, tab, t), _mp_pose(traj, tab, t + d)
    _, acc = traj.mp_rates(t)
    nb = rob.nbody
    f, Ld = [], []
    for b in range(nb):
        cdd = tuple((Pp[b]["c"][k] - 2 * P0[b]["c"][k] + Pm[b]["c"][k]) / (d * d) for k in range(3))
        f.append(tuple(mpf(float(tab.mass[b])) * (cdd[k] - g[k]) for k in range(3)))
        Ld.append(tuple((Pp[b]["L"][k] - Pm[b]["L"][k]) / (2 * d) for k in range(3)))

    def W(p, bodies):
        s = [mpf(0)] * 3
        for i in bodies:
            m = _mp_cross(tuple(P0[i]["c"][k] - p[k] for k in range(3)), f[i])
            s = [s[k] + m[k] + Ld[i][k] for k in range(3)]
        return s

    sub = subtrees(rob)
    tau = []
    for j in range(nb):
        if rob.jnt_type[j] == JNT_HINGE:
            w = W(P0[j]["x"], sub[j])
            k = rob.qpos_adr[j] - 7
            tau.append(sum(axes[j][c] * w[c] for c in range(3)) + mpf(float(tab.armature[k])) * acc[rob.dof_adr[j]])
    F = [sum(f[i][k] for i in range(nb)) for k in range(3)]
    x0 = P0[0]["x"]
    M = W(x0, range(nb))
    mtot = sum(mpf(float(m)) for m in tab.mass)
    com = [sum(mpf(float(tab.mass[i])) * P0[i]["c"][k] for i in range(nb)) / mtot for k in range(3)]
    xf = _mp_cross(x0, F)
    Mo = [M[k] + xf[k] for k in range(3)]
    gz = mpf(float(ground_z))
    zmp = [(gz * F[0] - Mo[1]) / F[2], (Mo[0] + gz * F[1]) / F[2]]
    fl = lambda xs: np.array([float(x) for x in xs])   # noqa: E731
    return {"tau": fl(tau), "root_wrench": fl(F + M), "com": fl(com), "zmp": fl(zmp)}


def mp_energy_rate(traj, tab, t, gravity=GRAVITY, step="1e-15", outer="1e-10"):
    """d/dt of kinetic plus potential energy at time t in 50 digits: sum of m |c'|^2 / 2 + w . L / 2 - m g . c over the bodies plus
    armature theta'^2 / 2 over the hinges, c' a central difference (`step`), the derivative a central difference (`outer`)."""
    rob, d, D = traj.rob, mpf(step), mpf(outer)
    g = [mpf(float(x)) for x in gravity]

    def energy(tt):
        (Pm, _), (P0, _), (Pp, _) = _mp_pose(traj, tab, tt - d), _mp_pose(traj, tab, tt), _mp_pose(traj, tab, tt + d)
        rates, _ = traj.mp_rates(tt)
        e = mpf(0)
        for b in range(rob.nbody):
            m = mpf(float(tab.mass[b]))
            cd = [(Pp[b]["c"][k] - Pm[b]["c"][k]) / (2 * d) for k in range(3)]
            e += m * sum(x * x for x in cd) / 2 + sum(P0[b]["w"][k] * P0[b]["L"][k] for k in range(3)) / 2
            e -= m * sum(g[k] * P0[b]["c"][k] for k in range(3))
        for j in range(rob.nbody):
            if rob.jnt_type[j] == JNT_HINGE:
                e += mpf(float(tab.armature[rob.qpos_adr[j] - 7])) * rates[rob.dof_adr[j]] ** 2 / 2
        return e

    t = mpf(t)
    return float((energy(t + D) - energy(t - D)) / (2 * D))

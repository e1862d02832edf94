"""A certificate for IK results: numpy float64, written from the definition of the problem alone.

Every other IK assertion of the suite compares the HIP kernel with ``oracle/gmr_oracle.c``; both read the same compiled blob
and restate the same loop, so an error made before the blob (an axis, an offset, a weight taken from the wrong slot) or in the
shared reading of the loop is invisible to them.  This module shares neither: it does not import ``oracle``, it never touches
``compile_model`` or its blob, it has no Jacobian, no QP and no iteration.  It reads the robot as ``gmr_amd.mjcf.load_robot``
returns it and the config as ``gmr_amd.ik_config.load_ik_config`` returns it, and answers one question about a qpos somebody
else computed: is it a constrained stationary point of the stage cost

    cost(table, q) = 1/2 sum_tasks ( w_p^2 |e_pos|^2 + w_r^2 |e_rot|^2 ),   (e_pos, e_rot) = log( T_body(q)^-1 T_target )

(the body-frame SE(3) log: mink's ``FrameTask`` error) under the joint ranges?  At a fixed point of the damped Gauss-Newton /
box-QP iteration dq = 0 solves the QP, which is exactly: the gradient of this cost vanishes on the free dofs and points into
the bound on the active ones -- whatever ``damping``, ``lm_damping`` and ``limit_gain`` are.

What it does NOT pin: the definition of the task error and of the target preparation are still this project's reading of
mink / of the reference's ``motion_retarget.py``; parity with the reference itself stays unpinned.
"""
import numpy as np

from gmr_amd.mjcf import JNT_FREE, JNT_HINGE

# Central-difference step of `gradient`: truncation ~ h^2 (1e-12 relative), rounding ~ eps * cost / h (1e-10 * cost).
FD_STEP = 1e-6
# A limited hinge counts as sitting on a bound within this distance: a constant of the certificate, not of any solver, well
# above the 7.9e-10 rad to which kernel and oracle agree and far below any distance the iteration leaves by choice.
ACTIVE_TOL = 1e-9


# ------------------------------------------------------------------ quaternions (wxyz) and the SE(3) log, vectorised over leading axes
def _qmul(a, b):
    aw, ax, ay, az = (a[..., i] for i in range(4))
    bw, bx, by, bz = (b[..., i] for i in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=-1)


def _qconj(a):
    return a * np.array([1.0, -1.0, -1.0, -1.0])


def _unit(q):
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def _qrot(q, v):
    """v turned by the unit quaternion q."""
    u = q[..., 1:]
    t = 2.0 * np.cross(u, v)
    return v + q[..., :1] * t + np.cross(u, t)


def _qexp(w):
    """Unit quaternion of the rotation vector w."""
    w = np.asarray(w, dtype=np.float64)
    ang = np.linalg.norm(w, axis=-1, keepdims=True)
    small = ang < 1e-8
    k = np.where(small, 0.5 - ang * ang / 48.0, np.sin(0.5 * ang) / np.where(small, 1.0, ang))
    return np.concatenate([np.cos(0.5 * ang), k * w], axis=-1)


def so3_log(q):
    """Rotation vector (angle in [0, pi]) of a unit quaternion."""
    q = np.where(q[..., :1] < 0.0, -q, q)
    v, w = q[..., 1:], q[..., :1]
    n = np.linalg.norm(v, axis=-1, keepdims=True)
    small = n < 1e-8
    # 2 atan2(n, w) / n;  near n = 0 (w = sqrt(1 - n^2)): 2 + n^2 / 3 + O(n^4)
    f = np.where(small, 2.0 + n * n / 3.0, 2.0 * np.arctan2(n, w) / np.where(small, 1.0, n))
    return f * v


def se3_log(q, t):
    """[V(omega)^-1 t, omega] of the rigid transform (unit quaternion q, translation t)."""
    om = so3_log(q)
    th2 = np.sum(om * om, axis=-1, keepdims=True)
    small = th2 < 1e-8
    th = np.sqrt(np.where(small, 1.0, th2))
    # (1 - (theta / 2) cot(theta / 2)) / theta^2 = 1/12 + theta^2 / 720 + O(theta^4)
    c2 = np.where(small, 1.0 / 12.0 + th2 / 720.0, (1.0 - 0.5 * th / np.tan(0.5 * th)) / np.where(small, 1.0, th2))
    k1 = np.cross(om, t)
    return np.concatenate([t - 0.5 * k1 + c2 * np.cross(om, k1), om], axis=-1)


# ------------------------------------------------------------------ the problem
class IKCertificate:
    """The IK problem of one (robot, config, human height), from the Python-side objects only."""

    def __init__(self, robot, config, human_height=None):
        self.robot = robot
        self.config = config
        self.human_height = human_height
        self.planar = bool(robot.planar_base)
        if robot.jnt_type[0] != JNT_FREE:
            raise ValueError("the root body carries the base joint")
        # (robot body, human body, w_p, w_r) per task of a table that is switched on, zero-weight entries dropped
        self.tables = []
        for tab, on in ((config.table1, config.use_ik_match_table1), (config.table2, config.use_ik_match_table2)):
            self.tables.append([(robot.body_index(t.frame), t.human, float(t.pos_weight), float(t.rot_weight))
                                for t in tab if on and (t.pos_weight != 0 or t.rot_weight != 0)])
        # tangent space: (kind, index); the planar base has x, y and the turn about z only
        self.dofs = [("tx", 0), ("tx", 1)] + ([("rot", 2)] if self.planar else [("tx", 2), ("rot", 0), ("rot", 1), ("rot", 2)])
        self.dofs += [("hinge", int(b)) for b in range(robot.nbody) if robot.jnt_type[b] == JNT_HINGE]

    # -- kinematics ---------------------------------------------------
    def fk(self, qpos):
        """World position [..., nb, 3] and wxyz quaternion [..., nb, 4] of every body, for qpos [..., nq]
        (root position, root quaternion, hinge angles: the robot's own layout)."""
        r = self.robot
        qpos = np.asarray(qpos, dtype=np.float64)
        lead = qpos.shape[:-1]
        xpos = np.zeros(lead + (r.nbody, 3))
        xquat = np.zeros(lead + (r.nbody, 4))
        for b in range(r.nbody):
            p = int(r.parent[b])
            if p < 0:  # the base joint writes the root body's pose; the body's own pos / quat are its value at qpos0
                a = int(r.qpos_adr[b])
                xpos[..., b, :] = qpos[..., a:a + 3]
                xquat[..., b, :] = _unit(qpos[..., a + 3:a + 7])
                continue
            xpos[..., b, :] = xpos[..., p, :] + _qrot(xquat[..., p, :], r.body_pos[b])
            q = _qmul(xquat[..., p, :], np.broadcast_to(r.body_quat[b], lead + (4,)))
            if r.jnt_type[b] == JNT_HINGE:  # the hinge sits at the body's origin and turns it about its local axis
                half = 0.5 * qpos[..., int(r.qpos_adr[b])]
                q = _qmul(q, np.concatenate([np.cos(half)[..., None], np.sin(half)[..., None] * r.jnt_axis[b]], axis=-1))
            xquat[..., b, :] = _unit(q)
        return xpos, xquat

    # -- targets ------------------------------------------------------
    def prepare_targets(self, human_pos, human_quat, names, human_height=None):
        """One frame of human key-points (pos [B, 3], quat [B, 4] wxyz, names[B]) -> {human body: (target pos, target quat)}.

        The reference's update_targets: every body of the scale table keeps its offset from the human root times its scale
        (the table times actual height / assumed height), about the root's own position times the root's scale; then table 1's
        rotation offset is applied on the right and table 1's position offset (minus the ground height along z) is added in
        the turned frame.  Table 2's offsets are never used.
        """
        cfg = self.config
        height = self.human_height if human_height is None else human_height
        ratio = 1.0 if height is None else height / cfg.human_height_assumption
        col = {n: i for i, n in enumerate(names)}
        hp = np.asarray(human_pos, dtype=np.float64)
        hq = np.asarray(human_quat, dtype=np.float64)
        root = hp[col[cfg.human_root_name]]
        scaled_root = cfg.human_scale_table[cfg.human_root_name] * ratio * root
        offsets = {t.human: t for t in cfg.table1 if t.pos_weight != 0 or t.rot_weight != 0}
        out = {}
        for n, i in col.items():
            if n not in cfg.human_scale_table or n not in offsets:
                continue
            p = scaled_root if n == cfg.human_root_name else (hp[i] - root) * (cfg.human_scale_table[n] * ratio) + scaled_root
            off = offsets[n]
            q = _unit(_qmul(_unit(hq[i]), _unit(np.asarray(off.rot_offset, dtype=np.float64))))
            local = np.asarray(off.pos_offset, dtype=np.float64) - cfg.ground_height * np.array([0.0, 0.0, 1.0])
            out[n] = (p + _qrot(q, local), q)
        return out

    # -- cost ---------------------------------------------------------
    def task_errors(self, table, qpos, targets):
        """[..., ntask, 6] body-frame errors (e_pos, e_rot) of a table's tasks."""
        tasks = self.tables[table]
        xpos, xquat = self.fk(qpos)
        body = [b for b, _, _, _ in tasks]
        tp = np.array([targets[h][0] for _, h, _, _ in tasks])
        tq = np.array([targets[h][1] for _, h, _, _ in tasks])
        inv = _qconj(xquat[..., body, :])
        return se3_log(_unit(_qmul(inv, np.broadcast_to(tq, inv.shape))), _qrot(inv, tp - xpos[..., body, :]))

    def cost(self, table, qpos, targets, unit_weights=False):
        e = self.task_errors(table, qpos, targets)
        wp = np.array([1.0 if unit_weights else w for _, _, w, _ in self.tables[table]])
        wr = np.array([1.0 if unit_weights else w for _, _, _, w in self.tables[table]])
        return 0.5 * (np.sum(wp ** 2 * np.sum(e[..., :3] ** 2, axis=-1), axis=-1) + np.sum(wr ** 2 * np.sum(e[..., 3:] ** 2, axis=-1), axis=-1))

    # -- stationarity -------------------------------------------------
    def perturbed(self, qpos, step):
        """[ndof, nq]: qpos moved by `step` along every tangent direction -- root translation in the world frame, root
        rotation by exp of a body-frame vector on the right, hinges additively."""
        qpos = np.asarray(qpos, dtype=np.float64)
        out = np.repeat(qpos[None], len(self.dofs), axis=0)
        for k, (kind, i) in enumerate(self.dofs):
            if kind == "tx":
                out[k, i] += step
            elif kind == "rot":
                w = np.zeros(3)
                w[i] = step
                out[k, 3:7] = _unit(_qmul(qpos[3:7], _qexp(w)))
            else:
                out[k, int(self.robot.qpos_adr[i])] += step
        return out

    def gradient(self, table, qpos, targets):
        """Central-difference gradient of `cost` over the tangent space (step FD_STEP), one entry per `self.dofs`."""
        both = np.concatenate([self.perturbed(qpos, FD_STEP), self.perturbed(qpos, -FD_STEP)])
        c = self.cost(table, both, targets)
        n = len(self.dofs)
        return (c[:n] - c[n:]) / (2.0 * FD_STEP)

    def bound_state(self, qpos):
        """Per dof: -1 on the lower bound, +1 on the upper bound (within ACTIVE_TOL), 0 otherwise; and whether every limited
        hinge is inside its range (again within ACTIVE_TOL)."""
        r = self.robot
        state = np.zeros(len(self.dofs), dtype=np.int64)
        feasible = True
        for k, (kind, b) in enumerate(self.dofs):
            if kind != "hinge" or not r.jnt_limited[b]:
                continue
            q, (lo, hi) = float(qpos[int(r.qpos_adr[b])]), r.jnt_range[b]
            feasible &= lo - ACTIVE_TOL <= q <= hi + ACTIVE_TOL
            state[k] = -1 if q <= lo + ACTIVE_TOL else (1 if q >= hi - ACTIVE_TOL else 0)
        return state, bool(feasible)

    def projected_gradient(self, table, qpos, targets):
        """The gradient with the components a joint limit explains set to zero.  With d = -g the descent direction: on a lower
        bound d < 0 is allowed (the cost falls only where the joint cannot go), on an upper bound d > 0; such components are
        zeroed, an active component of the other sign is kept -- the solver could have moved off the bound and did not.
        A qpos outside a range is no solution of the problem at all: every component is +inf."""
        g = self.gradient(table, qpos, targets)
        state, feasible = self.bound_state(qpos)
        if not feasible:
            return np.full_like(g, np.inf)
        d = -g
        explained = ((state < 0) & (d < 0.0)) | ((state > 0) & (d > 0.0))
        return np.where(explained, 0.0, g)

    def stationarity(self, table, q_final, q_init, targets):
        """The certified quantity: |projected gradient at q_final|_inf / |gradient at q_init|_inf."""
        return float(np.abs(self.projected_gradient(table, q_final, targets)).max() / np.abs(self.gradient(table, q_init, targets)).max())

    def used_tables(self):
        return [k for k in (0, 1) if self.tables[k]]


# ------------------------------------------------------------------ thresholds
# ORACLE_WORST: what the CPU oracle (oracle/gmr_oracle.c) reaches on the cases of tests/ik_certificate_cases.py, the worst over
# the cases of a family -- measured by tests/test_ik_certificate_host.py (it prints every value; run it with -s), 2026-10, x86-64,
# and rounded up to two digits.  The HIP kernel is held to 10 x these: it agrees with the oracle to <= 1e-6 rad, and that
# difference pushed through the local curvature may cost it up to that factor; nothing here was measured on the kernel.
#   stat_last : |projected gradient(q_final)|_inf / |gradient(qpos0)|_inf for the table of the frame's last stage
#   stat_other: the same for the other table (reachable cases only: float32 key-points make the targets consistent between
#               the tables to ~1e-7, and the tables weigh that inconsistency differently)
#   cost      : cost(q_final) / cost(qpos0), any table (reachable cases only)
ORACLE_WORST = {
    # (a), ten robots x two clips, 40 held frames of 2 x 51 solves: q_final is within a few ulp of the minimiser
    "reachable": {"stat_last": 7.9e-16, "stat_other": 5.9e-8, "cost": 1.3e-15},
    # (a) with tol = 1e-3, max_iter = 10 (unitree_g1 with and without hands), 200 held frames of 2 solves
    "reachable_default": {"stat_last": 6.0e-12, "stat_other": 4.9e-9, "cost": 4.5e-16},
    # (b), the held reference frame (3 frames of 2 x 3001 solves: 3.3e-12) and the synthetic robot (1.4e-12); both sit on the
    # rounding floor of the central difference, eps * cost / FD_STEP / |gradient(qpos0)| ~ 2e-12
    "limits": {"stat_last": 3.3e-12},
}
GPU_FACTOR = 10.0


def thresholds(family, tables):
    """{'stat<k>' / 'cost<k>': bound} for the certified tables of a case of `family`."""
    worst = ORACLE_WORST[family]
    out = {}
    for k in tables:
        out[f"stat{k}"] = GPU_FACTOR * worst["stat_last" if k == tables[-1] else "stat_other"]
        if "cost" in worst:
            out[f"cost{k}"] = GPU_FACTOR * worst["cost"]
    return out

"""The contract of gmr_motion_sample (include/gmr_amd.h), restated in numpy: the plan, the pose, the stencils of the generalized
velocity, and the chain that carries poses and twists down the tree with an explicit parent loop.  Nothing of the library under
test is used but the parsed robot (``compiled(...).robot``).

``chain(..., dtype=np.float64)`` is the definition evaluated in double; ``chain(..., dtype=np.float32)`` is the same loop with every
operation in float32, in the operand order the contract fixes -- the yardstick of the body velocities (the kernel differs from it
only where its sin / cos and its float64 hinge normalisation round differently).  The tree constants are the ones the library
holds: local translations and raw local rotations rounded to float32, the unit hinge axis in float64 (rounded to float32 for the
twist)."""
import numpy as np

_GEN = ("root_pos", "root_rot", "joint_pos", "root_lin_vel", "root_ang_vel", "joint_vel")
_BODY = ("body_pos_w", "body_quat_w", "body_lin_vel_w", "body_ang_vel_w")


class Tree:
    """The constants of the chain.  ``unit=True`` replaces the raw local rotations (the XML's values, |q|^2 - 1 up to 7e-7, which
    gmr_fk uses as they are) by their float64 normalisation: a rigid tree, for checking the twist formula against a derivative."""

    def __init__(self, robot, unit=False):
        nb = robot.nbody
        self.nb, self.nd = nb, robot.nq - 7
        self.parent = np.asarray(robot.parent, dtype=np.int64)
        self.lpos = np.asarray(robot.body_pos, dtype=np.float64).astype(np.float32)
        self.lrot = np.asarray(robot.body_quat_raw, dtype=np.float64)[:, [1, 2, 3, 0]].astype(np.float32)  # xyzw
        if unit:
            lr = np.asarray(robot.body_quat_raw, dtype=np.float64)[:, [1, 2, 3, 0]]
            self.lrot = lr / np.linalg.norm(lr, axis=1, keepdims=True)
        self.axis = np.asarray(robot.jnt_axis, dtype=np.float64)
        hinge = set(int(b) for b in robot.hinge_bodies())
        self.dof = np.array([int(robot.qpos_adr[b]) - 7 if b in hinge else -1 for b in range(nb)], dtype=np.int64)
        assert self.parent[0] == -1 and all(0 <= self.parent[b] < b for b in range(1, nb))


# ------------------------------------------------------------------ the plan
def plan(offs, fps, ids, times, k_per_id=1):
    """Per query: valid, the global rows (km0, i0, i1, kp1, km1), the weight a and the steps h0, h1 (python loop: the definition)."""
    offs = np.asarray(offs, dtype=np.int64)
    fps = np.asarray(fps, dtype=np.float64)
    times = np.asarray(times).reshape(-1)
    Q = times.size
    valid = np.zeros(Q, dtype=bool)
    rows = np.zeros((Q, 5), dtype=np.int64)
    a, h0, h1 = np.zeros(Q), np.zeros(Q), np.zeros(Q)
    for j in range(Q):
        s, t = int(ids[j // k_per_id]), np.float64(times[j])  # (a float32 time is promoted first)
        if s < 0 or s >= len(offs) - 1 or not np.isfinite(t):
            continue
        T, f = int(offs[s + 1] - offs[s]), fps[s]
        if T == 0:
            continue
        u = t * f
        if u <= 0:
            i0 = 0
        elif u >= T - 1:
            i0 = T - 1
        else:
            i0 = int(np.floor(u))
        i1 = min(i0 + 1, T - 1)
        a[j] = u - i0 if (i1 > i0 and 0 < u) else 0.0
        km0, kp0 = max(i0 - 1, 0), min(i0 + 1, T - 1)
        km1, kp1 = max(i1 - 1, 0), min(i1 + 1, T - 1)
        h0[j] = np.float64(kp0 - km0) * (1.0 / f)
        h1[j] = np.float64(kp1 - km1) * (1.0 / f)
        rows[j] = offs[s] + np.array([km0, i0, i1, kp1, km1])
        assert kp0 == i1
        valid[j] = True
    return valid, rows, a, h0, h1


def lerp(x0, x1, a):
    a = a.reshape((-1,) + (1,) * (x0.ndim - 1))
    with np.errstate(invalid="ignore"):
        return np.where(a == 0, x0, x0 + a * (x1 - x0))


def slerp(q0, q1, a):
    """The export's shortest-arc slerp (xyzw); a copy of q0 when a = 0 or q0 == q1."""
    with np.errstate(invalid="ignore", divide="ignore"):
        d = q0[:, 0] * q1[:, 0] + q0[:, 1] * q1[:, 1] + q0[:, 2] * q1[:, 2] + q0[:, 3] * q1[:, 3]
        neg = d < 0
        q1 = np.where(neg[:, None], -q1, q1)
        d = np.where(neg, -d, d)
        om = np.arccos(np.where(d < 1.0, d, 1.0))  # fmin(d, 1): 1 for a NaN d
        small = om < 1e-8
        so = np.sin(om)
        w0 = np.where(small, 1.0 - a, np.sin((1.0 - a) * om) / so)
        w1 = np.where(small, a, np.sin(a * om) / so)
        r = w0[:, None] * q0 + w1[:, None] * q1
        n = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
        r = r / n[:, None]
    copy = (a == 0) | np.all(q0 == q1, axis=1)
    return np.where(copy[:, None], q0, r)


def ang_vel(p, q, h):
    """rotvec(p (x) conj(q)) / h for xyzw quaternions [n, 4]; 0 where h = 0."""
    with np.errstate(invalid="ignore", divide="ignore"):
        pv, pw, qv, qw = p[:, :3], p[:, 3:], q[:, :3], q[:, 3:]
        w = pw * qw + (pv[:, 0:1] * qv[:, 0:1] + pv[:, 1:2] * qv[:, 1:2] + pv[:, 2:3] * qv[:, 2:3])
        v = qw * pv - pw * qv - np.cross(pv, qv)
        neg = w < 0
        w, v = np.where(neg, -w, w), np.where(neg, -v, v)
        n = np.sqrt(v[:, 0:1] * v[:, 0:1] + v[:, 1:2] * v[:, 1:2] + v[:, 2:3] * v[:, 2:3])
        f = np.where(n > 1e-12, 2.0 * np.arctan2(n, w) / n, 2.0)
        out = v * f / h[:, None]
    return np.where(h[:, None] == 0, 0.0, out)


def generalized(qpos, offs, fps, ids, times, k_per_id=1):
    """The six float64 generalized arrays of every query (NaN rows for an invalid one) and the plan."""
    qpos = np.asarray(qpos, dtype=np.float64)
    valid, rows, a, h0, h1 = plan(offs, fps, ids, times, k_per_id)
    if qpos.shape[0] == 0:
        qpos = np.zeros((1, qpos.shape[1]))
    xm0, x0, x1, xp1, xm1 = (qpos[rows[:, k]] for k in range(5))
    xyzw = [4, 5, 6, 3]
    lin = [0, 1, 2] + list(range(7, qpos.shape[1]))
    with np.errstate(invalid="ignore", divide="ignore"):
        v0 = np.where(h0[:, None] == 0, 0.0, (x1[:, lin] - xm0[:, lin]) / h0[:, None])
        v1 = np.where(h1[:, None] == 0, 0.0, (xp1[:, lin] - xm1[:, lin]) / h1[:, None])
    pos = lerp(x0[:, lin], x1[:, lin], a)
    vel = lerp(v0, v1, a)
    w0 = ang_vel(x1[:, xyzw], xm0[:, xyzw], h0)
    w1 = ang_vel(xp1[:, xyzw], xm1[:, xyzw], h1)
    out = {"root_pos": pos[:, :3], "joint_pos": pos[:, 3:], "root_rot": slerp(x0[:, xyzw], x1[:, xyzw], a),
           "root_lin_vel": vel[:, :3], "joint_vel": vel[:, 3:], "root_ang_vel": lerp(w0, w1, a)}
    for k in out:
        out[k] = np.where(valid[:, None], out[k], np.nan)
    return out, (valid, rows, a, h0, h1)


# ------------------------------------------------------------------ the chain (gmr_fk's formulas, in `dtype`)
def quat_mul(a, b):
    x1, y1, z1, w1 = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    x2, y2, z2, w2 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    half = a.dtype.type(0.5)
    ww = (z1 + x1) * (x2 + y2)
    yy = (w1 - y1) * (w2 + z2)
    zz = (w1 + y1) * (w2 - z2)
    xx = ww + yy + zz
    qq = half * (xx + (z1 - x1) * (x2 - y2))
    w = qq - ww + (z1 - y1) * (y2 - z2)
    x = qq - xx + (x1 + w1) * (x2 + w2)
    y = qq - yy + (w1 - x1) * (y2 + z2)
    z = qq - zz + (z1 + y1) * (w2 - x2)
    return np.stack([x, y, z, w], axis=-1)


def quat_rotate(q, v):
    """v (2 w^2 - 1) + (q_v x v) w 2 + q_v (q_v . v) 2, in gmr_fk's operand order."""
    two, one = q.dtype.type(2.0), q.dtype.type(1.0)
    w = q[..., 3]
    k = two * w * w - one
    cx = q[..., 1] * v[..., 2] - q[..., 2] * v[..., 1]
    cy = q[..., 2] * v[..., 0] - q[..., 0] * v[..., 2]
    cz = q[..., 0] * v[..., 1] - q[..., 1] * v[..., 0]
    d = q[..., 0] * v[..., 0] + q[..., 1] * v[..., 1] + q[..., 2] * v[..., 2]
    return np.stack([v[..., 0] * k + cx * w * two + q[..., 0] * d * two,
                     v[..., 1] * k + cy * w * two + q[..., 1] * d * two,
                     v[..., 2] * k + cz * w * two + q[..., 2] * d * two], axis=-1)


def hinge_quat(axis64, ang, dtype):
    """axis_angle_to_quat: sin / cos of the half angle in `dtype`, the product with the float64 axis and the renormalisation in
    float64, the result rounded to `dtype`."""
    th = ang / dtype(2.0)
    s, c = np.sin(th).astype(np.float64), np.cos(th).astype(np.float64)
    q = np.stack([axis64[0] * s, axis64[1] * s, axis64[2] * s, c], axis=-1)
    n = np.sqrt(np.sum(q * q, axis=-1, keepdims=True))
    return (q / np.maximum(n, 1e-9)).astype(dtype)


def chain(tree, gen, dtype=np.float64):
    """Poses and twists of every body, [Q, nbody, ...] in `dtype`, from the float64 generalized arrays `gen` cast to `dtype`."""
    dtype = np.dtype(dtype).type
    c = lambda x: np.asarray(x, dtype=np.float64).astype(dtype)
    rp, rr, jp = c(gen["root_pos"]), c(gen["root_rot"]), c(gen["joint_pos"])
    rv, rw, jv = c(gen["root_lin_vel"]), c(gen["root_ang_vel"]), c(gen["joint_vel"])
    Q, nb = rp.shape[0], tree.nb
    X, R = np.zeros((Q, nb, 3), dtype=dtype), np.zeros((Q, nb, 4), dtype=dtype)
    V, W = np.zeros((Q, nb, 3), dtype=dtype), np.zeros((Q, nb, 3), dtype=dtype)
    X[:, 0], R[:, 0], V[:, 0], W[:, 0] = rp, rr, rv, rw
    with np.errstate(invalid="ignore"):
        for j in range(1, nb):  # the explicit parent loop
            p = int(tree.parent[j])
            lt, lr = np.broadcast_to(tree.lpos[j].astype(dtype), (Q, 3)), np.broadcast_to(tree.lrot[j].astype(dtype), (Q, 4))
            di = int(tree.dof[j])
            jq = np.broadcast_to(np.array([0, 0, 0, 1], dtype=dtype), (Q, 4))
            if di >= 0:
                jq = hinge_quat(tree.axis[j], jp[:, di], dtype)
            X[:, j] = X[:, p] + quat_rotate(R[:, p], lt)
            R[:, j] = quat_mul(R[:, p], quat_mul(lr, jq))
            d = X[:, j] - X[:, p]
            wp = W[:, p]
            cross = np.stack([wp[:, 1] * d[:, 2] - wp[:, 2] * d[:, 1], wp[:, 2] * d[:, 0] - wp[:, 0] * d[:, 2],
                              wp[:, 0] * d[:, 1] - wp[:, 1] * d[:, 0]], axis=-1)
            V[:, j] = V[:, p] + cross
            if di >= 0:
                ax = np.broadcast_to(tree.axis[j].astype(np.float32).astype(dtype), (Q, 3))
                W[:, j] = wp + quat_rotate(R[:, j], ax) * jv[:, di:di + 1]
            else:
                W[:, j] = wp
    return {"body_pos_w": X, "body_quat_w": R, "body_lin_vel_w": V, "body_ang_vel_w": W}


def sample(tree, qpos, offs, fps, ids, times, k_per_id=1, dtype=np.float64):
    """All ten arrays of every query: the generalized ones in float64, the body ones through `chain` in `dtype`."""
    gen, pl = generalized(qpos, offs, fps, ids, times, k_per_id)
    out = dict(gen)
    out.update(chain(tree, gen, dtype))
    return out, pl

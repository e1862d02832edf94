"""Rotation edge cases: a 50-digit reference without thresholds, and deterministic case tables.

Every other comparison of the suite draws its rotations from random walks, which land on the branch thresholds of the device's
hand-written rotation math with probability zero, and compares with float64 numpy that has thresholds of its own.  This module
holds (1) the same operations written ONCE over an abstract number type and evaluated with mpmath at 50 digits (`MP`) -- and, for
the plain-float measurement of tests/test_rotation_edges_host.py, with numpy float64 / float32 scalars (`F64`, `F32`) --, and
(2) the tables of inputs that sit on those thresholds.  No GPU and no native code is touched here.

Inputs are the exact binary values of the arrays a kernel receives (`mpf(float(x))`); results are rounded once, at the end.

The reference has NO threshold that exists to avoid 0/0: a removable singularity is handled by its analytic limit AT the singular
point only (`a == 0`, `n == 0`, `d >= 1`).  What it does have are the reference project's DEFINITIONAL discontinuities, which are
semantics and not approximations:
  * smpl.py:93-95   the SMPL-X adapter's slerp blends linearly, q1 + t (q2 - q1), above dot 0.9995 (and normalises: R.from_quat)
  * smpl.py:88-91   ... on the sign-aligned pair (dot < 0 negates q2)
  * smpl.py:157-160 the interpolated rotation is stored as a rotation vector and read back: the quaternion gets w >= 0
  * torch_utils.py:321-340 (Joint.rot_to_dof, kinematics_model.py:38-53)  w made non-negative, angle 0 at |xyz| <= 1e-5, the sign
    from the joint axis; kinematics_model.py:184-197 clamps to the joint range
Quaternions are wxyz tuples unless a name says xyzw.
"""
import functools

import mpmath
import numpy as np

mp = mpmath.MPContext()   # a context of this module's own: the precision of mpmath's global one (sympy, other tests) is left alone
mp.dps = 50
mpf = mp.mpf

EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)
GPU_FACTOR = 10.0   # a kernel may deviate from the 50-digit reference by this many times what plain numpy does (FLOAT_WORST)
FLOOR_EPS = 8.0     # ... but never has to be closer than this many epsilons of the output's magnitude

# Worst |plain numpy - reference| per family and output over the family's whole table, measured by
# tests/test_rotation_edges_host.py::test_plain_float_worst (it prints every value with -s; x86-64, numpy float64, float32 for the
# kin-ops family) and rounded up to one digit (head-room for another libm).  The test recomputes them and fails if one of these is smaller than what it
# measures.  Nothing here was measured on a kernel.
FLOAT_WORST = {
    "smplx_chain3": {"quat": 6e-14},
    "smplx_small_chain3": {"quat": 3e-16},   # the angle grid up to 0.5 rad only: the series and its threshold without the 1000 rad rows
    "smplx_tree55": {"quat": 2e-13},
    "smplx_resample_chain3": {"quat": 2e-15},
    "smplx_resample_tree55": {"quat": 5e-15},
    "bvh_chain3": {"quat": 9e-15, "pos": 3e-15},
    "bvh_tree33": {"quat": 4e-14, "pos": 2e-13},
    "dof_to_rot": {"quat": 7e-8},
    "rot_to_dof": {"dof": 3e-7},
    "track": {"root_rot": 2e-16, "root_ang_vel": 3e-14},
    "evaluate_unitree_g1": {"task_err": 2e-15, "xpos": 5e-16, "xquat": 6e-16},
    "evaluate_galaxea_r1pro": {"task_err": 9e-16, "xpos": 5e-16, "xquat": 3e-16},
}


def bound(family, output, magnitude, eps=EPS64):
    """The largest admissible |kernel - reference| for an output of this magnitude."""
    return np.maximum(GPU_FACTOR * FLOAT_WORST[family][output], FLOOR_EPS * eps * np.abs(magnitude))


# ------------------------------------------------------------------ number types
class _Num:
    def __init__(self, name, c, sin, cos, sqrt, atan2, acos, rad, out):
        self.name, self.c, self.sin, self.cos, self.sqrt, self.atan2, self.acos, self.rad, self.out = name, c, sin, cos, sqrt, atan2, acos, rad, out

    def vec(self, xs):
        return tuple(self.c(x) for x in xs)


MP = _Num("mp", lambda x: mpf(float(x)), mp.sin, mp.cos, mp.sqrt, mp.atan2, mp.acos, lambda x: x * mp.pi / 180, float)
F64 = _Num("f64", np.float64, np.sin, np.cos, np.sqrt, np.arctan2, np.arccos, np.radians, float)
F32 = _Num("f32", np.float32, np.sin, np.cos, np.sqrt, np.arctan2, np.arccos, np.radians, float)


# ------------------------------------------------------------------ the operations, over any number type B
def qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return (aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
            aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw)


def qconj(a):
    return (a[0], -a[1], -a[2], -a[3])


def qneg(a):
    return (-a[0], -a[1], -a[2], -a[3])


def dot(a, b):
    s = a[0] * b[0]
    for x, y in zip(a[1:], b[1:]):
        s = s + x * y
    return s


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def qrot(B, q, v):
    """v turned by the unit quaternion q: v + 2 w (u x v) + 2 u x (u x v)."""
    u = q[1:]
    t = tuple(B.c(2) * x for x in cross(u, v))
    c = cross(u, t)
    return tuple(v[i] + q[0] * t[i] + c[i] for i in range(3))


def qnormalise(B, q):
    n = B.sqrt(dot(q, q))
    return tuple(x / n for x in q)


def qexp(B, v):
    """exp of a rotation vector: (cos(a/2), sin(a/2)/a v), the limit 1/2 v taken AT a = 0 only."""
    a = B.sqrt(dot(v, v))
    half = B.c(0.5)
    k = half if a == 0 else B.sin(a * half) / a
    return (B.cos(a * half), k * v[0], k * v[1], k * v[2])


def qlog(B, q):
    """Rotation vector of a unit quaternion on the short side (angle in [0, pi]); w = 0 is left as it is (angle pi)."""
    if q[0] < 0:
        q = qneg(q)
    n = B.sqrt(dot(q[1:], q[1:]))
    if n == 0:
        return (n, n, n)
    f = B.c(2) * B.atan2(n, q[0]) / n
    return (f * q[1], f * q[2], f * q[3])


def vinv_t(B, om, t):
    """V(omega)^-1 t = t - 1/2 omega x t + (1 - (th/2) cot(th/2)) / th^2  omega x (omega x t), the limit t AT omega = 0 only."""
    th2 = dot(om, om)
    if th2 == 0:
        return tuple(t)
    th, half = B.sqrt(th2), B.c(0.5)
    c2 = (B.c(1) - half * th * B.cos(half * th) / B.sin(half * th)) / th2
    k1 = cross(om, t)
    k2 = cross(om, k1)
    return tuple(t[i] - half * k1[i] + c2 * k2[i] for i in range(3))


def slerp_weights(B, d, a):
    """Textbook slerp weights sin((1-a) th)/sin th, sin(a th)/sin th for cos th = d in [0, 1]; the limit (1-a, a) AT th = 0 only."""
    one = B.c(1)
    if d >= one:
        return one - a, a
    th = B.acos(d)
    s = B.sin(th)
    return B.sin((one - a) * th) / s, B.sin(a * th) / s


def slerp(B, q0, q1, a):
    """Shortest-arc slerp of two unit quaternions, normalised (the tracking export's contract in include/gmr_amd.h)."""
    d = dot(q0, q1)
    if d < 0:
        q1, d = qneg(q1), -d
    w0, w1 = slerp_weights(B, d, a)
    return qnormalise(B, tuple(w0 * x + w1 * y for x, y in zip(q0, q1)))


def smplx_slerp(B, q0, q1, a):
    """smpl.py:75-107 and :157-160: sign-aligned pair; DEFINITIONAL linear blend above dot 0.9995; normalised; then w >= 0."""
    d = dot(q0, q1)
    if d < 0:
        q1, d = qneg(q1), -d
    if d > B.c(0.9995):
        q = tuple(x + a * (y - x) for x, y in zip(q0, q1))
    else:
        w0, w1 = slerp_weights(B, d, a)
        q = tuple(w0 * x + w1 * y for x, y in zip(q0, q1))
    q = qnormalise(B, q)
    return qneg(q) if q[0] < 0 else q


def axis_quat(B, ang, axis):
    h = ang * B.c(0.5)
    q = [B.cos(h), B.c(0), B.c(0), B.c(0)]
    q[1 + axis] = B.sin(h)
    return tuple(q)


def euler_quat(B, e, order):
    """lafan_vendor/utils.py:56-75: q(e0, axis o0) (x) (q(e1, o1) (x) q(e2, o2)), angles in radians."""
    return qmul(axis_quat(B, e[0], order[0]), qmul(axis_quat(B, e[1], order[1]), axis_quat(B, e[2], order[2])))


# ------------------------------------------------------------------ families: the whole operation of a kernel on arrays
@functools.lru_cache(maxsize=None)
def _qmul_memo(number_type, a, b):   # (keyed by the number type: mpf and float64 tuples of equal value hash alike)
    return qmul(a, b)


def smplx_quats(B, go, fp, parents, T_out=None):
    """Global joint orientations [T', J, 4] wxyz (float64) of gmr_smplx_keypoints: rotation vectors go [T, 3] (joint 0) and
    fp [T, J, 3] chained down `parents`; with T_out the frames are first resampled at np.linspace(0, T-1, T_out) by smplx_slerp."""
    T, J = fp.shape[:2]

    @functools.lru_cache(maxsize=None)
    def ex(x, y, z):
        return qexp(B, B.vec((x, y, z)))

    def local(i, j):
        r = go[i] if j == 0 else fp[i, j]
        return ex(float(r[0]), float(r[1]), float(r[2]))

    @functools.lru_cache(maxsize=None)
    def blend(r1, r2, a):
        return smplx_slerp(B, ex(*r1), ex(*r2), B.c(a))

    n = T if T_out is None else T_out
    out = np.zeros((n, J, 4))
    for k in range(n):
        if T_out is None:
            lq = [local(k, j) for j in range(J)]
        else:
            t = float(T - 1) if k == T_out - 1 and T_out > 1 else k * (float(T - 1) / float(T_out - 1) if T_out > 1 else 0.0)
            i1 = min(int(np.floor(t)), T - 1)
            i2 = min(i1 + 1, T - 1)
            a = t - i1
            rv = lambda i, j: tuple(float(x) for x in (go[i] if j == 0 else fp[i, j]))  # noqa: E731
            lq = [blend(rv(i1, j), rv(i2, j), a) for j in range(J)]
        g = []
        for j in range(J):
            g.append(lq[j] if parents[j] < 0 else _qmul_memo(B.name, g[parents[j]], lq[j]))
            out[k, j] = [B.out(x) for x in g[j]]
    return out


def bvh_fk(B, parents, order, lpos, eul_deg, scale):
    """gmr_bvh_fk_rows: Euler channels in degrees -> local quaternions, FK in hierarchy order (lafan_vendor/utils.py:88-103), the
    +90 degree turn about x and the scale (lafan1.py:20-21,31-32).  Returns pos [T, J, 3], quat [T, J, 4] wxyz as float64."""
    T, J = eul_deg.shape[:2]
    h = B.sqrt(B.c(0.5))
    rq = (h, h, B.c(0), B.c(0))
    sc = B.c(scale)

    @functools.lru_cache(maxsize=None)
    def local(x, y, z):
        return euler_quat(B, tuple(B.rad(B.c(v)) for v in (x, y, z)), order)

    pos, quat = np.zeros((T, J, 3)), np.zeros((T, J, 4))
    for f in range(T):
        gq, gp = [], []
        for j in range(J):
            lq = local(*(float(v) for v in eul_deg[f, j]))
            lp = B.vec(lpos[f, j])
            p = parents[j]
            if p < 0:
                gq.append(lq)
                gp.append(lp)
            else:
                r = qrot(B, gq[p], lp)
                gq.append(qmul(gq[p], lq))
                gp.append(tuple(r[i] + gp[p][i] for i in range(3)))
            quat[f, j] = [B.out(x) for x in qmul(rq, gq[j])]
            pos[f, j] = [B.out(gp[j][0] * sc), B.out(-gp[j][2] * sc), B.out(gp[j][1] * sc)]
    return pos, quat


def dof_to_rot(B, axes, dof_body, nbody, dof):
    """gmr_dof_to_rot (include/gmr_amd.h; Joint.dof_to_rot, torch_utils.axis_angle_to_quat): [T, ndof] -> [T, nbody-1, 4] xyzw,
    (axis sin(th/2), cos(th/2)) with the axis normalised, the identity for bodies without a hinge."""
    T = dof.shape[0]
    out = np.zeros((T, nbody - 1, 4))
    out[..., 3] = 1.0
    unit = []
    for ax in axes:
        a = B.vec(ax)
        n = B.sqrt(dot(a, a))
        unit.append(tuple(x / n for x in a))

    @functools.lru_cache(maxsize=None)
    def sc(th):
        h = B.c(th) * B.c(0.5)
        return B.sin(h), B.cos(h)

    for f in range(T):
        for d, b in enumerate(dof_body):
            s, c = sc(float(dof[f, d]))
            q = qnormalise(B, (unit[d][0] * s, unit[d][1] * s, unit[d][2] * s, c))
            out[f, b - 1] = [B.out(x) for x in q]
    return out


ROT_TO_DOF_EPS = float(np.float32(1e-5))  # torch_utils.py:322, compared in float32


def rot_to_dof_one(B, q_xyzw, axis, lo, hi):
    """Joint.rot_to_dof on one quaternion (xyzw): the DEFINITIONAL parts are w made non-negative (quat_pos), angle 0 and axis z at
    |xyz| <= 1e-5, the sign from the joint axis and the clamp to [lo, hi]."""
    x, y, z, w = q_xyzw
    if w < 0:
        x, y, z, w = -x, -y, -z, -w
    n = B.sqrt(x * x + y * y + z * z)
    if not n > B.c(ROT_TO_DOF_EPS):
        return min(max(B.c(0), B.c(lo)), B.c(hi))
    ang = B.c(2) * B.atan2(n, w)
    if (x * axis[0] + y * axis[1] + z * axis[2]) / n < 0:
        ang = -ang
    return min(max(ang, B.c(lo)), B.c(hi))


def rot_to_dof(B, axes, dof_body, lo, hi, rot):
    """gmr_rot_to_dof: [T, nbody-1, 4] xyzw float32 -> [T, ndof]."""
    T = rot.shape[0]
    out = np.zeros((T, len(dof_body)))
    for d, b in enumerate(dof_body):
        ax = B.vec(axes[d])
        for f in range(T):
            out[f, d] = B.out(rot_to_dof_one(B, B.vec(rot[f, b - 1]), ax, lo[d], hi[d]))
    return out


def track_root_rot(B, q0_xyzw, q1_xyzw, a):
    """One resampled root quaternion (xyzw) of gmr_motion_track: a = 0 or two identical rows copy the row (include/gmr_amd.h), else
    shortest-arc slerp, normalised."""
    if a == 0 or all(float(x) == float(y) for x, y in zip(q0_xyzw, q1_xyzw)):   # the contract: copies, bit for bit
        return tuple(float(x) for x in q0_xyzw)
    r = slerp(B, B.vec(np.roll(q0_xyzw, 1)), B.vec(np.roll(q1_xyzw, 1)), B.c(a))
    return (B.out(r[1]), B.out(r[2]), B.out(r[3]), B.out(r[0]))


def track_ang_vel(B, p_xyzw, q_xyzw, h):
    """log(p (x) conj(q)) / h for xyzw rows: the world-frame angular velocity that turns q into p in time h."""
    om = qlog(B, qmul(B.vec(np.roll(p_xyzw, 1)), qconj(B.vec(np.roll(q_xyzw, 1)))))
    return tuple(B.out(x / B.c(h)) for x in om)


# ------------------------------------------------------------------ case tables
def _nbrs(x, dtype=np.float64):
    x = dtype(x)
    return [np.nextafter(x, dtype(-np.inf)), x, np.nextafter(x, dtype(np.inf))]


OBLIQUE = np.array([2.0, -3.0, 6.0]) / 7.0   # an exactly representable direction of unit length (to rounding)
AXES = [np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0]), OBLIQUE]


def angle_grid(dtype=np.float64):
    """The angles of a single rotation [rad]: zeros, denormal-range and tiny values, the series threshold 1e-3 of from_rotvec and
    its neighbours, the half-angle threshold 1.6 of the sincos kernels (angle 3.2) and its neighbours, pi and 2 pi and their
    surroundings, and angles several turns out."""
    g = [0.0, -0.0, 1e-300, -1e-300, 1e-12, -1e-12, 1e-9, -1e-9]
    g += [float(v) for v in _nbrs(1e-3, dtype)] + [-float(v) for v in _nbrs(1e-3, dtype)]
    g += [0.5, np.pi / 2]
    g += [float(v) for v in _nbrs(3.2, dtype)]
    g += [np.pi - 1e-9, np.pi, np.pi + 1e-9, 2 * np.pi - 1e-9, 2 * np.pi, 2 * np.pi + 1e-9, 7.0, 50.0, 1000.0]
    return np.array(g, dtype=dtype)


def angle_branches(a):
    """(series arm of rotvec_to_quat: a <= 1e-3, short sincos kernel: a/2 <= 1.6) that the exact |angle| asks for."""
    a = abs(mpf(float(a)))
    return bool(a <= mpf(1e-3)), bool(a / 2 <= mpf(1.6))


DOT_EDGE = 0.9995
# separations [rad] of the pair grid.  dot = cos(sep / 2): the four values around DOT_EDGE put dot at 0.9995 (1 +- 1e-9) and
# 0.9995 (1 +- 1e-3); "linear" names the side of the SMPL-X adapter's definitional blend the pair is built for
PAIR_SEPS = [("same", 0.0, True), ("1e-9", 1e-9, True), ("4e-12", 4e-12, True), ("2e-8", 2e-8, True), ("4e-8", 4e-8, True),
             ("1e-4", 1e-4, True), ("0.0316", 0.0316, True)]
# (0.9995 (1 + 1e-3) > 1 is no dot of unit quaternions: above the edge the grid has 1 + 1e-9, 1 + 1e-4 and dot = 1, which is 1 + 5e-4)
for _name, _rel in (("dot+1e-9", 1e-9), ("dot+1e-4", 1e-4)):
    PAIR_SEPS.append((_name, float(2 * mp.acos(mpf(DOT_EDGE) * (1 + mpf(_rel)))), True))
for _name, _rel in (("dot-1e-9", 1e-9), ("dot-1e-3", 1e-3)):
    PAIR_SEPS.append((_name, float(2 * mp.acos(mpf(DOT_EDGE) * (1 - mpf(_rel)))), False))
PAIR_SEPS += [("1", 1.0, False), ("halfpi", np.pi / 2, False), ("pi-1e-6", np.pi - 1e-6, False), ("pi", np.pi, False)]
WEIGHTS = [0.0, 2.0 ** -20, 0.25, 0.5, 0.75, 1.0 - 2.0 ** -20]


def rotvec_pairs():
    """[(name, r0, r1, linear)]: rotation vectors about OBLIQUE whose quaternions are `sep` apart, and the same with r1 one full
    turn further (its quaternion negated).  The pair exactly pi apart starts from the zero vector about x, so that its dot,
    cos(fl(pi) / 2) = 6.1e-17, is one correctly signed number and not a cancelling sum."""
    out = []
    for name, sep, lin in PAIR_SEPS:
        for neg in (False, True):
            turn = 2 * np.pi if neg else 0.0
            if name == "pi":
                r0, r1 = np.zeros(3), np.array([sep + turn, 0.0, 0.0])
            else:
                r0, r1 = 0.4 * OBLIQUE, (0.4 + sep + turn) * OBLIQUE
            out.append((name + ("/neg" if neg else ""), r0, r1, lin))
    return out


def quat_pairs():
    """[(name, q0, q1)] wxyz float64 unit quaternions `sep` apart (q1 = q0 (x) exp(sep z), rounded once), each also with q1 negated;
    q1 = -q0 exactly; and for pi a pair whose dot is exactly 0 in any arithmetic."""
    q0 = qexp(MP, MP.vec(0.7 * OBLIQUE))
    q0f = np.array([float(x) for x in q0])
    out = []
    for name, sep, _ in PAIR_SEPS:
        if name == "pi":
            a, b = np.array([0.8, 0.6, 0.0, 0.0]), np.array([-0.6, 0.8, 0.0, 0.0])
        elif name == "same":
            a, b = q0f, q0f.copy()
        else:
            a, b = q0f, np.array([float(x) for x in qmul(q0, qexp(MP, MP.vec([0.0, 0.0, sep])))])
        out.append((name, a, b))
        out.append((name + "/neg", a, -b))
    # track_slerp's om = acos(min(d, 1)) of the float64 dot d takes no value in (0, 1.49e-8): its threshold 1e-8 has exactly two
    # neighbours, d = 1 (om = 0, the lerp arm) and d = 1 - 2^-53 (om = 1.49e-8, the trigonometric arm).  Both, from the identity:
    one = np.array([1.0, 0.0, 0.0, 0.0])
    w = float(np.nextafter(1.0, 0.0))
    out.append(("om=0", one, np.array([1.0, 1e-9, 0.0, 0.0])))
    out.append(("om=1ulp", one, np.array([w, float(mp.sqrt(1 - mpf(w) ** 2)), 0.0, 0.0])))
    return out


def ang_vel_cases():
    """[(name, p)] wxyz: rows p two frames after the identity, for track_ang_vel.  With q the identity w and v of p (x) conj(q) are
    p's own components, exactly: n = |v| on 1e-12 and one ulp either side of it, w = 0, w one step either side of 0, w < 0."""
    lo, mid, hi = (float(v) for v in _nbrs(1e-12))
    c, s_ = float(np.cos(0.25)), float(np.sin(0.25))
    return [("n<1e-12", np.array([1.0, lo, 0.0, 0.0])), ("n=1e-12", np.array([1.0, mid, 0.0, 0.0])), ("n>1e-12", np.array([1.0, hi, 0.0, 0.0])),
            ("n=1e-12/oblique", np.concatenate([[1.0], 1e-12 * OBLIQUE])), ("n=0", np.array([1.0, 0.0, 0.0, 0.0])), ("n=0/w<0", np.array([-1.0, 0.0, 0.0, 0.0])),
            ("w=0", np.array([0.0, 0.0, 1.0, 0.0])), ("w=+tiny", np.array([1e-17, 0.0, 1.0, 0.0])), ("w=-tiny", np.array([-1e-17, 0.0, 1.0, 0.0])),
            ("w=-0.0", np.array([-0.0, 0.0, 1.0, 0.0])), ("w<0", np.array([-c, s_ * OBLIQUE[0], s_ * OBLIQUE[1], s_ * OBLIQUE[2]])),
            ("w<0/n=1e-12", np.array([-1.0, 0.0, 0.0, mid]))]


def smplx_angle_clip(J, joint, dtype=np.float64, max_angle=np.inf):
    """Un-resampled clip for the angle grid: frame = (angle, axis); first half: the edge rotation on `joint` and 0.3 rad about
    OBLIQUE on every other joint, second half: the edge rotation on every joint.  Returns (go [T, 3], fp [T, J, 3], n_single)."""
    rows = [a * ax for ax in AXES for a in angle_grid() if abs(a) <= max_angle]
    n = len(rows)
    fp = np.zeros((2 * n, J, 3))
    fp[:n] = 0.3 * OBLIQUE
    fp[:n, joint] = rows
    fp[n:] = np.asarray(rows)[:, None, :]
    fp = fp.astype(dtype)
    return fp[:, 0].copy(), fp, n


def smplx_pair_clips(J, joint, dtype=np.float64):
    """Resampled clips for the pair grid: frames r0, r1, r0, r1, ... of every pair in turn, so that every consecutive pair of
    frames is a pair of the grid (or one reversed).  Clip 0: on `joint` only, the others constant; clip 1: on every joint."""
    seq = []
    for _, r0, r1, _ in rotvec_pairs():
        seq += [r0, r1]
    seq = np.asarray(seq)
    T = len(seq)
    one = np.zeros((T, J, 3))
    one[:] = 0.3 * OBLIQUE
    one[:, joint] = seq
    every = np.repeat(seq[:, None, :], J, axis=1)
    return [(x[:, 0].astype(dtype).copy(), x.astype(dtype)) for x in (one, every)]


BVH_DEGREES = [0.0, -0.0, 90.0, -90.0, 180.0, -180.0] + [s * float(v) for s in (1.0, -1.0) for v in _nbrs(183.3464944)] \
    + [360.0, -360.0, 540.0, -540.0, 36000.0, -36000.0, 1e-7, 1e-300]
BVH_BASE = np.array([20.0, -35.0, 50.0])
BVH_ORDERS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


def bvh_clip(J, joint):
    """Euler channels [T, J, 3] in degrees: every value of BVH_DEGREES on each channel of `joint` in turn (BVH_BASE elsewhere),
    then on all channels of all joints; local positions [T, J, 3]: fixed offsets, a moving root."""
    rows = []
    for v in BVH_DEGREES:
        for c in range(3):
            e = np.tile(BVH_BASE, (J, 1))
            e[joint, c] = v
            rows.append(e)
        rows.append(np.full((J, 3), v))
    eul = np.asarray(rows)
    T = len(eul)
    offsets = np.array([[3.0 + j, -7.5 + 0.25 * j, 11.0 - j] for j in range(J)])
    lpos = np.repeat(offsets[None], T, axis=0)
    lpos[:, 0] = [[0.5 * f, 90.0 + 0.125 * f, -0.25 * f] for f in range(T)]
    return eul, lpos, offsets


def bvh_parents(J):
    """A chain for J = 3; for larger J a tree with a long spine and side branches (depth ~ J / 2)."""
    return np.array([-1] + [j - 1 if (j % 4 or J <= 3) else j // 2 for j in range(1, J)], dtype=np.int32)


def dof_angle_clip(ndof, hinge):
    """float32 hinge angles [T, ndof]: the angle grid on `hinge` (0.3 elsewhere), then on all hinges."""
    g = angle_grid(np.float32)
    one = np.full((len(g), ndof), 0.3, dtype=np.float32)
    one[:, hinge] = g
    return np.concatenate([one, np.repeat(g[:, None], ndof, axis=1)]).astype(np.float32)


ROT_LENS = [1e-5 * (1 + 1e-3), 1e-5 * (1 - 1e-3), 0.0, 1e-7, 1e-3]


def rot_to_dof_clip(axes, dof_body, nbody, lo, hi):
    """float32 joint rotations [T, nbody-1, 4] xyzw, every hinge about its own axis: |xyz| in ROT_LENS x axis sign x w sign, angles
    1e-3 inside and outside both ends of the joint's range (0.5 and -0.5 rad for a hinge without limits) also with the quaternion
    negated, and scaled copies (x 0.5, x 2) of two of those frames.  Returns (rot, labels)."""
    frames, labels = [], []

    def frame(fn):
        r = np.zeros((nbody - 1, 4))
        r[:, 3] = 1.0
        for d, b in enumerate(dof_body):
            ax = np.asarray(axes[d], dtype=np.float64)
            r[b - 1] = fn(d, ax / np.linalg.norm(ax))
        return r

    for ln in ROT_LENS:
        for sa in (1.0, -1.0):
            for sw in (1.0, -1.0):
                frames.append(frame(lambda d, ax: np.concatenate([sa * ln * ax, [sw * np.sqrt(1.0 - ln * ln)]])))
                labels.append(("len", ln, sa, sw))
    for end in (0, 1):
        for off in (-1e-3, 1e-3):
            for sg in (1.0, -1.0):
                def fn(d, ax):
                    lim = (lo[d], hi[d])[end]
                    th = float(lim) + off if np.isfinite(lim) else (0.5 if end else -0.5)
                    return sg * np.concatenate([np.sin(0.5 * th) * ax, [np.cos(0.5 * th)]])
                frames.append(frame(fn))
                labels.append(("clamp", end, off, sg))
    base_len, base_clamp = frames[0], frames[len(ROT_LENS) * 4 + 2]  # |xyz| just above the threshold: x 0.5 puts it below; a clamped angle
    for s in (0.5, 2.0):
        frames += [s * base_len, s * base_clamp]
        labels += [("scaled", s, "len"), ("scaled", s, "clamp")]
    return np.asarray(frames).astype(np.float32), labels


def track_clips(nq, fps_out):
    """qpos [N, nq] float64 (wxyz root quaternion at 3:7, constant hinges, a moving root position), one group of clips per pair
    (q0, q1) of quat_pairs():
      [q0, q1] at fps_out / 4                    -> weights 0, .25, .5, .75 and the copied last frame
      [q0, q0, q1] at fps_out (1 + 2^-20)        -> output row 1 interpolates frames 1, 2 with weight 2^-20 (WEIGHTS[1])
      [q0, q1] at fps_out (1 - 2^-20)            -> output row 1 interpolates frames 0, 1 with weight 1 - 2^-20 (WEIGHTS[5])
    then one clip [identity, identity, p] at fps_out (rows copied: a = 0) per entry of ang_vel_cases(), whose central and one-sided
    differences put track_ang_vel on exactly known inputs, and last a standing clip of 9 identical rows at fps_out / 4.
    Returns (qpos, seq_offsets, fps_in per clip)."""
    rows, lens, fps = [], [], []
    hinges = np.linspace(-0.4, 0.4, nq - 7)

    def clip(quats, rate, i):
        for k, q in enumerate(quats):
            rows.append(np.concatenate([[0.1 * i, 0.05 * k, 0.8], q, hinges]))
        lens.append(len(quats))
        fps.append(rate)

    for i, (_, a, b) in enumerate(quat_pairs()):
        clip((a, b), fps_out / 4, i)
        clip((a, a, b), fps_out * (1.0 + WEIGHTS[1]), i)
        clip((a, b), fps_out * WEIGHTS[5], i)
    one = np.array([1.0, 0.0, 0.0, 0.0])
    for i, (_, p) in enumerate(ang_vel_cases()):
        clip((one, one, p), fps_out, i)
    stand = np.array([float(x) for x in qexp(MP, MP.vec(0.3 * OBLIQUE))])
    clip([stand] * 9, fps_out / 4, 7)
    for r in rows[-9:]:
        r[:3] = [1.0, 2.0, 0.79]
    return np.asarray(rows), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.asarray(fps)


def track_reference(B, qpos, offs, out_offs, ratio, fps_out, rows=None):
    """(root_rot [M, 4] xyzw, root_ang_vel [M, 3]) of gmr_motion_track by the contract in include/gmr_amd.h.  The velocities are
    taken from `rows` (the call's own root_rot) when given, else from the resampled rows computed here."""
    M = int(out_offs[-1])
    rot = np.zeros((M, 4))
    for s in range(len(offs) - 1):
        T = int(offs[s + 1] - offs[s])
        for k in range(int(out_offs[s + 1] - out_offs[s])):
            u = k * float(ratio[s])
            i0 = min(max(int(np.floor(u)), 0), T - 1)
            i1 = min(i0 + 1, T - 1)
            a = u - i0 if i1 > i0 else 0.0
            x0, x1 = qpos[offs[s] + i0, [4, 5, 6, 3]], qpos[offs[s] + i1, [4, 5, 6, 3]]
            rot[out_offs[s] + k] = track_root_rot(B, x0, x1, a)
    src = rot if rows is None else rows
    vel = np.zeros((M, 3))
    for s in range(len(offs) - 1):
        Ms = int(out_offs[s + 1] - out_offs[s])
        for k in range(Ms):
            km, kp = max(k - 1, 0), min(k + 1, Ms - 1)
            if kp > km:
                vel[out_offs[s] + k] = track_ang_vel(B, src[out_offs[s] + kp], src[out_offs[s] + km], (kp - km) / fps_out)
    return rot, vel


# ------------------------------------------------------------------ the families: inputs once, evaluated over any number type
SMPLX_PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 15, 15, 15,
                 20, 25, 26, 20, 28, 29, 20, 31, 32, 20, 34, 35, 20, 37, 38, 21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50, 21, 52, 53]
SMPLX_EDGE_JOINT = 16   # left_shoulder: five ancestors, a whole hand below it
TRACK_FPS_OUT = 120.0   # the 2-frame clips of the pair grid come in at 30
FAMILIES = list(FLOAT_WORST)


@functools.lru_cache(maxsize=None)
def g1_hinges():
    """(axes [ndof, 3] float64, body of every hinge, nbody, float32 lower / upper limits) of unitree_g1, in dof order."""
    from gmr_amd import params
    from gmr_amd.mjcf import load_robot
    r = load_robot(params.ROBOT_XML_DICT["unitree_g1"], name="unitree_g1")
    hb = sorted((int(b) for b in r.hinge_bodies()), key=lambda b: int(r.qpos_adr[b]))
    rng = np.asarray(r.jnt_range, dtype=np.float64)[hb]
    return (np.asarray(r.jnt_axis, dtype=np.float64)[hb], hb, int(r.nbody), rng[:, 0].astype(np.float32), rng[:, 1].astype(np.float32),
            np.asarray(r.jnt_limited, dtype=bool)[hb], int(r.nq))


# ------------------------------------------------------------------ gmr_evaluate: task errors and body poses
K_LIE_EPS = 1e-10   # kLieEps of ik_kernel.hip.h (mink.lie.utils.get_epsilon(float64)): |w| and th^2 are compared with it
SQRT_LIE = 1e-5
# turn angles of the prepared target about a body axis.  The key-points reach the kernel through FK and the target preparation,
# which round at 1e-16 absolute: an ulp of 1e-5 cannot be placed, so sqrt(kLieEps) comes with neighbours at 1 +- 1e-9
TURN_ANGLES = [0.0, 1e-12, 1e-9, SQRT_LIE * (1 - 1e-9), SQRT_LIE, SQRT_LIE * (1 + 1e-9), 1e-4, 1.0, np.pi / 2, np.pi - 1e-3, np.pi - 1e-6,
               np.pi - 1e-9, np.pi, np.pi + 1e-9,
               # |w| = cos(angle / 2) against kLieEps: inside it on either side of w = 0 with a sign that is a number (1e-11 against the
               # 1e-16 to which w is known), and 1e-3 inside and outside of it
               np.pi - 2e-11, np.pi + 2e-11, np.pi - 2e-10 * (1 - 1e-3), np.pi - 2e-10 * (1 + 1e-3)]
TURN_PI = float(np.pi)   # the turn whose w is zero to rounding: the sign of omega is a convention there, not a number
TURN_OFFSET = 0.1   # m, along the body axis after the turn axis: omega x t is not zero, V^-1 t matters


def fk_bodies(B, robot, qpos):
    """World position and wxyz quaternion of every body (tests/ik_certificate.IKCertificate.fk, over the number type B)."""
    from gmr_amd.mjcf import JNT_HINGE
    xpos, xquat = [], []
    for b in range(robot.nbody):
        p, a = int(robot.parent[b]), int(robot.qpos_adr[b])
        if p < 0:
            xpos.append(B.vec(qpos[a:a + 3]))
            xquat.append(qnormalise(B, B.vec(qpos[a + 3:a + 7])))
            continue
        r = qrot(B, xquat[p], B.vec(robot.body_pos[b]))
        xpos.append(tuple(xpos[p][i] + r[i] for i in range(3)))
        q = qmul(xquat[p], B.vec(robot.body_quat[b]))
        if robot.jnt_type[b] == JNT_HINGE:
            h = B.c(qpos[a]) * B.c(0.5)
            s_, ax = B.sin(h), B.vec(robot.jnt_axis[b])
            q = qmul(q, (B.cos(h), s_ * ax[0], s_ * ax[1], s_ * ax[2]))
        xquat.append(qnormalise(B, q))
    return xpos, xquat


def prepared_target(B, cfg, off, root, hp, hq, is_root):
    """One body of IKCertificate.prepare_targets (the reference's update_targets, actual height = assumed height), over B."""
    sroot = tuple(B.c(cfg.human_scale_table[cfg.human_root_name]) * x for x in B.vec(root))
    if is_root:
        p = sroot
    else:
        sc = B.c(cfg.human_scale_table[off.human])
        p = tuple((B.c(x) - B.c(r)) * sc + s_ for x, r, s_ in zip(hp, root, sroot))
    q = qnormalise(B, qmul(qnormalise(B, B.vec(hq)), qnormalise(B, B.vec(off.rot_offset))))
    lo = B.vec(off.pos_offset)
    local = (lo[0], lo[1], lo[2] - B.c(cfg.ground_height))
    r = qrot(B, q, local)
    return tuple(p[i] + r[i] for i in range(3)), q


def task_error(B, xpos_b, xquat_b, tp, tq):
    """(e_pos, e_rot) = Log(T_body^-1 T_target), plus the branch quantities (w of the relative quaternion, th^2)."""
    inv = qconj(xquat_b)
    rel = qnormalise(B, qmul(inv, tq))
    t = qrot(B, inv, tuple(tp[i] - xpos_b[i] for i in range(3)))
    om = qlog(B, rel)
    return vinv_t(B, om, t) + tuple(om), rel[0], dot(om, om), t


@functools.lru_cache(maxsize=None)
def evaluate_setup(robot_name):
    """Everything of the gmr_evaluate family that needs no number type: model, certificate, the fixed valid qpos, the frames."""
    from gmr_amd.mjcf import JNT_HINGE
    from tests import ik_certificate as ikc
    from tests.util import compiled
    cm = compiled("smplx", robot_name)
    r, cfg = cm.robot, cm.config
    cert = ikc.IKCertificate(r, cfg)
    qpos = np.zeros(r.nq)
    qpos[:3] = [0.1, -0.2, 0.8]
    qpos[3:7] = [float(x) for x in qexp(MP, MP.vec([0.0, 0.0, 0.3] if cert.planar else 0.3 * OBLIQUE))]
    hb = sorted((int(b) for b in r.hinge_bodies()), key=lambda b: int(r.qpos_adr[b]))
    for k, b in enumerate(hb):
        lo, hi = (float(v) for v in r.jnt_range[b]) if r.jnt_limited[b] else (-1.0, 1.0)
        qpos[int(r.qpos_adr[b])] = lo + (hi - lo) * (0.3 + 0.4 * ((k * 7) % 10) / 10.0)
    offsets = {t.human: t for t in cfg.table1 if t.pos_weight != 0 or t.rot_weight != 0}
    names = sorted(set(offsets) | {cfg.human_root_name})
    col = {n: i for i, n in enumerate(names)}
    xpos, xquat = cert.fk(qpos)
    # base key-points: every prepared target on its table-1 body (any valid values would do)
    base_p = np.zeros((len(names), 3))
    base_q = np.tile([1.0, 0.0, 0.0, 0.0], (len(names), 1))
    root = np.array([0.05, 0.1, 0.9])
    base_p[:] = root

    def invert(h, tp, tq, root_now):
        off = offsets[h]
        ro = ikc._unit(np.asarray(off.rot_offset, dtype=np.float64))
        hq = ikc._qmul(tq, ikc._qconj(ro))
        local = np.asarray(off.pos_offset, dtype=np.float64) - cfg.ground_height * np.array([0.0, 0.0, 1.0])
        ps = tp - ikc._qrot(ikc._unit(ikc._qmul(ikc._unit(hq), ro)), local)
        s_root = cfg.human_scale_table[cfg.human_root_name]
        if h == cfg.human_root_name:
            return ps / s_root, hq
        return (ps - s_root * root_now) / cfg.human_scale_table[h] + root_now, hq

    nt0 = len(cm.tasks[0])
    frames, P, Q = [], [], []
    for k in cert.used_tables():
        for i, (b, h, wp, wr) in enumerate(cert.tables[k]):
            if h not in offsets:
                continue
            for ax in range(3):
                for ang in TURN_ANGLES:
                    v = np.zeros(3)
                    v[ax] = ang
                    tq = ikc._qmul(xquat[b], np.array([float(x) for x in qexp(MP, MP.vec(v))]))
                    o = np.zeros(3)
                    o[(ax + 1) % 3] = TURN_OFFSET
                    tp = xpos[b] + ikc._qrot(xquat[b], o)
                    hp, hq = invert(h, tp, tq, root)
                    p_, q_ = base_p.copy(), base_q.copy()
                    p_[col[h]], q_[col[h]] = hp, hq
                    frames.append(dict(row=k * nt0 + i, body=int(b), human=h, angle=float(ang), axis=ax))
                    P.append(p_)
                    Q.append(q_)
    # the hinge-angle run: sincos_fk's ballot at a half-angle of 1.6
    hv = [float(v) for v in angle_grid() if abs(v) <= float(np.nextafter(3.2, 4.0))]
    hv += [-v for v in hv if v > 0 and -v not in hv]
    hq_ = np.repeat(qpos[None], 2 * len(hv), axis=0)
    one = int(r.qpos_adr[hb[len(hb) // 2]])
    for n, v in enumerate(hv):
        hq_[n, one] = v
        hq_[len(hv) + n, [int(r.qpos_adr[b]) for b in hb]] = v
    return dict(cm=cm, cert=cert, qpos=qpos, names=names, col=col, offsets=offsets, frames=frames, pos=np.asarray(P), quat=np.asarray(Q),
                hinge_qpos=hq_, hinge_values=hv, root_name=cfg.human_root_name)


def evaluate_eval(B, robot_name):
    """{'task_err': [N, 6], 'xpos', 'xquat': the hinge run's body poses} plus the branch quantities 'w', 'th2' and the
    alternative result for the other sign of omega ('task_err_alt'), over B."""
    s_ = evaluate_setup(robot_name)
    r, cfg = s_["cm"].robot, s_["cm"].config
    xpos, xquat = fk_bodies(B, r, s_["qpos"])
    N = len(s_["frames"])
    err, alt, w, th2 = np.zeros((N, 6)), np.zeros((N, 6)), [], []
    for f, fr in enumerate(s_["frames"]):
        c, h = s_["col"][fr["human"]], fr["human"]
        tp, tq = prepared_target(B, cfg, s_["offsets"][h], s_["pos"][f, s_["col"][s_["root_name"]]], s_["pos"][f, c], s_["quat"][f, c],
                                 h == s_["root_name"])
        e, w_, t2, t = task_error(B, xpos[fr["body"]], xquat[fr["body"]], tp, tq)
        err[f] = [B.out(x) for x in e]
        om = tuple(-x for x in e[3:])
        alt[f] = [B.out(x) for x in vinv_t(B, om, t) + om]
        w.append(w_)
        th2.append(t2)
    hq = s_["hinge_qpos"]
    xp, xq = np.zeros((len(hq), r.nbody, 3)), np.zeros((len(hq), r.nbody, 4))
    for f in range(len(hq)):
        a, b = fk_bodies(B, r, hq[f])
        xp[f] = [[B.out(x) for x in v] for v in a]
        xq[f] = [[B.out(x) for x in v] for v in b]
    return {"task_err": [err], "xpos": [xp], "xquat": [xq], "task_err_alt": [alt], "w": w, "th2": th2}


@functools.lru_cache(maxsize=None)
def family_inputs(family):
    """The list of input sets (dicts of arrays) of a family; one kernel launch each."""
    if family.startswith("smplx"):
        tree = family.endswith("tree55")
        parents = np.array(SMPLX_PARENTS if tree else [-1, 0, 1], dtype=np.int32)
        J, joint = len(parents), SMPLX_EDGE_JOINT if tree else 0
        if "resample" in family:
            return [dict(go=go, fp=fp, parents=parents, T_out=4 * len(fp) - 3, joint=joint)
                    for dt in (np.float64, np.float32) for go, fp in smplx_pair_clips(J, joint, dt)]
        go, fp, n = smplx_angle_clip(J, joint, max_angle=0.5 if "small" in family else np.inf)
        return [dict(go=go, fp=fp, parents=parents, T_out=None, joint=joint, n_single=n)]
    if family.startswith("bvh"):
        J = 33 if family.endswith("tree33") else 3
        eul, lpos, offsets = bvh_clip(J, J // 2)
        return [dict(order=o, parents=bvh_parents(J), eul=eul, lpos=lpos, offsets=offsets, scale=0.01) for o in BVH_ORDERS]
    if family.startswith("evaluate_"):
        return [evaluate_setup(family[len("evaluate_"):])]
    axes, hb, nbody, lo, hi, _, nq = g1_hinges()
    if family == "dof_to_rot":
        return [dict(dof=dof_angle_clip(len(hb), 7))]
    if family == "rot_to_dof":
        rot, labels = rot_to_dof_clip(axes, hb, nbody, lo, hi)
        return [dict(rot=rot, labels=labels)]
    if family == "track":
        from gmr_amd.schedule import track_plan
        qpos, offs, fps_in = track_clips(nq, TRACK_FPS_OUT)
        out_offs, ratio = track_plan(offs, fps_in, TRACK_FPS_OUT)
        return [dict(qpos=qpos, offs=offs, fps_in=fps_in, out_offs=out_offs, ratio=ratio)]
    raise KeyError(family)


def family_eval(B, family, rows=None):
    """{output: [array per input set]} of a family over the number type B, as float64 arrays."""
    ins = family_inputs(family)
    if family.startswith("smplx"):
        return {"quat": [smplx_quats(B, i["go"], i["fp"], i["parents"], i["T_out"]) for i in ins]}
    if family.startswith("bvh"):
        res = [bvh_fk(B, i["parents"], i["order"], i["lpos"], i["eul"], i["scale"]) for i in ins]
        return {"pos": [r[0] for r in res], "quat": [r[1] for r in res]}
    if family.startswith("evaluate_"):
        return evaluate_eval(B, family[len("evaluate_"):])
    axes, hb, nbody, lo, hi, _, _ = g1_hinges()
    if family == "dof_to_rot":
        return {"quat": [dof_to_rot(B, axes, hb, nbody, i["dof"]) for i in ins]}
    if family == "rot_to_dof":
        return {"dof": [rot_to_dof(B, axes, hb, lo, hi, i["rot"]) for i in ins]}
    i = ins[0]
    rot, vel = track_reference(B, i["qpos"], i["offs"], i["out_offs"], i["ratio"], TRACK_FPS_OUT, rows)
    return {"root_rot": [rot], "root_ang_vel": [vel]}


@functools.lru_cache(maxsize=None)
def reference(family):
    """The 50-digit reference of a family, rounded to the kernel's output type (float32 for the kin-ops family)."""
    out = family_eval(MP, family)
    if family in ("dof_to_rot", "rot_to_dof"):
        out = {k: [a.astype(np.float32).astype(np.float64) for a in v] for k, v in out.items()}
    return out


def plain_float(family):
    """The same definitions in plain numpy float64 (float32 for the kin-ops family)."""
    with np.errstate(all="ignore"):
        return family_eval(F32 if family in ("dof_to_rot", "rot_to_dof") else F64, family)


def deviation(family, out, got, ref):
    """|got - reference| per element for one output of a family (a list over the input sets).  For the task errors of the
    gmr_evaluate family the frames turned by exactly pi are compared with the nearer of the two results that differ in the sign of
    omega: w is zero to rounding there and its sign is not decided by the inputs to any precision a float64 pipeline has."""
    d = [np.abs(x - y) for x, y in zip(got, ref[out])]
    if family.startswith("evaluate_") and out == "task_err":
        pi = np.array([fr["angle"] == TURN_PI for fr in evaluate_setup(family[len("evaluate_"):])["frames"]])
        alt = np.abs(got[0] - ref["task_err_alt"][0])
        use = pi & (alt.max(axis=1) < d[0].max(axis=1))
        d[0] = np.where(use[:, None], alt, d[0])
    return d


def worst(a, b):
    return max(float(np.abs(x - y).max()) for x, y in zip(a, b))


def family_worst(family, out, got, ref):
    return max(float(x.max()) for x in deviation(family, out, got, ref))

"""Self-collision repair: the contract above gmr_self_collision_repair_input (include/gmr_amd.h) restated in numpy, without a GPU and
without native code.

(1) numpy float64, vectorised over frames and pairs: FK as tests/dynamics_reference.fk, the capsule ends and the clamped closest
    points of tests/self_collision_reference.py (here with the points themselves, `closest`), the gradient of step 5 (`gradient`),
    the I passes (`repair`) and the per-clip reduction (`statistics`, a plain loop over frames).  Every sum the contract orders -- over
    the hinges of a pair, over the pairs of a frame -- is a loop in that order.
(2) the same code in np.longdouble (`repair(..., dtype=np.longdouble)`: x86's 80-bit format, 64 bits of mantissa), with its own FK.
    The map is iterated and has a threshold (v_p > 0), so (1) and (2) differ by more than one rounding: FLOAT_WORST is that
    distance, measured on every row of the GPU tests' cases (tests/self_collision_repair_inputs.py), and the GPU tests allow
    GPU_FACTOR times it.  Nothing in it was measured on a kernel.
"""
import numpy as np

from tests import dynamics_reference as R
from tests import self_collision_reference as SR

ITERATIONS, DAMPING, STEP_CAP, RESOLVE_TOL = 16, 1e-6, 0.2, 1e-4   # the call's defaults: conventions, not measured on a robot

# |float64 - longdouble| over every row of a case of tests/self_collision_repair_inputs.CASES, measured by its measure_floor (x86-64,
# numpy float64 against the 80-bit long double), rounded up to one digit: "qpos" the worst hinge angle of qpos_out in rad,
# "clearance" the worst of clearance_before and clearance_after in m.  tests/test_self_collision_repair_host.py re-measures them and
# fails if a recorded figure is smaller than what it measures.
#     g1            qpos 2.42e-14   clearance 7.04e-16        k1            qpos 9.33e-15   clearance 5.97e-16
#     g1_margin     qpos 2.71e-14   clearance 1.05e-15        k1_margin     qpos 1.91e-14   clearance 5.97e-16
#     g1_frozen     qpos 2.71e-14   clearance 1.05e-15        reach         qpos 7.91e-16   clearance 2.96e-16
FLOAT_WORST = {"g1": {"qpos": 3e-14, "clearance": 8e-16}, "g1_margin": {"qpos": 3e-14, "clearance": 2e-15},
               "g1_frozen": {"qpos": 3e-14, "clearance": 2e-15}, "k1": {"qpos": 1e-14, "clearance": 6e-16},
               "k1_margin": {"qpos": 2e-14, "clearance": 6e-16}, "reach": {"qpos": 8e-16, "clearance": 3e-16}}
GPU_FACTOR = 16.0        # foot locking's margin over its floor
QPOS_BOUND_MIN = 1e-9    # rad: the bound of qpos_out is never looser than this


def bound(case, output):
    """The largest admissible |kernel - numpy reference|: GPU_FACTOR times the reference's own distance to the extended evaluator on
    the same rows, and for qpos never more than QPOS_BOUND_MIN."""
    b = GPU_FACTOR * FLOAT_WORST[case][output]
    return min(b, QPOS_BOUND_MIN) if output == "qpos" else b


# ------------------------------------------------------------------ pieces
def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _rot(q, v):
    t = 2.0 * _cross(q[..., 1:], v)
    return v + q[..., :1] * t + _cross(q[..., 1:], t)


def fk(rob, q, dtype=np.float64):
    """dynamics_reference.fk; in another dtype the same steps in that dtype."""
    if dtype is np.float64:
        return R.fk(rob, q)
    N = q.shape[0]
    X, Q = np.zeros((N, rob.nbody, 3), dtype), np.zeros((N, rob.nbody, 4), dtype)
    X[:, 0] = q[:, 0:3]
    Q[:, 0] = q[:, 3:7] / np.sqrt(np.sum(q[:, 3:7] * q[:, 3:7], axis=1, keepdims=True))
    for b in range(1, rob.nbody):
        p = int(rob.parent[b])
        X[:, b] = X[:, p] + _rot(Q[:, p], np.asarray(rob.body_pos[b], dtype))
        r = R._qmul(Q[:, p], np.broadcast_to(np.asarray(rob.body_quat[b], dtype), (N, 4)))
        if rob.jnt_type[b] == R.JNT_HINGE:
            h = q[:, rob.qpos_adr[b]] / dtype(2)
            r = R._qmul(r, np.concatenate([np.cos(h)[:, None], np.sin(h)[:, None] * np.asarray(rob.jnt_axis[b], dtype)], 1))
        Q[:, b] = r
    return X, Q


def closest(p1, q1, p2, q2):
    """self_collision_reference.segment_distance with the closest points: (a, b) [..., 3] with a = p1 + s d1, b = p2 + t d2."""
    with np.errstate(all="ignore"):
        d1, d2, r = q1 - p1, q2 - p2, p1 - p2
        a, e, f, c, b = _dot(d1, d1), _dot(d2, d2), _dot(d2, r), _dot(d1, r), _dot(d1, d2)
        den = a * e - b * b
        c01 = SR._clamp01
        s = np.where(den > 0.0, c01((b * f - c * e) / den), 0.0)
        t = np.where(e > 0.0, (b * s + f) / e, 0.0)
        lo, hi = ~(e > 0.0) | (t < 0.0), t > 1.0
        s = np.where(lo, np.where(a > 0.0, c01(-c / a), 0.0), np.where(hi, np.where(a > 0.0, c01((b - c) / a), 0.0), s))
        t = np.where(lo, 0.0, np.where(hi, 1.0, t))
        return p1 + s[..., None] * d1, p2 + t[..., None] * d2


def hinge_bodies(rob):
    """The hinge bodies in qpos order."""
    hb = [b for b in range(rob.nbody) if rob.jnt_type[b] == R.JNT_HINGE]
    return sorted(hb, key=lambda b: int(rob.qpos_adr[b]))


def ancestor_matrix(rob):
    """[nbody, nh] bool: hinge i (qpos order) lies on the path from the root to the body, the body's own hinge included."""
    hb = hinge_bodies(rob)
    col = {b: i for i, b in enumerate(hb)}
    A = np.zeros((rob.nbody, len(hb)), bool)
    for b, path in enumerate(R.ancestors(rob)):
        A[b, [col[j] for j in path]] = True
    return A


def mask_array(rob, hinge_mask):
    """The uint64 hinge mask as [nh] bool."""
    nh = len(hinge_bodies(rob))
    return np.array([(int(hinge_mask) >> i) & 1 == 1 for i in range(nh)], bool)


def limits(rob):
    """(lo, hi) [nh] in qpos order, -inf / +inf for an unlimited hinge."""
    hb = hinge_bodies(rob)
    lo, hi = np.full(len(hb), -np.inf), np.full(len(hb), np.inf)
    for i, b in enumerate(hb):
        if rob.jnt_limited[b]:
            lo[i], hi[i] = rob.jnt_range[b]
    return lo, hi


class Evaluation:
    """Steps 1, 2, 4 and 5 at qpos [N, nq]: `c` [N, P] clearances, `nw` [N, P], `g` [N, P, nh] the gradient entries (0 outside the
    moving set), `moving` [P] bool (M_p is not empty)."""

    def __init__(self, rob, caps, pairs, q, hinge_mask, dtype=np.float64, gradient=True):
        q = np.asarray(q, dtype)
        with np.errstate(all="ignore"):
            X, Qt = fk(rob, q, dtype)
            xb, rb = X[:, caps.body], Qt[:, caps.body]
            P0, P1 = xb + _rot(rb, caps.p0[None].astype(dtype)), xb + _rot(rb, caps.p1[None].astype(dtype))
            ia, ib = pairs.pairs[:, 0], pairs.pairs[:, 1]
            a, b = closest(P0[:, ia], P1[:, ia], P0[:, ib], P1[:, ib])
            w = a - b
            self.nw = np.sqrt(_dot(w, w))
            self.c = self.nw - (caps.radius[ia] + caps.radius[ib]).astype(dtype)[None]
            A = ancestor_matrix(rob)
            m = mask_array(rob, hinge_mask)
            AX, AY = A[caps.body[ia]], A[caps.body[ib]]
            self.in_x, self.in_y = AX & ~AY & m, AY & ~AX & m          # [P, nh]
            self.moving = (self.in_x | self.in_y).any(axis=1)
            if not gradient:
                return
            n = np.where((self.nw > 0.0)[..., None], w / self.nw[..., None], 0.0)
            hb = hinge_bodies(rob)
            self.g = np.zeros(self.c.shape + (len(hb),), dtype)
            for i, hbody in enumerate(hb):
                u = _rot(Qt[:, hbody], np.asarray(rob.jnt_axis[hbody], dtype))[:, None]      # [N, 1, 3]
                o = X[:, hbody][:, None]
                gx = _dot(n, _cross(u, a - o))
                gy = -_dot(n, _cross(u, b - o))
                self.g[:, :, i] = np.where(self.in_x[:, i][None], gx, np.where(self.in_y[:, i][None], gy, 0.0))


def frame_clearance(c):
    """The report's per-frame minimum over the pairs [N, P]: NaN when any pair is NaN."""
    bad = np.isnan(c).any(axis=1)
    return np.where(bad, np.nan, np.where(np.isnan(c), np.inf, c).min(axis=1))


def repair(rob, caps, pairs, q, seq_offsets, margin=0.0, iterations=ITERATIONS, damping=DAMPING, step_cap=STEP_CAP,
           resolve_tol=RESOLVE_TOL, hinge_mask=(1 << 64) - 1, dtype=np.float64):
    """Every output of the call by name (per-frame arrays for all N rows: a row outside every clip is not the reference's business),
    plus `nw_min`, the smallest nw of a pair with v_p > 0 in any pass, and `violating` [N] bool (V > 0 in the first pass)."""
    q_in = np.asarray(q, np.float64)
    N, nq = q_in.shape
    q0 = q_in.astype(dtype)
    qc = q0.copy()
    valid = np.isfinite(q_in).all(axis=1)
    lo, hi = limits(rob)
    cols = np.array([int(rob.qpos_adr[b]) for b in hinge_bodies(rob)])
    m = mask_array(rob, hinge_mask)
    margin, damping, step_cap = dtype(margin), dtype(damping), dtype(step_cap)
    live = valid.copy()               # frames whose passes may still change something
    nw_min = np.inf
    before = violating = None
    with np.errstate(all="ignore"):
        for it in range(iterations):
            rows = np.flatnonzero(live)
            ev = Evaluation(rob, caps, pairs, qc[rows] if it else qc, hinge_mask, dtype)
            if it == 0:
                before = np.where(valid, frame_clearance(ev.c), np.nan)
                c, g, nw = ev.c[rows], ev.g[rows], ev.nw[rows]
            else:
                c, g, nw = ev.c, ev.g, ev.nw
            v = margin - c
            v = np.where((v > 0.0) & ev.moving[None], v, 0.0)       # (a NaN gives 0)
            active = np.flatnonzero((v > 0.0).any(axis=0))
            V = np.zeros(len(rows), dtype)
            acc = np.zeros((len(rows), len(cols)), dtype)
            for p in active:                                          # ascending; a pair with v = 0 adds 0.0
                gp = g[:, p]
                s2 = np.zeros(len(rows), dtype)
                for i in range(len(cols)):                            # ascending from 0.0
                    s2 = s2 + gp[:, i] * gp[:, i]
                rho = v[:, p] / (s2 + damping)
                acc = acc + (v[:, p] * rho)[:, None] * gp
                V = V + v[:, p]
            if it == 0:
                violating = np.zeros(N, bool)
                violating[rows] = V > 0.0
            if active.size:
                nw_min = min(nw_min, float(nw[:, active][v[:, active] > 0.0].min()))
            go = V > 0.0
            live[rows[~go]] = False
            rows, acc, V = rows[go], acc[go], V[go]
            if not rows.size:
                break
            dq = acc / V[:, None]
            mx = np.abs(dq).max(axis=1)
            scale = np.where(mx > step_cap, step_cap / mx, dtype(1.0))
            cur, start = qc[rows][:, cols], q0[rows][:, cols]
            new = cur + scale[:, None] * dq
            lw, hw = np.minimum(lo[None].astype(dtype), start), np.maximum(hi[None].astype(dtype), start)
            new = np.where(new < lw, lw, np.where(new > hw, hw, new))
            new = np.where(m[None] & (dq != 0.0), new, cur)           # a hinge without a step keeps its bits
            tmp = qc[rows]
            tmp[:, cols] = new
            qc[rows] = tmp
        after = np.where(valid, frame_clearance(Evaluation(rob, caps, pairs, qc, hinge_mask, dtype, gradient=False).c), np.nan)
    qout = np.where(valid[:, None], qc.astype(np.float64), q_in)
    qout[:, :7] = q_in[:, :7]
    move = np.where(valid, np.abs(qc[:, cols] - q0[:, cols]).max(axis=1, initial=0.0), 0.0).astype(np.float64)
    out = {"qpos": qout, "clearance_before": before.astype(np.float64), "clearance_after": after.astype(np.float64), "move": move}
    out.update(statistics(out["clearance_after"], out["move"], seq_offsets, float(margin), resolve_tol))
    out["nw_min"], out["violating"] = nw_min, violating
    return out


def statistics(clearance_after, move, seq_offsets, margin, resolve_tol):
    """The per-clip statistics of the contract from the per-frame arrays, frame by frame."""
    S, N = len(seq_offsets) - 1, clearance_after.shape[0]
    out = {"repaired_frames": np.zeros(S, np.int32), "unresolved_frames": np.zeros(S, np.int32), "move_max": np.zeros(S, np.float64),
           "clearance_min_after": np.full(S, np.inf), "nonfinite_frames": np.zeros(S, np.int32)}
    thr = np.float64(margin) - np.float64(resolve_tol)
    for s in range(S):
        a = min(max(int(seq_offsets[s]), 0), N)
        b = min(max(int(seq_offsets[s + 1]), a), N)
        for k in range(a, b):
            c, mv = clearance_after[k], move[k]
            if np.isnan(c):
                out["nonfinite_frames"][s] += 1
                continue
            out["repaired_frames"][s] += int(mv > 0.0)
            out["unresolved_frames"][s] += int(c < thr)
            out["move_max"][s] = max(out["move_max"][s], mv)
            out["clearance_min_after"][s] = min(out["clearance_min_after"][s], c)
    return out

"""Self-collision: the contract above gmr_self_collision_input (include/gmr_amd.h) restated twice, without a GPU and without native
code.

(1) numpy float64, vectorised over frames and pairs: FK as tests/dynamics_reference.fk, the capsule ends, the clamped closest-point
    clearance in the contract's operation order (`pair_clearance`), the per-frame reduction (`frames`) and the per-clip statistics
    (`statistics`, a plain loop over frames).
(2) mpmath at 50 digits (`mp_pair_clearance`) along the analytic trajectories of tests/dynamics_reference.Trajectory: poses from
    rotation matrices (not the quaternion sandwich of (1)), every pair of a frame.

The bound of the GPU tests is GPU_FACTOR times the distance of (1) to (2), measured on rows of the GPU tests' own cases
(tests/self_collision_inputs.py) over all their pairs, and kept here per case.  Nothing in it was measured on a kernel.
"""
import numpy as np

from tests import dynamics_reference as R

mp, mpf = R.mp, R.mpf

# |numpy reference - 50-digit evaluator| of a pair clearance, the worst over ALL pairs of the rows self_collision_inputs.floor_rows
# picks (every clip's first row, the rows nearest the margin, the deepest rows, the rows with the smallest gap between the best and
# the second-best pair), measured by self_collision_inputs.measure_floor (x86-64, numpy float64), rounded up to one digit:
#     unitree_g1 (0.03 m)             2.78e-15   (26 rows x 869 pairs)
#     booster_k1 (0.05 m)             1.20e-15   (25 rows x 296 pairs)
#     unitree_g1_with_hands (0.01 m)  1.11e-15   (25 rows x 1 633 pairs)
# tests/test_self_collision_host.py re-measures them and fails if a recorded figure is smaller than what it measures.
FLOAT_WORST = {"unitree_g1": 3e-15, "booster_k1": 2e-15, "unitree_g1_with_hands": 2e-15}
# The same for the synthetic trees of tests/synthetic_trees.py at each tree's radius, the worst over ALL pairs of ALL 332 rows
# (self_collision_inputs.measure_floor(tree, range(332)); 193 s for the slowest, the 64-body star), rounded up to one digit;
# tests/test_synthetic_trees_host.py re-measures the rows of floor_rows.  tree/chain/2 has no pair: its figure is the worst
# |numpy FK - 50 digits| of a body origin over the 332 rows (self_collision_inputs.measure_origin_floor), which the transition
# search's test holds that tree's points to.
#     tree/chain/2   origins   1.78e-15
#     tree/chain/3   (0.01 m)  3.12e-16   (1 pair)         tree/star/5    (0.01 m)  1.89e-15   (18 pairs)
#     tree/chain/4   (0.01 m)  1.36e-15   (3 pairs)        tree/star/9    (0.01 m)  1.59e-15   (81 pairs)
#     tree/chain/5   (0.01 m)  1.72e-15   (6 pairs)        tree/star/17   (0.01 m)  1.72e-15   (354 pairs)
#     tree/chain/8   (0.01 m)  3.11e-15   (21 pairs)       tree/star/33   (0.01 m)  1.97e-15   (1 471 pairs)
#     tree/chain/9   (0.01 m)  2.14e-15   (27 pairs)       tree/star/64   (0.01 m)  2.07e-15   (5 815 pairs)
#     tree/chain/16  (0.01 m)  3.55e-15   (105 pairs)      tree/comb/5    (0.01 m)  2.02e-15   (18 pairs)
#     tree/chain/17  (0.01 m)  3.36e-15   (120 pairs)      tree/comb/9    (0.03 m)  2.32e-15   (45 pairs)
#     tree/chain/32  (0.01 m)  5.19e-15   (458 pairs)      tree/comb/17   (0.01 m)  3.66e-15   (165 pairs)
#     tree/chain/33  (0.01 m)  4.27e-15   (494 pairs)      tree/comb/33   (0.01 m)  6.11e-15   (586 pairs)
#     tree/chain/64  (0.01 m)  7.02e-15   (1 948 pairs)    tree/comb/64   (0.01 m)  7.27e-15   (2 136 pairs)
FLOAT_WORST.update({
    "tree/chain/2": 2e-15, "tree/chain/3": 4e-16, "tree/chain/4": 2e-15, "tree/chain/5": 2e-15, "tree/chain/8": 4e-15, "tree/chain/9": 3e-15,
    "tree/chain/16": 4e-15, "tree/chain/17": 4e-15, "tree/chain/32": 6e-15, "tree/chain/33": 5e-15, "tree/chain/64": 8e-15,
    "tree/star/5": 2e-15, "tree/star/9": 2e-15, "tree/star/17": 2e-15, "tree/star/33": 2e-15, "tree/star/64": 3e-15,
    "tree/comb/5": 3e-15, "tree/comb/9": 3e-15, "tree/comb/17": 4e-15, "tree/comb/33": 7e-15, "tree/comb/64": 8e-15})
GPU_FACTOR = 10.0


def bound(robot):
    """The largest admissible |kernel - numpy reference| of a clearance: ten times the numpy reference's own measured distance to
    50 digits, as an absolute figure in metres."""
    return GPU_FACTOR * FLOAT_WORST[robot]


# ------------------------------------------------------------------ numpy float64
def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _clamp01(x):
    return np.where(x > 0.0, np.where(x < 1.0, x, 1.0), 0.0)   # 0 for a NaN


def segment_distance(p1, q1, p2, q2):
    """The contract's clamped closest points, in its operation order; arrays [..., 3]."""
    with np.errstate(all="ignore"):
        d1, d2, r = q1 - p1, q2 - p2, p1 - p2
        a, e, f, c, b = _dot(d1, d1), _dot(d2, d2), _dot(d2, r), _dot(d1, r), _dot(d1, d2)
        den = a * e - b * b
        s = np.where(den > 0.0, _clamp01((b * f - c * e) / den), 0.0)
        t = np.where(e > 0.0, (b * s + f) / e, 0.0)
        lo, hi = ~(e > 0.0) | (t < 0.0), t > 1.0
        s = np.where(lo, np.where(a > 0.0, _clamp01(-c / a), 0.0), np.where(hi, np.where(a > 0.0, _clamp01((b - c) / a), 0.0), s))
        t = np.where(lo, 0.0, np.where(hi, 1.0, t))
        w = (p1 + s[..., None] * d1) - (p2 + t[..., None] * d2)
        return np.sqrt(_dot(w, w))


def ends(rob, caps, q):
    """World ends (P, Q) [N, C, 3] of the capsules at qpos [N, nq]."""
    with np.errstate(all="ignore"):
        X, Qt = R.fk(rob, np.asarray(q, dtype=np.float64))
        xb, rb = X[:, caps.body], Qt[:, caps.body]
        return xb + R._rot(rb, caps.p0[None]), xb + R._rot(rb, caps.p1[None])


def pair_clearance(rob, caps, pairs, q):
    """[N, P]: the clearance of every pair in every frame."""
    P, Q = ends(rob, caps, q)
    ia, ib = pairs.pairs[:, 0], pairs.pairs[:, 1]
    with np.errstate(all="ignore"):
        return segment_distance(P[:, ia], Q[:, ia], P[:, ib], Q[:, ib]) - (caps.radius[ia] + caps.radius[ib])[None]


def frames(cl, margin=0.0):
    """The per-frame outputs of the contract from the pair clearances [N, P]: the minimum (NaN when any pair is NaN), the lowest
    index that attains it (-1 in a NaN frame), the pairs below the margin (0 in a NaN frame)."""
    bad = np.isnan(cl).any(axis=1)
    safe = np.where(np.isnan(cl), np.inf, cl)
    clearance = np.where(bad, np.nan, safe.min(axis=1))
    pair = np.where(bad, -1, safe.argmin(axis=1)).astype(np.int32)          # (argmin: the first of equals)
    with np.errstate(all="ignore"):
        hits = np.where(bad, 0, (cl < margin).sum(axis=1)).astype(np.int32)
    return {"clearance": clearance, "pair": pair, "hits": hits}


def statistics(clearance, pair, hits, seq_offsets):
    """The per-clip statistics of the contract from the three per-frame arrays, frame by frame."""
    S = len(seq_offsets) - 1
    N = clearance.shape[0]
    out = {"clearance_min": np.full(S, np.inf), "worst_frame": np.full(S, -1, np.int32), "worst_pair": np.full(S, -1, np.int32),
           "colliding_frames": np.zeros(S, np.int32), "longest_run": np.zeros(S, np.int32), "hits_sum": np.zeros(S, np.int64),
           "nonfinite_frames": np.zeros(S, np.int32)}
    for s in range(S):
        a = min(max(int(seq_offsets[s]), 0), N)
        b = min(max(int(seq_offsets[s + 1]), a), N)
        run = 0
        for k in range(a, b):
            c, h = clearance[k], int(hits[k])
            out["hits_sum"][s] += h
            if np.isnan(c):
                out["nonfinite_frames"][s] += 1
                run = 0
                continue
            if out["worst_frame"][s] < 0 or c < out["clearance_min"][s]:
                out["clearance_min"][s], out["worst_frame"][s], out["worst_pair"][s] = c, k - a, pair[k]
            if h > 0:
                out["colliding_frames"][s] += 1
                run += 1
                out["longest_run"][s] = max(out["longest_run"][s], run)
            else:
                run = 0
    return out


def self_collision(rob, caps, pairs, q, seq_offsets, margin=0.0):
    """Every output of the call by name, plus `pair_clearance` [N, P]."""
    cl = pair_clearance(rob, caps, pairs, q)
    out = frames(cl, margin)
    out.update(statistics(out["clearance"], out["pair"], out["hits"], seq_offsets))
    out["pair_clearance"] = cl
    return out


# ------------------------------------------------------------------ 50 digits
def _mp_vec(v):
    return tuple(mpf(float(x)) for x in v)


def _mp_dot(u, v):
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]


def mp_segment_distance(p1, q1, p2, q2):
    """The distance of two segments in 50 digits (the same closest-point construction: it is exact in exact arithmetic)."""
    c01 = lambda x: mpf(0) if x < 0 else (mpf(1) if x > 1 else x)   # noqa: E731
    d1, d2, r = tuple(q1[k] - p1[k] for k in range(3)), tuple(q2[k] - p2[k] for k in range(3)), tuple(p1[k] - p2[k] for k in range(3))
    a, e, f, c, b = _mp_dot(d1, d1), _mp_dot(d2, d2), _mp_dot(d2, r), _mp_dot(d1, r), _mp_dot(d1, d2)
    den = a * e - b * b
    s = c01((b * f - c * e) / den) if den > 0 else mpf(0)
    t = (b * s + f) / e if e > 0 else mpf(0)
    if not e > 0 or t < 0:
        t, s = mpf(0), (c01(-c / a) if a > 0 else mpf(0))
    elif t > 1:
        t, s = mpf(1), (c01((b - c) / a) if a > 0 else mpf(0))
    w = tuple((p1[k] + s * d1[k]) - (p2[k] + t * d2[k]) for k in range(3))
    return mp.sqrt(_mp_dot(w, w))


def mp_ends(traj, caps, t):
    """World ends of every capsule at the mpf time t on an analytic trajectory: poses as rotation matrices in 50 digits."""
    rob = traj.rob
    q = traj.mp_q(t)
    n = mp.sqrt(sum(x * x for x in q[3:7]))
    X, Q = [tuple(q[0:3])], [tuple(x / n for x in q[3:7])]
    for b in range(1, rob.nbody):
        p = int(rob.parent[b])
        d = R._mp_matvec(R._mp_mat(Q[p]), _mp_vec(rob.body_pos[b]))
        X.append(tuple(X[p][c] + d[c] for c in range(3)))
        r = R._mp_qmul(Q[p], _mp_vec(rob.body_quat[b]))
        if rob.jnt_type[b] == R.JNT_HINGE:
            h = q[rob.qpos_adr[b]] / 2
            r = R._mp_qmul(r, (mp.cos(h),) + tuple(mp.sin(h) * x for x in _mp_vec(rob.jnt_axis[b])))
        Q.append(r)
    mats = [R._mp_mat(qb) for qb in Q]
    P, E = [], []
    for i in range(len(caps)):
        b = int(caps.body[i])
        e0, e1 = R._mp_matvec(mats[b], _mp_vec(caps.p0[i])), R._mp_matvec(mats[b], _mp_vec(caps.p1[i]))
        P.append(tuple(X[b][c] + e0[c] for c in range(3)))
        E.append(tuple(X[b][c] + e1[c] for c in range(3)))
    return P, E


def mp_pair_clearance(traj, caps, pairs, t):
    """[P] floats, rounded once from 50 digits: the clearance of every pair at time t."""
    P, E = mp_ends(traj, caps, t)
    rad = [mpf(float(x)) for x in caps.radius]
    return np.array([float(mp_segment_distance(P[a], E[a], P[b], E[b]) - (rad[a] + rad[b])) for a, b in pairs.pairs.tolist()])

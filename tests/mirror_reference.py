"""The numpy definition of gmr_motion_mirror (the contract above gmr_mirror_input in include/gmr_amd.h), both modes, and a 50-digit
evaluator of the GMR_MIRROR_CLIP_START root map.  No GPU and no torch are needed here.

  world       copies and sign flips: the GPU must equal it bit for bit.
  clip_start  the hinge columns are world's; the root columns follow the contract's operation order in float64.  The GPU is
              allowed GPU_FACTOR times this function's own worst distance to mp_clip_start_root on the same rows (FLOAT_WORST,
              re-measured by tests/test_symmetry_host.py), as an absolute figure with no other factor.  Nothing in the bound was
              measured on a kernel.
  mp_clip_start_root  the definition as the contract words it -- psi = atan2(f_y, f_x), cos 2 psi, sin 2 psi, r_z(2 psi) -- in
              50-digit arithmetic: it shares the formula's meaning with the float64 code, not its algebra.
"""
import numpy as np
from mpmath import mp, mpf

mp.dps = 50

WORLD_ROOT_SIGN = np.array([1.0, -1.0, 1.0, 1.0, -1.0, 1.0, -1.0])   # (x, -y, z), (w, -x, y, -z)
HEADING_EPS = 1e-12

# Worst |clip_start - mp_clip_start_root| over the root columns of the rows of tests/mirror_inputs.py, per robot: metres on the
# position columns, quaternion components on the others.  Recorded figures are rounded up; tests/test_symmetry_host.py re-measures
# them and fails if one is smaller than what it measures.
FLOAT_WORST = {"unitree_g1": {"pos": 3e-15, "quat": 5e-16},
               "booster_k1": {"pos": 3e-15, "quat": 5e-16},
               "unitree_g1_with_hands": {"pos": 3e-15, "quat": 5e-16}}
GPU_FACTOR = 10.0


def bound(robot, what):
    """The largest admissible |kernel - clip_start| on the root columns: ``what`` is "pos" or "quat"."""
    return GPU_FACTOR * FLOAT_WORST[robot][what]


def hinges(plan, q):
    """out[c] = q[col_src[c]], negated where col_sign[c] < 0 (all columns; the root's hold the identity)."""
    g = q[..., plan.col_src]
    return np.where(plan.col_sign < 0.0, -g, g)


def world(plan, q):
    out = hinges(plan, q)
    out[..., :7] = np.where(WORLD_ROOT_SIGN < 0.0, -q[..., :7], q[..., :7])
    return out


def heading(r0):
    """(cos psi, sin psi, cos 2psi, sin 2psi) of first-row root quaternions [..., 4], in the contract's operation order."""
    with np.errstate(all="ignore"):
        w0, x0, y0, z0 = (r0[..., i] for i in range(4))
        n = np.sqrt(((w0 * w0 + x0 * x0) + y0 * y0) + z0 * z0)
        w, x, y, z = w0 / n, x0 / n, y0 / n, z0 / n
        fx, fy = 1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y + w * z)
        h2 = fx * fx + fy * fy
        flat = h2 < HEADING_EPS
        h = np.sqrt(h2)
        cp, sp = np.where(flat, 1.0, fx / h), np.where(flat, 0.0, fy / h)
        c2, s2 = np.where(flat, 1.0, (fx * fx - fy * fy) / h2), np.where(flat, 0.0, (2.0 * fx * fy) / h2)
    return cp, sp, c2, s2


def clip_start(plan, q, offs, fill=None):
    """The mirrored rows of every clip; rows outside every clip hold ``fill`` (None: a copy of q)."""
    out = q.copy() if fill is None else np.full_like(q, fill)
    N = q.shape[0]
    for s in range(len(offs) - 1):
        a = min(max(int(offs[s]), 0), N)
        b = min(max(int(offs[s + 1]), a), N)
        if b <= a:
            continue
        rows = q[a:b]
        res = hinges(plan, rows)
        cp, sp, c2, s2 = heading(rows[0, 3:7])
        p0 = rows[0, 0:3]
        with np.errstate(all="ignore"):
            dx, dy = rows[:, 0] - p0[0], rows[:, 1] - p0[1]
            res[:, 0] = p0[0] + (c2 * dx + s2 * dy)
            res[:, 1] = p0[1] + ((-c2) * dy + s2 * dx)
            res[:, 2] = rows[:, 2]
            w, x, y, z = (rows[:, 3 + i] for i in range(4))
            res[:, 3] = cp * w + sp * z
            res[:, 4] = (-cp) * x + (-sp) * y
            res[:, 5] = cp * y + (-sp) * x
            res[:, 6] = (-cp) * z + sp * w
        out[a:b] = res
    return out


def world_clips(plan, q, offs, fill=None):
    """``world`` on the rows of the clips, ``fill`` elsewhere."""
    out = q.copy() if fill is None else np.full_like(q, fill)
    N = q.shape[0]
    for s in range(len(offs) - 1):
        a = min(max(int(offs[s]), 0), N)
        b = min(max(int(offs[s + 1]), a), N)
        out[a:b] = world(plan, q[a:b])
    return out


# ------------------------------------------------------------------ 50 digits
def _mp_qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return [aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
            aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw]


def mp_heading(first):
    """psi of a first row (float64 values taken as exact), or 0 where the heading is not defined."""
    w, x, y, z = (mpf(float(v)) for v in first[3:7])
    n = mp.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    fx, fy = 1 - 2 * (y * y + z * z), 2 * (x * y + w * z)
    return mpf(0) if fx * fx + fy * fy < mpf(HEADING_EPS) else mp.atan2(fy, fx)


def mp_clip_start_root(row, first):
    """The seven root columns of one mirrored row, as mpf: ``row`` and ``first`` are float64 qpos rows taken as exact."""
    psi = mp_heading(first)
    c2, s2 = mp.cos(2 * psi), mp.sin(2 * psi)
    p0 = [mpf(float(v)) for v in first[0:3]]
    p = [mpf(float(v)) for v in row[0:3]]
    dx, dy = p[0] - p0[0], p[1] - p0[1]
    pos = [p0[0] + c2 * dx + s2 * dy, p0[1] + s2 * dx - c2 * dy, p[2]]
    w, x, y, z = (mpf(float(v)) for v in row[3:7])
    quat = _mp_qmul([mp.cos(psi), mpf(0), mpf(0), mp.sin(psi)], [w, -x, y, -z])
    return pos + quat


def measure_floor(plan, q, offs, rows=None):
    """Worst |clip_start - mp_clip_start_root| over ``rows`` (None: every row of every clip): {"pos": ., "quat": .}."""
    got = clip_start(plan, q, offs)
    worst = {"pos": 0.0, "quat": 0.0}
    for s in range(len(offs) - 1):
        a, b = int(offs[s]), int(offs[s + 1])
        for i in range(a, b):
            if rows is not None and i not in rows:
                continue
            want = mp_clip_start_root(q[i], q[a])
            err = [abs(float(mpf(float(g)) - w)) for g, w in zip(got[i, :7], want)]
            worst["pos"] = max(worst["pos"], max(err[:3]))
            worst["quat"] = max(worst["quat"], max(err[3:]))
    return worst

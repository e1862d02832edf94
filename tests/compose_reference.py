"""The numpy restatement of gmr_motion_compose (the contract above gmr_compose_input in include/gmr_amd.h) and a 50-digit evaluator
of its mathematical definition.  No GPU and no torch are needed here.

  compose     the contract's operation order in float64: the kernels must equal it bit for bit everywhere except the root
              quaternion of blended rows, where the slerp's acos / sin may differ between the two libms (SLERP_RAD).
  mp_compose  the definition as mathematics -- headings as atan2 angles, exact rotations by the accumulated angle, the half angle as
              cos / sin of half of it, the slerp through the relative rotation's angle -- in 50-digit arithmetic.  It shares the
              formula's meaning with the float64 code, not its algebra.  compose is allowed mp_bound = 32 K eps (1 + L) against it (K
              the segments of the chain, L the largest |coordinate|: a few eps per composition, carried over K compositions).
"""
import numpy as np
from mpmath import mp, mpf

mp.dps = 50

EPS = float(np.finfo(np.float64).eps)
HEADING_EPS = 1e-12
SLERP_RAD = 1e-12          # the project's slerp bound (tests/test_gpu_motion_sample.py)
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def mp_bound(k_segments, largest):
    return 32.0 * k_segments * EPS * (1.0 + largest)


def heading(r):
    """(cos psi, sin psi) of root quaternions [..., 4] (w x y z), in the contract's operation order."""
    with np.errstate(all="ignore"):
        w0, x0, y0, z0 = (r[..., i] for i in range(4))
        n = np.sqrt(((w0 * w0 + x0 * x0) + y0 * y0) + z0 * z0)
        w, x, y, z = w0 / n, x0 / n, y0 / n, z0 / n
        fx, fy = 1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y + w * z)
        h2 = fx * fx + fy * fy
        flat = h2 < HEADING_EPS
        h = np.sqrt(h2)
        return np.where(flat, 1.0, fx / h), np.where(flat, 0.0, fy / h)


def half_angle(c, s):
    """(hw, hz) of the contract, before the sign fix: hw >= 0 in both branches."""
    with np.errstate(all="ignore"):
        if c < 0.0:
            m = np.sqrt((1.0 - c) * 0.5)
            return np.abs(s) / (2.0 * m), (-m if s < 0.0 else m)
        hw = np.sqrt((1.0 + c) * 0.5)
        return hw, s / (2.0 * hw)


def place_quat(hw, hz, r):
    w, x, y, z = (r[..., i] for i in range(4))
    return np.stack([hw * w - hz * z, hw * x - hz * y, hw * y + hz * x, hw * z + hz * w], -1)


def place(T, rows, first):
    """Rows [n, nq] placed by T = (c, s, tx, ty, hw, hz); a chain's first segment is used without arithmetic."""
    out = np.array(rows, dtype=np.float64)
    if first:
        return out
    c, s, tx, ty, hw, hz = T
    with np.errstate(all="ignore"):
        px, py = rows[:, 0], rows[:, 1]
        out[:, 0] = (c * px - s * py) + tx
        out[:, 1] = (s * px + c * py) + ty
        out[:, 3:7] = place_quat(hw, hz, rows[:, 3:7])
    return out


def slerp(q0, q1, a):
    """track_slerp (gmr_amd/csrc/track_kernel.hip.h) on xyzw rows [n, 4], a [n]."""
    with np.errstate(all="ignore"):
        d = q0[:, 0] * q1[:, 0] + q0[:, 1] * q1[:, 1] + q0[:, 2] * q1[:, 2] + q0[:, 3] * q1[:, 3]
        neg = d < 0.0
        q1 = np.where(neg[:, None], -q1, q1)
        d = np.where(neg, -d, d)
        om = np.arccos(np.fmin(d, 1.0))
        small = om < 1e-8
        s = np.sin(om)
        w0 = np.where(small, 1.0 - a, np.sin((1.0 - a) * om) / s)
        w1 = np.where(small, a, np.sin(a * om) / s)
        r = w0[:, None] * q0 + w1[:, None] * q1
        n = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
        return r / n[:, None]


def clamp_rows(r, n):
    return np.clip(np.asarray(r, dtype=np.int64), 0, n - 1)


def transforms(plan, q):
    """seg_transform [n_seg, 6] of the contract, composed sequentially per output clip."""
    N = q.shape[0]
    T = np.zeros((plan.n_seg, 6))
    with np.errstate(all="ignore"):
        for o in range(plan.n_out):
            k0, k1 = int(plan.clip_segs[o]), int(plan.clip_segs[o + 1])
            c, s, tx, ty, hw, hz = IDENTITY
            for k in range(k0, k1):
                if k == k0:
                    c, s, tx, ty, hw, hz = IDENTITY
                else:
                    B = int(plan.seg_blend[k])
                    a = B // 2
                    va = q[int(clamp_rows(int(plan.seg_src[k - 1]) + int(plan.seg_len[k - 1]) - B + a, N))]
                    vb = q[int(clamp_rows(int(plan.seg_src[k]) + a, N))]
                    ca, sa = (float(v) for v in heading(va[3:7]))
                    cb, sb = (float(v) for v in heading(vb[3:7]))
                    cd = ca * cb + sa * sb
                    sd = sa * cb - ca * sb
                    tdx = va[0] - (cd * vb[0] - sd * vb[1])
                    tdy = va[1] - (sd * vb[0] + cd * vb[1])
                    qa = place_quat(hw, hz, va[3:7])
                    nx, ny = (c * tdx - s * tdy) + tx, (s * tdx + c * tdy) + ty
                    c1, s1 = c * cd - s * sd, s * cd + c * sd
                    n = np.sqrt(c1 * c1 + s1 * s1)
                    c, s, tx, ty = c1 / n, s1 / n, nx, ny
                    hw, hz = half_angle(c, s)
                    qb = place_quat(hw, hz, vb[3:7])
                    if ((qa[0] * qb[0] + qa[1] * qb[1]) + qa[2] * qb[2]) + qa[3] * qb[3] < 0.0:
                        hw, hz = -hw, -hz
                T[k] = (c, s, tx, ty, hw, hz)
    return T


def compose(plan, q, fill=None, T=None):
    """(qpos_out [n_out_frames, nq], seg_transform [n_seg, 6]); rows no segment writes hold ``fill`` (None: 0)."""
    N = q.shape[0]
    T = transforms(plan, q) if T is None else T
    out = np.full((plan.n_out_frames, q.shape[1]), 0.0 if fill is None else fill)
    with np.errstate(all="ignore"):
        for o in range(plan.n_out):
            k0, k1 = int(plan.clip_segs[o]), int(plan.clip_segs[o + 1])
            for k in range(k0, k1):
                src, L, B, dst = int(plan.seg_src[k]), int(plan.seg_len[k]), int(plan.seg_blend[k]), int(plan.seg_out[k])
                nxt = int(plan.seg_blend[k + 1]) if k + 1 < k1 else 0
                W = L - nxt
                own = place(T[k], q[clamp_rows(src + np.arange(W), N)], k == k0)
                if B:
                    j = np.arange(B)
                    prev = place(T[k - 1], q[clamp_rows(int(plan.seg_src[k - 1]) + int(plan.seg_len[k - 1]) - B + j, N)], k - 1 == k0)
                    u = (j + 1).astype(np.float64) / float(B + 1)
                    w = (u * u) * (3.0 - 2.0 * u)
                    x0, x1 = prev, own[:B]
                    mix = x0 + w[:, None] * (x1 - x0)
                    mix[:, 3:7] = slerp(x0[:, [4, 5, 6, 3]], x1[:, [4, 5, 6, 3]], w)[:, [3, 0, 1, 2]]
                    own[:B] = mix
                rows = dst + np.arange(W)
                ok = (rows >= 0) & (rows < plan.n_out_frames)
                out[rows[ok]] = own[ok]
    return out, T


def quat_angle(a, b):
    """The rotation angle between unit-ish wxyz quaternion rows, sign-free: 2 atan2(|a x b part|, |a . b|) in radians."""
    a = a / np.linalg.norm(a, axis=-1, keepdims=True)
    b = b / np.linalg.norm(b, axis=-1, keepdims=True)
    d = np.abs(np.sum(a * b, axis=-1))
    e = np.minimum(np.linalg.norm(a - b, axis=-1), np.linalg.norm(a + b, axis=-1))
    return 2.0 * np.arctan2(e * np.sqrt(np.maximum(1.0 - 0.25 * e * e, 0.0)), d)


# ------------------------------------------------------------------ 50 digits
def _mpv(row):
    return [mpf(float(v)) for v in row]


def _mp_qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return [aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
            aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw]


def mp_heading(r):
    w, x, y, z = r
    n = mp.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    fx, fy = 1 - 2 * (y * y + z * z), 2 * (x * y + w * z)
    return mpf(0) if fx * fx + fy * fy < mpf(HEADING_EPS) else mp.atan2(fy, fx)


def _mp_place(theta, t, row):
    p = [mp.cos(theta) * row[0] - mp.sin(theta) * row[1] + t[0], mp.sin(theta) * row[0] + mp.cos(theta) * row[1] + t[1], row[2]]
    return p + _mp_qmul([mp.cos(theta / 2), mpf(0), mpf(0), mp.sin(theta / 2)], row[3:7]) + list(row[7:])


def _mp_slerp(q0, q1, a):
    """The shortest-arc slerp of two wxyz quaternions, normalised."""
    n0, n1 = mp.sqrt(sum(v * v for v in q0)), mp.sqrt(sum(v * v for v in q1))
    q0, q1 = [v / n0 for v in q0], [v / n1 for v in q1]
    d = sum(x * y for x, y in zip(q0, q1))
    if d < 0:
        q1, d = [-v for v in q1], -d
    om = mp.acos(min(d, mpf(1)))
    if om < mpf(10) ** -30:
        r = [(1 - a) * x + a * y for x, y in zip(q0, q1)]
    else:
        r = [(mp.sin((1 - a) * om) * x + mp.sin(a * om) * y) / mp.sin(om) for x, y in zip(q0, q1)]
    n = mp.sqrt(sum(v * v for v in r))
    return [v / n for v in r]


def mp_compose(plan, q, o):
    """Output clip o as mpf rows (lists of nq) and its segments' (theta, tx, ty), float64 inputs taken as exact.  The quaternion's
    overall sign per segment is the float64 contract's business (a dot product's sign): compare quaternions sign-free."""
    k0, k1 = int(plan.clip_segs[o]), int(plan.clip_segs[o + 1])
    rows, maps = {}, []
    theta, t = mpf(0), [mpf(0), mpf(0)]
    for k in range(k0, k1):
        src, L, B, dst = int(plan.seg_src[k]), int(plan.seg_len[k]), int(plan.seg_blend[k]), int(plan.seg_out[k])
        if k > k0:
            a = B // 2
            va = _mpv(q[int(plan.seg_src[k - 1]) + int(plan.seg_len[k - 1]) - B + a])
            vb = _mpv(q[src + a])
            d = mp_heading(va[3:7]) - mp_heading(vb[3:7])
            td = [va[0] - (mp.cos(d) * vb[0] - mp.sin(d) * vb[1]), va[1] - (mp.sin(d) * vb[0] + mp.cos(d) * vb[1])]
            t = [mp.cos(theta) * td[0] - mp.sin(theta) * td[1] + t[0], mp.sin(theta) * td[0] + mp.cos(theta) * td[1] + t[1]]
            theta = theta + d
        maps.append((theta, t))
        nxt = int(plan.seg_blend[k + 1]) if k + 1 < k1 else 0
        for j in range(L - nxt):
            x1 = _mp_place(theta, t, _mpv(q[src + j]))
            if j < B:
                th0, t0 = maps[-2]
                x0 = _mp_place(th0, t0, _mpv(q[int(plan.seg_src[k - 1]) + int(plan.seg_len[k - 1]) - B + j]))
                u = mpf(j + 1) / mpf(B + 1)
                w = u * u * (3 - 2 * u)
                mix = [a0 + w * (a1 - a0) for a0, a1 in zip(x0, x1)]
                mix[3:7] = _mp_slerp(x0[3:7], x1[3:7], w)
                x1 = mix
            rows[dst + j] = x1
    return rows, maps


def measure_floor(plan, q, o, got=None):
    """Worst distance of ``compose`` (or ``got``) to mp_compose on output clip o: {"pos": metres and hinge radians over the
    columns outside the quaternion, "quat": the largest quaternion component difference on rows outside blends (sign-free),
    "slerp": the largest rotation angle between the two on blended rows}."""
    got = compose(plan, q)[0] if got is None else got
    want, _ = mp_compose(plan, q, o)
    blended = plan.blended_rows()
    worst = {"pos": 0.0, "quat": 0.0, "slerp": 0.0}
    for r, row in want.items():
        g = [mpf(float(v)) for v in got[r]]
        cols = [0, 1, 2] + list(range(7, len(row)))
        worst["pos"] = max(worst["pos"], max(abs(float(g[c] - row[c])) for c in cols))
        sign = -1 if sum(x * y for x, y in zip(g[3:7], row[3:7])) < 0 else 1
        if blended[r]:
            gn = mp.sqrt(sum(v * v for v in g[3:7]))
            rel = _mp_qmul([g[3] / gn, -g[4] / gn, -g[5] / gn, -g[6] / gn], [sign * v for v in row[3:7]])
            worst["slerp"] = max(worst["slerp"], float(2 * mp.atan2(mp.sqrt(rel[1] ** 2 + rel[2] ** 2 + rel[3] ** 2), abs(rel[0]))))
        else:
            worst["quat"] = max(worst["quat"], max(abs(float(g[3 + i] - sign * row[3 + i])) for i in range(4)))
    return worst

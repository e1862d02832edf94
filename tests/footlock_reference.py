"""The foot locking of gmr_motion_footlock as the contract above gmr_footlock_input in include/gmr_amd.h states it, restated in
numpy: FK from the pack's tree, runs, anchors, ramps, the damped iteration.  No GPU and no library.

Runs, anchors and ramps are plain loops over frames.  The FK and the iteration are written once for one frame and evaluated on
arrays with one element per solved frame: every operation is elementwise, in the contract's order, in the array's dtype --
float64, or numpy.longdouble for the rounding floor (tests/test_footlock_host.py)."""
import numpy as np

JNT_HINGE, JNT_FREE = 1, 2
TILE = 64
DEFAULTS = {"blend_frames": 5, "min_run": 2, "iterations": 8, "damping": 1e-6, "step_cap": 0.2}
FIELDS = ("qpos", "pos", "shift", "runs", "locked_frames", "shift_max", "residual_max", "limit_frames")


# ------------------------------------------------------------------ chains
def paths_and_chains(robot, body_ids):
    """Per column: the bodies from the root's child down to the contact body, and the indices into that path of the hinges that lie
    on no other column's path.  ValueError("EINVAL: ...") / ValueError("EUNSUPPORTED: ...") where the entry refuses."""
    nb = robot.nbody
    ids = [int(b) for b in body_ids]
    if any(b < 0 or b >= nb for b in ids) or len(set(ids)) != len(ids):
        raise ValueError("EINVAL: body id out of range or named twice")
    if robot.planar_base:
        raise ValueError("EUNSUPPORTED: planar base")
    paths = []
    for b in ids:
        p, j = [], b
        while j >= 0 and robot.jnt_type[j] != JNT_FREE:
            p.append(j)
            j = int(robot.parent[j])
        if len(p) > 32:
            raise ValueError("EUNSUPPORTED: path longer than 32 bodies")
        paths.append(p[::-1])
    count = {}
    for p in paths:
        for j in p:
            count[j] = count.get(j, 0) + 1
    chains = [[i for i, j in enumerate(p) if robot.jnt_type[j] == JNT_HINGE and count[j] == 1] for p in paths]
    if any(len(c) < 3 for c in chains):
        raise ValueError("EINVAL: a chain of fewer than 3 hinges")
    if any(len(c) > 16 for c in chains):
        raise ValueError("EUNSUPPORTED: a chain of more than 16 hinges")
    return paths, chains


# ------------------------------------------------------------------ FK, elementwise over frames
def _qmul(a, b):
    return (a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
            a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
            a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0])


def _rot(q, v):
    tx, ty, tz = 2.0 * (q[2] * v[2] - q[3] * v[1]), 2.0 * (q[3] * v[0] - q[1] * v[2]), 2.0 * (q[1] * v[1] - q[2] * v[0])
    return (v[0] + q[0] * tx + (q[2] * tz - q[3] * ty),
            v[1] + q[0] * ty + (q[3] * tx - q[1] * tz),
            v[2] + q[0] * tz + (q[1] * ty - q[2] * tx))


def _root(rows):
    """rows [n, >= 7] -> (x, r): position and the quaternion divided by its norm, tuples of [n] arrays."""
    w, x, y, z = rows[:, 3], rows[:, 4], rows[:, 5], rows[:, 6]
    n = np.sqrt(w * w + x * x + y * y + z * z)
    return (rows[:, 0], rows[:, 1], rows[:, 2]), (w / n, x / n, y / n, z / n)


def _walk(robot, path, root, theta, visit=None):
    """The path's FK from the root pose; theta(i): angles [n] of path element i; visit(i, axis, x, r) behind every hinge."""
    dt = root[0][0].dtype
    x, r = root
    for i, j in enumerate(path):
        bp = tuple(dt.type(v) for v in robot.body_pos[j])
        bq = tuple(dt.type(v) for v in robot.body_quat[j])
        w = _rot(r, bp)
        x = (x[0] + w[0], x[1] + w[1], x[2] + w[2])
        t = _qmul(r, bq)
        if robot.jnt_type[j] == JNT_HINGE:
            ax = tuple(dt.type(v) for v in robot.jnt_axis[j])
            h = dt.type(0.5) * theta(i)
            sn, cs = np.sin(h), np.cos(h)
            r = _qmul(t, (cs, sn * ax[0], sn * ax[1], sn * ax[2]))
            if visit is not None:
                visit(i, ax, x, r)
        else:
            r = t
    return x


def foot_positions(robot, path, qpos):
    """p [n, 3] of the path's last body at the rows' own angles (dtype of qpos)."""
    with np.errstate(all="ignore"):
        x = _walk(robot, path, _root(qpos), lambda i: qpos[:, robot.qpos_adr[path[i]]])
    return np.stack(x, axis=1)


# ------------------------------------------------------------------ runs, anchors, ramps: loops
def runs_loop(L, min_run):
    """[(first, last)] of the maximal runs of L with at least min_run frames."""
    out, k, n = [], 0, len(L)
    while k < n:
        if not L[k]:
            k += 1
            continue
        e = k
        while e + 1 < n and L[e + 1]:
            e += 1
        if e - k + 1 >= min_run:
            out.append((k, e))
        k = e + 1
    return out


def runs_tiled(L, min_run):
    """The same from 64-bit masks per tile of 64 frames and a carry across tiles (how the kernel walks a clip)."""
    out, n = [], len(L)
    open_, start = False, 0
    full = (1 << TILE) - 1
    for k0 in range(0, n, TILE):
        m = 0
        for l in range(min(TILE, n - k0)):
            m |= int(bool(L[k0 + l])) << l
        b = 0
        while b < TILE:
            if not open_:
                rest = (m >> b) << b
                if not rest:
                    break
                b = (rest & -rest).bit_length() - 1
                open_, start = True, k0 + b
            zeros = (((~m) & full) >> b) << b
            eb = (zeros & -zeros).bit_length() - 1 if zeros else TILE
            if eb == TILE:
                break
            if k0 + eb - start >= min_run:
                out.append((start, k0 + eb - 1))
            open_, b = False, eb
    if open_ and n - start >= min_run:
        out.append((start, n - 1))
    return out


def tree_sum(v):
    """Balanced binary tree over 64 values, neighbours first."""
    v = list(v)
    assert len(v) == TILE
    while len(v) > 1:
        v = [v[i] + v[i + 1] for i in range(0, len(v), 2)]
    return v[0]


def anchor(px, py, first, last):
    """Mean of the run's p.x and p.y: per tile of the clip a tree sum with zeros outside the run, tiles added to 0 in order."""
    zero = px.dtype.type(0.0)
    sx, sy = zero, zero
    for k0 in range(first // TILE * TILE, last + 1, TILE):
        ks = range(k0, k0 + TILE)
        sx = sx + tree_sum([px[k] if first <= k <= last else zero for k in ks])
        sy = sy + tree_sum([py[k] if first <= k <= last else zero for k in ks])
    n = px.dtype.type(last - first + 1)
    return sx / n, sy / n


def smooth(t):
    return t * t * (3.0 - 2.0 * t)


def ramp_weights(k, e, f, W, dtype=np.float64):
    """(w-, w+) of frame k outside every run: e / f the nearest run frames before / after, or None."""
    T = np.dtype(dtype).type
    wm = smooth(T(1.0) - T(k - e) / T(W + 1)) if e is not None and k - e <= W else T(0.0)
    wp = smooth(T(1.0) - T(f - k) / T(W + 1)) if f is not None and f - k <= W else T(0.0)
    return wm, wp


def shifts(p, L, valid, W, min_run):
    """One clip, one column.  p [n, 3]; L, valid [n] -> (d [n, 3], solve [n] bool, runs)."""
    n = len(L)
    T = p.dtype.type
    d = np.zeros((n, 3), p.dtype)
    solve = np.zeros(n, bool)
    runs = runs_loop(L, min_run)
    inrun = np.zeros(n, bool)
    for a, b in runs:
        ax, ay = anchor(p[:, 0], p[:, 1], a, b)
        for k in range(a, b + 1):
            d[k, 0], d[k, 1] = ax - p[k, 0], ay - p[k, 1]
        inrun[a:b + 1] = True
        solve[a:b + 1] = True
    ends, starts = [b for _, b in runs], [a for a, _ in runs]
    for k in range(n):
        if inrun[k] or not valid[k]:
            continue
        e = max([x for x in ends if x < k], default=None)
        f = min([x for x in starts if x > k], default=None)
        wm, wp = ramp_weights(k, e, f, W, p.dtype)
        if not (wm > 0 or wp > 0):
            continue
        for i in (0, 1):
            t = wm * d[e, i] if wm > 0 else T(0.0)
            u = wp * d[f, i] if wp > 0 else T(0.0)
            den = wm + wp if wm + wp > 1.0 else T(1.0)
            d[k, i] = (t + u) / den
        solve[k] = True
    return d, solve, runs


# ------------------------------------------------------------------ the iteration, elementwise over the solved frames
def solve_frames(robot, path, chain, rows, tgt, iterations, damping, step_cap):
    """rows [n, nq], tgt [n, 3] -> (chain angles [n, nc], residual [n], on_limit [n])."""
    dt = rows.dtype
    T = dt.type
    n = rows.shape[0]
    root = _root(rows)
    ang = [rows[:, robot.qpos_adr[j]].copy() if robot.jnt_type[j] == JNT_HINGE else np.zeros(n, dt) for j in path]
    q0 = [ang[i].copy() for i in chain]
    inf = T(np.inf)
    lo = [T(robot.jnt_range[path[i], 0]) if robot.jnt_limited[path[i]] else -inf for i in chain]
    hi = [T(robot.jnt_range[path[i], 1]) if robot.jnt_limited[path[i]] else inf for i in chain]
    lw = [np.where(lo[c] < q0[c], lo[c], q0[c]) for c in range(len(chain))]
    hw = [np.where(hi[c] > q0[c], hi[c], q0[c]) for c in range(len(chain))]
    lam, cap = T(damping), T(step_cap)
    for _ in range(iterations):
        p = _walk(robot, path, root, lambda i: ang[i])
        e = (tgt[:, 0] - p[0], tgt[:, 1] - p[1], tgt[:, 2] - p[2])
        J = []

        def visit(i, ax, o, r):
            if i not in chain:
                return
            w = _rot(r, ax)
            l = (p[0] - o[0], p[1] - o[1], p[2] - o[2])
            J.append((w[1] * l[2] - w[2] * l[1], w[2] * l[0] - w[0] * l[2], w[0] * l[1] - w[1] * l[0]))

        _walk(robot, path, root, lambda i: ang[i], visit)
        z = np.zeros(n, dt)
        g00, g10, g11, g20, g21, g22 = z, z, z, z, z, z
        for j in J:
            g00 = g00 + j[0] * j[0]; g10 = g10 + j[1] * j[0]; g11 = g11 + j[1] * j[1]
            g20 = g20 + j[2] * j[0]; g21 = g21 + j[2] * j[1]; g22 = g22 + j[2] * j[2]
        g00, g11, g22 = g00 + lam, g11 + lam, g22 + lam
        l00 = np.sqrt(g00); l10 = g10 / l00; l20 = g20 / l00
        l11 = np.sqrt(g11 - l10 * l10); l21 = (g21 - l20 * l10) / l11
        l22 = np.sqrt(g22 - l20 * l20 - l21 * l21)
        z0 = e[0] / l00; z1 = (e[1] - l10 * z0) / l11; z2 = (e[2] - l20 * z0 - l21 * z1) / l22
        y2 = z2 / l22; y1 = (z1 - l21 * y2) / l11; y0 = (z0 - l10 * y1 - l20 * y2) / l00
        dq = [j[0] * y0 + j[1] * y1 + j[2] * y2 for j in J]
        mx = np.zeros(n, dt)
        for v in dq:
            mx = np.where(np.abs(v) > mx, np.abs(v), mx)
        with np.errstate(all="ignore"):
            scale = np.where(mx > cap, cap / np.where(mx > 0, mx, T(1.0)), T(1.0))
        for c, i in enumerate(chain):
            q = ang[i] + scale * dq[c]
            ang[i] = np.where(q < lw[c], lw[c], np.where(q > hw[c], hw[c], q))
    p = _walk(robot, path, root, lambda i: ang[i])
    ex, ey, ez = tgt[:, 0] - p[0], tgt[:, 1] - p[1], tgt[:, 2] - p[2]
    res = np.sqrt(ex * ex + ey * ey + ez * ez)
    on = np.zeros(n, bool)
    for c, i in enumerate(chain):
        on |= (np.isfinite(lo[c]) & (ang[i] == lw[c])) | (np.isfinite(hi[c]) & (ang[i] == hw[c]))
    return np.stack([ang[i] for i in chain], axis=1), res, on


# ------------------------------------------------------------------ the whole call
def footlock(robot, qpos, seq_offsets, contact, body_ids, blend_frames=5, min_run=2, iterations=8, damping=1e-6, step_cap=0.2,
             dtype=np.float64):
    """The outputs of gmr_motion_footlock by name (FIELDS), computed in ``dtype``; plus ``run_list[s][c]``: [(first, last)]."""
    qpos = np.asarray(qpos, dtype=np.float64)
    N, nq = qpos.shape
    Cn = len(body_ids)
    paths, chains = paths_and_chains(robot, body_ids)
    contact = np.asarray(contact).reshape(N, Cn)
    S = len(seq_offsets) - 1
    q = qpos.astype(dtype)
    out = {"qpos": q.copy(), "pos": np.zeros((N, Cn, 3), dtype), "shift": np.zeros((N, Cn, 3), dtype),
           "runs": np.zeros((S, Cn), np.int32), "locked_frames": np.zeros((S, Cn), np.int32), "shift_max": np.zeros((S, Cn), dtype),
           "residual_max": np.zeros((S, Cn), dtype), "limit_frames": np.zeros((S, Cn), np.int32), "run_list": [[None] * Cn for _ in range(S)]}
    valid_all = np.isfinite(qpos).all(axis=1)
    for s in range(S):
        a = min(max(int(seq_offsets[s]), 0), N)
        b = min(max(int(seq_offsets[s + 1]), a), N)
        valid = valid_all[a:b]
        for c in range(Cn):
            p = foot_positions(robot, paths[c], q[a:b])
            p[~valid] = np.nan
            out["pos"][a:b, c] = p
            L = (contact[a:b, c] != 0) & valid
            d, solve, runs = shifts(p, L, valid, blend_frames, min_run)
            out["shift"][a:b, c] = d
            out["runs"][s, c] = len(runs)
            out["locked_frames"][s, c] = sum(e - f + 1 for f, e in runs)
            out["run_list"][s][c] = runs
            ks = np.flatnonzero(solve)
            if ks.size == 0:
                continue
            out["shift_max"][s, c] = np.sqrt((d[ks, 0] * d[ks, 0] + d[ks, 1] * d[ks, 1]).max())
            tgt = np.stack([p[ks, 0] + d[ks, 0], p[ks, 1] + d[ks, 1], p[ks, 2]], axis=1)
            ang, res, on = solve_frames(robot, paths[c], chains[c], q[a:b][ks], tgt, iterations, damping, step_cap)
            for n, i in enumerate(chains[c]):
                out["qpos"][a + ks, robot.qpos_adr[paths[c][i]]] = ang[:, n]
            out["residual_max"][s, c] = res.max()
            out["limit_frames"][s, c] = int(on.sum())
    return out

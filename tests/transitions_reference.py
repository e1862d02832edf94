"""The transition search: the contract above gmr_transitions_input (include/gmr_amd.h) restated twice, without a GPU and without
native code.

(1) numpy float64 in the contract's operation order (`points`, `row_moments`, `window_moments`, `grams`, `pair_costs`, `search`):
    given the same points the kernels must equal it bit for bit.
(2) mpmath at 50 digits: `mp_cost`, the closed form of the definition, and `mp_brute`, which knows no closed form for the angle: it
    evaluates mean_k sum_p w_p |a - (R b + t)|^2 directly, the shift at its closed-form optimum t = mean(a) - R mean(b), on a grid
    of angles and then by golden-section refinement.

The bound of (1) against (2) has the form c eps P L (1 + R^2), R the largest |xy| among the points used.  C_MEASURED is the worst
ratio over tests/test_transitions_host.py's cases, measured on the CPU (x86-64, numpy float64) and rounded up; the tests allow four
times it, so that a change of summation order shows and rounding noise does not.  Nothing in it was measured on a kernel.
"""
import numpy as np
from mpmath import mp, mpf

from tests import dynamics_reference as R

mp.dps = 50

EPS = float(np.finfo(np.float64).eps)
C_MEASURED = 0.13        # worst |numpy - 50 digits| / (eps P L (1 + R^2)); re-measured by tests/test_transitions_host.py
FACTOR = 4.0


def bound(P, L, radius):
    """The largest admissible |cost - 50-digit cost|."""
    return FACTOR * C_MEASURED * EPS * P * L * (1.0 + radius * radius)


def clip_rows(offs, s, n):
    a = min(max(int(offs[s]), 0), n)
    return a, min(max(int(offs[s + 1]), a), n)


# ------------------------------------------------------------------ numpy float64
def points(rob, q, offs, body_ids):
    """[N, P, 3]: the bodies' positions, each clip's first-row root (x, y) subtracted; rows outside every clip are NaN."""
    q = np.asarray(q, dtype=np.float64)
    out = np.full((q.shape[0], len(body_ids), 3), np.nan)
    with np.errstate(all="ignore"):
        X = R.fk(rob, q)[0][:, np.asarray(body_ids)]
        for s in range(len(offs) - 1):
            a, b = clip_rows(offs, s, q.shape[0])
            if b > a:
                out[a:b] = X[a:b]
                out[a:b, :, 0] = X[a:b, :, 0] - q[a, 0]
                out[a:b, :, 1] = X[a:b, :, 1] - q[a, 1]
    return out


def row_moments(pts, w):
    """[N, 3] = (m.x, m.y, q): sums over the points in ascending order, from 0."""
    m = np.zeros((pts.shape[0], 3))
    with np.errstate(all="ignore"):
        for p in range(pts.shape[1]):
            x, y = pts[:, p, 0], pts[:, p, 1]
            m[:, 0] = m[:, 0] + w[p] * x
            m[:, 1] = m[:, 1] + w[p] * y
            m[:, 2] = m[:, 2] + w[p] * (x * x + y * y)
    return m


def window_moments(m, L):
    """[T - L + 1, 3] = (M.x, M.y, V) of one clip's rows m [T, 3]."""
    n = m.shape[0] - L + 1
    if n <= 0:
        return np.zeros((0, 3))
    s = np.zeros((n, 3))
    with np.errstate(all="ignore"):
        for k in range(L):
            s = s + m[k:k + n]
        s = s / float(L)
        return np.stack([s[:, 0], s[:, 1], s[:, 2] - (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1])], -1)


def moments(pts, w, offs, L):
    """[N, 6] as the library's `moments`; what it does not write is NaN."""
    out = np.full((pts.shape[0], 6), np.nan)
    m = row_moments(pts, w)
    for s in range(len(offs) - 1):
        a, b = clip_rows(offs, s, pts.shape[0])
        out[a:b, :3] = m[a:b]
        wm = window_moments(m[a:b], L)
        out[a:a + wm.shape[0], 3:] = wm
    return out


def grams(A, B, w):
    """(Gd, Gc, Gz) [TA, TB] of the rows of two clips' points [T, P, 3]."""
    gd, gc, gz = (np.zeros((A.shape[0], B.shape[0])) for _ in range(3))
    with np.errstate(all="ignore"):
        for p in range(A.shape[1]):
            xf, yf, zf = (A[:, p, c][:, None] for c in range(3))
            xg, yg, zg = (B[:, p, c][None, :] for c in range(3))
            dz = zf - zg
            gd = gd + w[p] * (xf * xg + yf * yg)
            gc = gc + w[p] * (xf * yg - yf * xg)
            gz = gz + w[p] * (dz * dz)
    return gd, gc, gz


def pair_terms(A, B, w, L):
    """(V_i [ni, 1], V_j [1, nj], D, C, Z [ni, nj]) of every window of A against every window of B."""
    ni, nj = A.shape[0] - L + 1, B.shape[0] - L + 1
    if ni <= 0 or nj <= 0:
        z = np.zeros((max(ni, 0), max(nj, 0)))
        return np.zeros((max(ni, 0), 1)), np.zeros((1, max(nj, 0))), z, z, z
    gd, gc, gz = grams(A, B, w)
    wa, wb = window_moments(row_moments(A, w), L), window_moments(row_moments(B, w), L)
    sd, sc, sz = (np.zeros((ni, nj)) for _ in range(3))
    with np.errstate(all="ignore"):
        for k in range(L):
            sd, sc, sz = sd + gd[k:k + ni, k:k + nj], sc + gc[k:k + ni, k:k + nj], sz + gz[k:k + ni, k:k + nj]
        mix, miy, mjx, mjy = wa[:, 0][:, None], wa[:, 1][:, None], wb[:, 0][None, :], wb[:, 1][None, :]
        D = sd / float(L) - (mix * mjx + miy * mjy)
        C = sc / float(L) - (mix * mjy - miy * mjx)
        return wa[:, 2][:, None], wb[:, 2][None, :], D, C, sz / float(L)


def pair_costs(A, B, w, L):
    """[TA - L + 1, TB - L + 1]: the cost of every window of A against every window of B."""
    vi, vj, D, C, Z = pair_terms(A, B, w, L)
    with np.errstate(all="ignore"):
        cost = ((vi + vj) - 2.0 * np.sqrt(D * D + C * C)) + Z
        return np.where(cost < 0.0, 0.0, cost)   # (a NaN stays)


def first_minimum(cost, allowed):
    """(minimum, lowest index at it) over the entries that are allowed and not NaN; (+inf, -1) when there is none."""
    ok = allowed & ~np.isnan(cost)
    if not ok.any():
        return np.inf, -1
    c = np.where(ok, cost, np.inf)
    m = c[ok].min()
    return m, int(np.flatnonzero(ok & (c == m))[0])


def search(pts, w, offs, L, src, src_offs, stride, dst, dst_offs, min_gap):
    """(cost_out [E, n_targets], best_cost [E, D], best_frame [E, D]) from points [N, P, 3]."""
    E, NT = int(src_offs[-1]), int(dst_offs[-1])
    dense, best, frame = np.full((E, NT), np.inf), np.full((E, len(dst)), np.inf), np.full((E, len(dst)), -1, np.int32)
    for a, ca in enumerate(src):
        a0, a1 = clip_rows(offs, ca, pts.shape[0])
        n = int(src_offs[a + 1] - src_offs[a])
        for b, cb in enumerate(dst):
            b0, b1 = clip_rows(offs, cb, pts.shape[0])
            cost = pair_costs(pts[a0:a1], pts[b0:b1], w, L)[::stride][:n]
            nj = cost.shape[1]
            if n == 0 or nj == 0:
                continue
            i, j = (np.arange(n) * stride)[:, None], np.arange(nj)[None, :]
            allowed = np.ones(cost.shape, bool) if ca != cb else np.abs(j - i) >= min_gap
            dense[src_offs[a]:src_offs[a] + n, dst_offs[b]:dst_offs[b] + nj] = np.where(allowed, cost, np.inf)
            for u in range(n):
                best[src_offs[a] + u, b], frame[src_offs[a] + u, b] = first_minimum(cost[u], allowed[u])
    return dense, best, frame


def best_of_dense(dense, offs, L, src, src_offs, stride, dst, dst_offs, min_gap, n_rows):
    """(best_cost, best_frame) as the row-wise first minimum of a dense matrix (an excluded pair is known by its indices, not by
    its +inf)."""
    E = int(src_offs[-1])
    best, frame = np.full((E, len(dst)), np.inf), np.full((E, len(dst)), -1, np.int32)
    for a, ca in enumerate(src):
        for u in range(int(src_offs[a + 1] - src_offs[a])):
            for b, cb in enumerate(dst):
                row = dense[src_offs[a] + u, dst_offs[b]:dst_offs[b + 1]]
                j = np.arange(row.size)
                allowed = np.ones(row.size, bool) if ca != cb else np.abs(j - u * stride) >= min_gap
                best[src_offs[a] + u, b], frame[src_offs[a] + u, b] = first_minimum(row, allowed)
    return best, frame


# ------------------------------------------------------------------ 50 digits
def _mp_pts(A):
    return [[[mpf(float(v)) for v in pt] for pt in row] for row in A]


def _mp_weights(w, normalise):
    w = [mpf(float(v)) for v in w]
    return [v / sum(w) for v in w] if normalise else w


def mp_cost(A, B, w, normalise=False):
    """(cost, D, C) of the definition's closed form on windows A, B [L, P, 3] (float64 values taken exactly), weights as given --
    or, with ``normalise``, divided by their 50-digit sum: the closed form is the minimum only for weights that sum to 1, and
    float64 weights do so to an epsilon."""
    A, B, w = _mp_pts(A), _mp_pts(B), _mp_weights(w, normalise)
    L, P = len(A), len(w)
    mean = lambda f: sum(sum(w[p] * f(k, p) for p in range(P)) for k in range(L)) / L   # noqa: E731
    Ma = (mean(lambda k, p: A[k][p][0]), mean(lambda k, p: A[k][p][1]))
    Mb = (mean(lambda k, p: B[k][p][0]), mean(lambda k, p: B[k][p][1]))
    Qa = mean(lambda k, p: A[k][p][0] ** 2 + A[k][p][1] ** 2)
    Qb = mean(lambda k, p: B[k][p][0] ** 2 + B[k][p][1] ** 2)
    D = mean(lambda k, p: A[k][p][0] * B[k][p][0] + A[k][p][1] * B[k][p][1]) - (Ma[0] * Mb[0] + Ma[1] * Mb[1])
    C = mean(lambda k, p: A[k][p][0] * B[k][p][1] - A[k][p][1] * B[k][p][0]) - (Ma[0] * Mb[1] - Ma[1] * Mb[0])
    Z = mean(lambda k, p: (A[k][p][2] - B[k][p][2]) ** 2)
    cost = (Qa - (Ma[0] ** 2 + Ma[1] ** 2)) + (Qb - (Mb[0] ** 2 + Mb[1] ** 2)) - 2 * mp.sqrt(D * D + C * C) + Z
    return max(cost, mpf(0)), D, C


def mp_objective(A, B, w, theta):
    """mean_k sum_p w_p |a - (R(theta) b + t)|^2 at the best shift t = mean(a) - R mean(b), evaluated point by point."""
    L, P = len(A), len(w)
    c, s = mp.cos(theta), mp.sin(theta)
    rb = [[(c * B[k][p][0] - s * B[k][p][1], s * B[k][p][0] + c * B[k][p][1], B[k][p][2]) for p in range(P)] for k in range(L)]
    W = sum(w) * L
    t = [sum(w[p] * (A[k][p][i] - rb[k][p][i]) for k in range(L) for p in range(P)) / W for i in range(2)]
    return sum(w[p] * ((A[k][p][0] - rb[k][p][0] - t[0]) ** 2 + (A[k][p][1] - rb[k][p][1] - t[1]) ** 2 + (A[k][p][2] - rb[k][p][2]) ** 2)
               for k in range(L) for p in range(P)) / L


def mp_brute(A, B, w, grid=360, refine=80, normalise=False):
    """(minimum, angle at it) by brute force: a float64 grid of angles to bracket, then golden section in 50 digits."""
    A64, B64, w64 = np.asarray(A, float), np.asarray(B, float), np.asarray(w, float)

    def f64(th):
        c, s = np.cos(th), np.sin(th)
        rb = np.stack([c * B64[..., 0] - s * B64[..., 1], s * B64[..., 0] + c * B64[..., 1], B64[..., 2]], -1)
        t = np.sum(w64[None, :, None] * (A64 - rb), axis=(0, 1)) / (w64.sum() * A64.shape[0])
        t[2] = 0.0
        return float(np.sum(w64[None, :] * np.sum((A64 - rb - t) ** 2, axis=-1)) / A64.shape[0])
    ths = -np.pi + 2.0 * np.pi * np.arange(grid) / grid
    k = int(np.argmin([f64(th) for th in ths]))
    step = mpf(2) * mp.pi / grid
    Am, Bm, wm = _mp_pts(A), _mp_pts(B), _mp_weights(w, normalise)
    lo, hi = mpf(float(ths[k])) - step, mpf(float(ths[k])) + step
    g = (mp.sqrt(5) - 1) / 2
    x1, x2 = hi - g * (hi - lo), lo + g * (hi - lo)
    f1, f2 = mp_objective(Am, Bm, wm, x1), mp_objective(Am, Bm, wm, x2)
    for _ in range(refine):
        if f1 < f2:
            hi, x2, f2 = x2, x1, f1
            x1 = hi - g * (hi - lo)
            f1 = mp_objective(Am, Bm, wm, x1)
        else:
            lo, x1, f1 = x1, x2, f2
            x2 = lo + g * (hi - lo)
            f2 = mp_objective(Am, Bm, wm, x2)
    th = (lo + hi) / 2
    return mp_objective(Am, Bm, wm, th), th


# ------------------------------------------------------------------ the host tests' cases
CASES = [(P, L) for P in (1, 3, 30) for L in (1, 2, 8)]


def case(P, L, seed=0):
    """(A, B [L, P, 3], w [P] summing to 1, R): two random windows up to 50 m from the clip origin, B a noisy turned copy of A in
    part so that the minimum is neither 0 nor far from it."""
    rng = np.random.default_rng(1000 * P + 10 * L + seed)
    scale = (1.0, 7.0, 35.0)[(P + L + seed) % 3]
    A = rng.uniform(-1.0, 1.0, (L, P, 3)) * scale
    th = rng.uniform(-np.pi, np.pi)
    c, s = np.cos(th), np.sin(th)
    B = np.stack([c * A[..., 0] + s * A[..., 1], -s * A[..., 0] + c * A[..., 1], A[..., 2]], -1) + rng.normal(size=A.shape) * 0.1 * scale
    B[..., :2] += rng.uniform(-0.4, 0.4, 2) * scale
    w = rng.uniform(0.2, 1.0, P)
    w = w / w.sum()
    radius = float(max(np.hypot(A[..., 0], A[..., 1]).max(), np.hypot(B[..., 0], B[..., 1]).max()))
    if radius > 50.0:
        A, B, radius = A * (49.0 / radius), B * (49.0 / radius), 49.0
        radius = float(max(np.hypot(A[..., 0], A[..., 1]).max(), np.hypot(B[..., 0], B[..., 1]).max()))
    return A, B, w, radius

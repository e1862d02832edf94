"""The numpy restatement of gmr_motion_retime_plan and gmr_motion_retime_apply (the contract above gmr_retime_plan_input in
include/gmr_amd.h), in the contract's order of operations.  No GPU and no torch are needed here.

  plan    need, ticks, cum, out_len, clip_stats, need_max: the kernels must equal it bit for bit (max, min, one product and one
          quotient per hinge, a sum in ascending order, a quotient, a product by 1024 and a ceil: IEEE operations numpy and the GPU
          round alike; everything behind ticks is integer).
  apply   qpos_out and src_time: bit for bit everywhere except the root quaternion of rows with u != 0 whose two source quaternions
          differ, where the slerp's acos / sin belong to two libms (compose_reference.SLERP_RAD).
  bound   the property's b: how far above 1 the rounding of one lerp can put |dq| fps / vmax of an output interval.
"""
import numpy as np

from tests import compose_reference as CR

Q = 1024
EPS = CR.EPS
NAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]


def clip_rows(offs, s, N):
    a = min(max(int(offs[s]), 0), N)
    b = min(max(int(offs[s + 1]), a), N)
    return a, b


def stretches(need, max_stretch):
    """s of the contract for the needs of one clip's intervals: a non-finite interval stretches as 1."""
    with np.errstate(invalid="ignore"):
        fin = need < np.inf
        return np.where(fin, np.minimum(np.maximum(1.0, np.where(fin, need, 1.0)), max_stretch), 1.0)


def window_max(s, W):
    n = s.size
    return np.array([s[max(i - W, 0):min(i + W, n - 1) + 1].max() for i in range(n)]) if n else s.copy()


def window_mean(d, W):
    """The sum over [i-W, i+W] inside the clip in ascending order, starting from the first term, over the number of terms."""
    n = d.size
    acc, cnt = np.zeros(n), np.zeros(n, dtype=np.int64)
    idx = np.arange(n)
    for j in range(-W, W + 1):
        k = idx + j
        ok = (k >= 0) & (k < n)
        term = d[np.clip(k, 0, max(n - 1, 0))] if n else d
        acc = np.where(ok & (cnt == 0), term, np.where(ok, acc + term, acc))
        cnt = cnt + ok
    return acc / cnt.astype(np.float64) if n else acc


def plan(q, offs, fps, vmax, window, max_stretch):
    """dict(need [N] f64, ticks [N] i64, cum [N] i64, out_len [S] i64, clip_stats [S, 4] i64, need_max [S] f64); rows outside every
    clip hold 0."""
    q = np.asarray(q, dtype=np.float64)
    vmax = np.asarray(vmax, dtype=np.float64)
    N, S, W = q.shape[0], len(offs) - 1, int(window)
    fps, cap = np.float64(fps), np.float64(max_stretch)
    need, ticks, cum = np.zeros(N), np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    out_len, stats, need_max = np.zeros(S, dtype=np.int64), np.zeros((S, 4), dtype=np.int64), np.zeros(S)
    with np.errstate(all="ignore"):
        for s in range(S):
            a, b = clip_rows(offs, s, N)
            n = b - a
            if n == 0:
                continue
            nd = np.zeros(n - 1)
            bad = np.zeros(n - 1, dtype=bool)
            if vmax.size and n > 1:
                per = (np.abs(q[a + 1:b, 7:] - q[a:b - 1, 7:]) * fps) / vmax[None, :]
                bad = np.any(~(per < np.inf), axis=1)
                nd = np.where(bad, NAN, np.max(np.where(per < np.inf, per, 0.0), axis=1))
            m = window_mean(window_max(stretches(nd, cap), W), W)
            tk = np.ceil(m * 1024.0).astype(np.int64)
            need[a:b - 1], ticks[a:b - 1] = nd, tk
            cum[a:b] = np.concatenate([[0], np.cumsum(tk)])
            total = int(cum[b - 1])
            out_len[s] = (total + Q - 1) // Q + 1
            fin = nd < np.inf
            stats[s] = (np.count_nonzero(fin & (nd > 1.0)), np.count_nonzero(fin & (nd > cap)), np.count_nonzero(~fin), total)
            need_max[s] = nd[fin].max() if fin.any() else 0.0
    return {"need": need, "ticks": ticks, "cum": cum, "out_len": out_len, "clip_stats": stats, "need_max": need_max}


def sample_points(cum, ticks, a, b, rows):
    """(i, u, done) of the output rows ``rows`` of the clip [a, b): done where tau >= total."""
    n = b - a
    tau = np.asarray(rows, dtype=np.int64) * Q
    total = int(cum[b - 1])
    done = (tau >= total) | (n < 2)
    i = np.full(tau.shape, n - 1, dtype=np.int64)
    u = np.zeros(tau.shape)
    if n >= 2 and (~done).any():
        found = np.searchsorted(cum[a:b - 1], tau, side="right") - 1          # the last interval with cum <= tau
        found = np.clip(found, 0, np.minimum(np.asarray(rows, dtype=np.int64), n - 2))
        live = ~done
        i[live] = found[live]
        with np.errstate(all="ignore"):
            u[live] = (tau[live] - cum[a + found[live]]).astype(np.float64) / ticks[a + found[live]].astype(np.float64)
    return i, u, done


def apply(q, offs, ticks, cum, out_offs, n_out, fill=0.0):
    """(qpos_out [n_out, nq], src_time [n_out], slerped [n_out] bool: the rows whose root quaternion went through the slerp); rows no
    clip writes hold ``fill``."""
    q = np.asarray(q, dtype=np.float64)
    N, S = q.shape[0], len(offs) - 1
    out = np.full((n_out, q.shape[1]), fill)
    st = np.full(n_out, fill)
    slerped = np.zeros(n_out, dtype=bool)
    with np.errstate(all="ignore"):
        for s in range(S):
            a, b = clip_rows(offs, s, N)
            oa, ob = clip_rows(out_offs, s, n_out)
            if b == a or ob == oa:
                continue
            i, u, done = sample_points(cum, ticks, a, b, np.arange(ob - oa))
            x0 = q[a + i]
            x1 = q[a + np.where(u != 0.0, np.minimum(i + 1, b - a - 1), i)]
            uu = u[:, None]
            y = np.where(uu == 0.0, x0, x0 + uu * (x1 - x0))
            same = np.all(np.ascontiguousarray(x0[:, 3:7]).view(np.uint64) == np.ascontiguousarray(x1[:, 3:7]).view(np.uint64), axis=1)
            turn = (u != 0.0) & ~same
            y[:, 3:7] = x0[:, 3:7]
            if turn.any():
                y[turn, 3:7] = CR.slerp(x0[turn, 3:7], x1[turn, 3:7], u[turn])   # wxyz as stored
            out[oa:ob], st[oa:ob], slerped[oa:ob] = y, i.astype(np.float64) + u, turn
    return out, st, slerped


def retime(q, offs, fps, vmax, window, max_stretch):
    """Both steps: (plan dict, qpos_out, src_time, out_offsets, slerped)."""
    p = plan(q, offs, fps, vmax, window, max_stretch)
    oo = np.concatenate([[0], np.cumsum(p["out_len"])]).astype(np.int64)
    out, st, sl = apply(q, offs, p["ticks"], p["cum"], oo, int(oo[-1]))
    return p, out, st, oo, sl


def ratios(out, out_offs, fps, vmax):
    """|dq| fps / vmax of every output interval and hinge, per clip: a list of [rows - 1, nh] arrays."""
    res = []
    for s in range(len(out_offs) - 1):
        a, b = int(out_offs[s]), int(out_offs[s + 1])
        res.append(np.abs(np.diff(out[a:b, 7:], axis=0)) * fps / np.asarray(vmax)[None, :] if b - a > 1 else np.zeros((0, len(vmax))))
    return res


def bound(fps, q_abs_max, vmax_min, window, max_stretch):
    """The property's b.  An output interval is Q ticks long and every source interval has at least Q, so an output interval lies
    inside one source interval or spans the row between two.  A piece of dt ticks inside source interval i moves hinge j by
    |slope_ij| dt / ticks_i, and |slope_ij| fps / vmax_j = need_ij <= need_i <= s_i <= m_i <= ticks_i / Q where the interval is
    not capped: in exact arithmetic the two pieces together give |dq| fps / vmax <= (dt_1 + dt_2) / Q = 1.  What rounding adds:
      - each of the two rows is one lerp x0 + u (x1 - x0), u a rounded quotient: a difference, a product and a sum of values of at
        most max|q|, within 4 eps max|q| per row, 8 eps max|q| for the step, times fps / vmax_min; the test's own difference,
        product and quotient add 3 eps to a ratio near 1;
      - need, s, d, m and m 1024 are rounded before the ceil, so ticks_i may fall short of Q need_i by a relative (2 W + 6) eps: 2 W
        additions, a quotient and a product, need's own difference, product and quotient (maxima and minima are exact).
    Derived, not measured."""
    return 8.0 * EPS * q_abs_max * fps / vmax_min + (2.0 * window + 6.0) * EPS + 3.0 * EPS

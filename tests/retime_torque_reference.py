"""The numpy restatement of gmr_motion_retime_plan_torque and of the cubic resampling of gmr_motion_retime_apply (the contracts above
gmr_retime_torque_input and gmr_retime_plan_input in include/gmr_amd.h), in the contracts' order of operations.  No GPU and no
torch are needed here.

  need         per row e, rho, static_over; per interval need.  A difference, a product, a sum, a quotient and a square root per
               element: IEEE operations that numpy rounds correctly.  Whether the GPU's float64 quotient and square root do is what
               tests/test_gpu_retime_torque.py records; it allows need 1 ulp.
  plan_tail    everything behind need -- ticks, cum, out_len, clip_stats, need_max -- with tests/retime_reference's stretches /
               window_max / window_mean, and the end alignment.  Integer behind the ceil: bit for bit from a given need.
  apply_cubic  qpos_out and src_time with retime_reference.sample_points.
"""
import numpy as np

from tests import retime_reference as RR

Q = RR.Q
NAN = RR.NAN
ALIGN_SPAN = 64


def rows(tau, tau_static, torque_limit, limit_scale):
    """(e_max [N], nonfinite [N] bool, static_over [N] int32): the per-row values of the contract."""
    tau, g = np.asarray(tau, dtype=np.float64), np.asarray(tau_static, dtype=np.float64)
    lim = np.asarray(torque_limit, dtype=np.float64)
    N, nh = tau.shape
    if nh == 0:
        return np.zeros(N), np.zeros(N, dtype=bool), np.zeros(N, dtype=np.int32)
    with np.errstate(all="ignore"):
        L = np.float64(limit_scale) * lim
        d = tau - g
        head = np.where(d >= 0.0, L[None, :] - g, L[None, :] + g)
        limited = (lim < np.inf)[None, :]
        e = np.where(limited & (head > 0.0), np.abs(d) / head, 0.0)
        bad = np.any(~(np.abs(tau) < np.inf) | ~(np.abs(g) < np.inf), axis=1)
        emax = np.where(bad, 0.0, np.max(np.where(np.isnan(e), 0.0, e), axis=1))
        over = np.where(bad, 0, np.count_nonzero(limited & (np.abs(g) >= L[None, :]), axis=1)).astype(np.int32)
    return emax, bad, over


def need(tau, tau_static, offs, torque_limit, limit_scale, need_floor=None):
    """(need [N] f64, static_over [N] i32); rows outside every clip hold 0."""
    emax, bad, over = rows(tau, tau_static, torque_limit, limit_scale)
    N = emax.size
    rho = np.sqrt(emax)
    out, so = np.zeros(N), np.zeros(N, dtype=np.int32)
    with np.errstate(all="ignore"):
        for s in range(len(offs) - 1):
            a, b = RR.clip_rows(offs, s, N)
            if b == a:
                continue
            so[a:b] = over[a:b]
            nd = np.maximum(rho[a:b - 1], rho[a + 1:b])
            nf = bad[a:b - 1] | bad[a + 1:b]
            if need_floor is not None:
                fl = np.asarray(need_floor, dtype=np.float64)[a:b - 1]
                nd = np.where(np.isnan(fl), nd, np.maximum(nd, fl))
                nf = nf | ~(fl < np.inf)
            out[a:b - 1] = np.where(nf, NAN, nd)
    return out, so


def align(ticks, cum, n):
    """The end alignment of one clip of n >= 2 rows: (ticks [n - 1], cum [n]) with the total a multiple of Q."""
    ticks, cum = ticks.copy(), cum.copy()
    t = int(cum[n - 1])
    r = (Q - t % Q) % Q
    k = min(n - 1, ALIGN_SPAN)
    if r:
        add = np.full(k, r // k, dtype=np.int64)
        add[:r % k] += 1
        ticks[n - 1 - k:n - 1] += add
        cum[n - k:n] += np.cumsum(add)
    return ticks, cum


def plan_tail(nd_all, offs, window, max_stretch, align_end=True):
    """dict(ticks, cum, out_len, clip_stats, need_max) from need [N] as the entry wrote it: the velocity contract from need on, then
    the alignment."""
    nd_all = np.asarray(nd_all, dtype=np.float64)
    N, S, W, cap = nd_all.size, len(offs) - 1, int(window), np.float64(max_stretch)
    ticks, cum = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    out_len, stats, need_max = np.zeros(S, dtype=np.int64), np.zeros((S, 4), dtype=np.int64), np.zeros(S)
    with np.errstate(all="ignore"):
        for s in range(S):
            a, b = RR.clip_rows(offs, s, N)
            n = b - a
            if n == 0:
                continue
            nd = nd_all[a:b - 1]
            m = RR.window_mean(RR.window_max(RR.stretches(nd, cap), W), W)
            tk = np.ceil(m * 1024.0).astype(np.int64)
            cm = np.concatenate([[0], np.cumsum(tk)]).astype(np.int64)
            if align_end and n >= 2:
                tk, cm = align(tk, cm, n)
            ticks[a:b - 1], cum[a:b] = tk, cm
            total = int(cm[-1])
            out_len[s] = (total + Q - 1) // Q + 1
            fin = nd < np.inf
            stats[s] = (np.count_nonzero(fin & (nd > 1.0)), np.count_nonzero(fin & (nd > cap)), np.count_nonzero(~fin), total)
            need_max[s] = nd[fin].max() if fin.any() else 0.0
    return {"ticks": ticks, "cum": cum, "out_len": out_len, "clip_stats": stats, "need_max": need_max}


def plan(tau, tau_static, offs, torque_limit, limit_scale, window, max_stretch, need_floor=None, align_end=True):
    """The whole entry: dict(need, ticks, cum, out_len, clip_stats, need_max, static_over)."""
    nd, so = need(tau, tau_static, offs, torque_limit, limit_scale, need_floor)
    p = {"need": nd}
    p.update(plan_tail(nd, offs, window, max_stretch, align_end))
    p["static_over"] = so
    return p


def cubic(p0, p1, p2, p3, u):
    m1, m2, c = 0.5 * (p2 - p0), 0.5 * (p3 - p1), p2 - p1
    return p1 + u * (m1 + u * (((3.0 * c - 2.0 * m1) - m2) + u * ((m1 + m2) - 2.0 * c)))


def _dot(a, b):
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]) + a[:, 3] * b[:, 3]


def apply_cubic(q, offs, ticks, cum, out_offs, n_out, fill=0.0):
    """(qpos_out [n_out, nq], src_time [n_out], curved [n_out] bool: the rows with u != 0); rows no clip writes hold ``fill``."""
    q = np.asarray(q, dtype=np.float64)
    N, S = q.shape[0], len(offs) - 1
    out = np.full((n_out, q.shape[1]), fill)
    st = np.full(n_out, fill)
    curved = np.zeros(n_out, dtype=bool)
    with np.errstate(all="ignore"):
        for s in range(S):
            a, b = RR.clip_rows(offs, s, N)
            oa, ob = RR.clip_rows(out_offs, s, n_out)
            if b == a or ob == oa:
                continue
            n = b - a
            i, u, done = RR.sample_points(cum, ticks, a, b, np.arange(ob - oa))
            turn = ~done & (u != 0.0)
            y = q[a + i].copy()
            if turn.any():
                it, uu = i[turn], u[turn][:, None]
                first, last = (it == 0)[:, None], (it + 2 > n - 1)[:, None]
                s0, p1, p2, s3 = q[a + np.maximum(it - 1, 0)].copy(), q[a + it], q[a + it + 1].copy(), q[a + np.minimum(it + 2, n - 1)].copy()
                for p in (s0, p2, s3):   # the stored rows onto row i's hemisphere, before any reflection
                    flip = _dot(p[:, 3:7], p1[:, 3:7]) < 0.0
                    p[flip, 3:7] = -p[flip, 3:7]
                p0 = np.where(first, p1 + (p1 - p2), s0)
                p3 = np.where(last, p2 + (p2 - p1), s3)
                yt = cubic(p0, p1, p2, p3, uu)
                qq = yt[:, 3:7]
                nrm = np.sqrt(((qq[:, 0] * qq[:, 0] + qq[:, 1] * qq[:, 1]) + qq[:, 2] * qq[:, 2]) + qq[:, 3] * qq[:, 3])
                yt[:, 3:7] = qq / nrm[:, None]
                y[turn] = yt
            out[oa:ob], st[oa:ob], curved[oa:ob] = y, i.astype(np.float64) + u, turn
    return out, st, curved


def lengths_to_offsets(out_len):
    return np.concatenate([[0], np.cumsum(out_len)]).astype(np.int64)


def tau_pair(rob, tab, q, offs, fps):
    """(tau, tau_static) of qpos by the dynamics restatement: differenced, and with zero velocity and acceleration."""
    from tests import dynamics_reference as DR
    v, acc = DR.differences(q, offs, fps)
    full = DR.dynamics(rob, tab, q, v, acc)["tau"]
    rest = DR.dynamics(rob, tab, q, np.zeros_like(v), np.zeros_like(acc))["tau"]
    return full, rest


def ratio(tau, torque_limit, offs):
    """Per clip the largest |tau| / limit over frames and hinges with a finite limit."""
    with np.errstate(all="ignore"):
        r = np.where(np.isfinite(torque_limit)[None, :], np.abs(tau) / torque_limit[None, :], 0.0)
    return np.array([r[int(a):int(b)].max() if b > a and r.shape[1] else 0.0 for a, b in zip(offs[:-1], offs[1:])])


def loop(rob, tab, q, offs, fps, limit_scale=0.95, window=12, max_stretch=8.0, passes=4, interp_cubic=True):
    """dataset.retime_to_torque_limits restated: (qpos, offsets, info) with per clip passes, ratios before / after, capped counts
    summed over the passes, and per pass the clips' ratios (``history``) and rows (``rows``) going in."""
    offs = np.asarray(offs, dtype=np.int64)
    S = len(offs) - 1
    used, capped, ratios, rows_of = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64), [], []
    lim = np.asarray(tab.torque_limit, dtype=np.float64)
    for p in range(passes + 1):
        full, rest = tau_pair(rob, tab, q, offs, fps)
        ratios.append(ratio(full, lim, offs))
        rows_of.append(np.diff(offs))
        if p == passes:
            break
        pl = plan(full, rest, offs, lim, limit_scale, window, max_stretch)
        if not pl["clip_stats"][:, 0].any():
            break
        used += pl["clip_stats"][:, 0] > 0
        capped += pl["clip_stats"][:, 1]
        oo = lengths_to_offsets(pl["out_len"])
        if interp_cubic:
            q = apply_cubic(q, offs, pl["ticks"], pl["cum"], oo, int(oo[-1]))[0]
        else:
            q = RR.apply(q, offs, pl["ticks"], pl["cum"], oo, int(oo[-1]))[0]
        offs = oo
    return q, offs, {"passes": used, "capped": capped, "before": ratios[0], "after": ratios[-1], "history": ratios, "rows": rows_of}

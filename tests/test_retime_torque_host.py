"""Retiming to torque limits without a GPU: the contract's crafted cases against the numpy restatement
(tests/retime_torque_reference.py), the end alignment, the cubic resampling, the acceleration fact that asks for it, the loop of
dataset.retime_to_torque_limits restated on the CPU, and the header, exports, binding, layout and static stream check of
gmr_motion_retime_plan_torque."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from tests import retime_reference as RR
from tests import retime_torque_inputs as ti
from tests import retime_torque_reference as TR
from tests.test_stream_order_host import check_api, reachable, stream_prototypes, units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "gmr_motion_retime_plan_torque"
EPS = RR.EPS
INF = np.inf


# ------------------------------------------------------------------ 1: the need, case by case
def one(tau, g, lim, scale=1.0, floor=None, cap=8.0, window=0, align=False):
    """A clip of two equal rows of one hinge: its one interval's (need, ticks, stats row, static_over of row 0)."""
    t, s = np.array([[tau], [tau]], dtype=np.float64), np.array([[g], [g]], dtype=np.float64)
    fl = None if floor is None else np.array([floor, 0.0])
    p = TR.plan(t, s, np.array([0, 2]), np.array([lim], dtype=np.float64), scale, window, cap, fl, align)
    return p["need"][0], int(p["ticks"][0]), p["clip_stats"][0].tolist(), int(p["static_over"][0])


def test_the_crafted_cases_of_the_contract():
    assert one(3.0, 3.0, 10.0) == (0.0, 1024, [0, 0, 0, 1024], 0)                           # d = 0
    assert one(10.0, 2.0, 10.0) == (1.0, 1024, [0, 0, 0, 1024], 0)                          # |tau| = L exactly: need 1, not stretched
    assert one(-10.0, -2.0, 10.0)[0] == 1.0                                                 # ... on the other side
    assert one(34.0, 2.0, 10.0)[:2] == (2.0, 2048)                                          # d = 32 over a head of 8: s^2 = 4
    assert one(-30.0, 2.0, 10.0)[:2] == (np.sqrt(32.0 / 12.0), int(np.ceil(np.sqrt(32.0 / 12.0) * 1024.0)))   # d < 0: head = L + g
    assert one(12.0, 10.0, 10.0) == (0.0, 1024, [0, 0, 0, 1024], 1)                         # head = 0: no need, counted
    assert one(15.0, 12.0, 10.0) == (0.0, 1024, [0, 0, 0, 1024], 1)                         # gravity beyond the limit, the motion hurts
    n, tk, st, over = one(9.0, 12.0, 10.0)                                                  # ... and helps: d = -3, head = 22
    assert (n, tk, over) == (np.sqrt(3.0 / 22.0), 1024, 1)
    assert one(-15.0, -12.0, 10.0)[3] == 1 and one(-9.0, -12.0, 10.0)[0] == np.sqrt(3.0 / 22.0)   # the mirror images
    assert one(1e6, 0.0, INF) == (0.0, 1024, [0, 0, 0, 1024], 0)                            # no limit: no need, no count
    assert one(9.6, 0.0, 10.0, scale=0.95)[0] > 1.0 and one(9.5, 0.0, 10.0, scale=0.95)[0] == 1.0   # the margin scales the limit
    assert one(0.0, 9.5, 10.0, scale=0.95)[3] == 1 and one(0.0, 9.4, 10.0, scale=0.95)[3] == 0      # ... for the static count too
    assert one(34.0, 2.0, 10.0, floor=3.0)[:2] == (3.0, 3072)                               # a floor above
    assert one(34.0, 2.0, 10.0, floor=1.5)[:2] == (2.0, 2048)                               # ... below
    n, tk, st, _ = one(34.0, 2.0, 10.0, floor=np.nan)                                       # ... and NaN: non-finite, stretches as 1
    assert np.isnan(n) and tk == 1024 and st == [0, 0, 1, 1024]
    assert np.isnan(one(34.0, 2.0, 10.0, floor=INF)[0])
    n, tk, st, _ = one(802.0, 2.0, 10.0)                                                    # need 10 above max_stretch 8: capped
    assert (n, tk, st) == (10.0, 8192, [1, 1, 0, 8192])


def test_a_non_finite_row_makes_both_its_intervals_non_finite_and_counts_nothing():
    rng = np.random.default_rng(3)
    tau, g = rng.normal(size=(5, 3)), np.full((5, 3), 20.0)                                  # gravity beyond the limit in every row
    lim = np.array([10.0, 10.0, INF])
    base = TR.plan(tau, g, [0, 5], lim, 1.0, 0, 8.0, None, False)
    assert base["static_over"].tolist() == [2] * 5 and base["clip_stats"][0, 2] == 0
    for arr, col, val in ((0, 1, np.nan), (1, 0, INF), (0, 2, -INF)):                       # the unlimited column too: "any entry"
        t2, g2 = tau.copy(), g.copy()
        (t2 if arr == 0 else g2)[2, col] = val
        p = TR.plan(t2, g2, [0, 5], lim, 1.0, 0, 8.0, None, False)
        assert np.isnan(p["need"][1:3]).all() and np.array_equal(p["need"][[0, 3, 4]], base["need"][[0, 3, 4]])
        assert p["need"][1:3].view(np.uint64).tolist() == [0x7FF8000000000000] * 2
        assert p["static_over"].tolist() == [2, 2, 0, 2, 2] and p["clip_stats"][0, 2] == 2 and p["ticks"][1:3].tolist() == [1024, 1024]


def test_the_row_need_is_one_square_root_of_the_rows_largest_e_and_the_interval_takes_the_larger_row():
    c = ti.case(ti.G1, "lens")
    emax, bad, over = TR.rows(c.tau, c.tau_static, c.limit, c.scale)
    p = ti.reference(ti.G1, "lens")
    assert not bad.any() and over.max() >= 1 and (emax > 64.0).any() and (emax < 1.0).any()   # every branch is in the random case
    a, b = int(ti.OFFS[-2]), int(ti.OFFS[-1])
    assert np.array_equal(p["need"][a:b - 1], np.sqrt(np.maximum(emax[a:b - 1], emax[a + 1:b]))) and p["need"][b - 1] == 0.0
    assert p["clip_stats"][:, 1].sum() > 0 and np.isinf(c.limit).any()
    # the scaling law the need inverts: played s times slower, tau(s) = g + (tau - g) / s^2 meets the scaled limit exactly at s = rho
    j = np.argmax(np.where(np.isfinite(c.limit), np.abs(c.tau[a:b] - c.tau_static[a:b]) / c.limit, 0.0), axis=1)
    r = np.arange(a, b)
    rho = np.sqrt(emax[a:b])
    slow = c.tau_static[r, j] + (c.tau[r, j] - c.tau_static[r, j]) / np.maximum(rho, 1e-3) ** 2
    hit = (rho > 1.0) & (np.abs(c.tau_static[r, j]) < c.scale * c.limit[j])
    assert hit.sum() > 20 and np.all(np.abs(slow[hit]) <= c.scale * c.limit[j][hit] * (1.0 + 8 * EPS))


@pytest.mark.parametrize("model", list(ti.MODELS))
def test_the_inputs_have_the_columns_their_models_promise(model):
    c = ti.case(model, "ragged")
    assert c.tau.shape == (310, ti.MODELS[model]) and c.offs.tolist() == [0, 37, 37, 38, 101, 310]
    p = ti.reference(model, "ragged", True, True)
    assert p["out_len"][1] == 0 and p["out_len"][2] == 1 and np.all(p["clip_stats"][:, 3] % 1024 == 0)
    if ti.MODELS[model] == 0:
        q = ti.reference(model, "ragged", False, True)
        assert not q["need"].any() and q["out_len"].tolist() == [37, 0, 1, 63, 209]           # a model without hinges needs nothing
    from tests import dynamics_reference as DR
    assert DR.model(model)[0].nq - 7 == ti.MODELS[model] and DR.model(model)[0].nq <= 64


# ------------------------------------------------------------------ 2: the end alignment
@pytest.mark.parametrize("intervals", [1, 2, 63, 64, 65])
@pytest.mark.parametrize("r", [0, 1, 1023])
def test_alignment_makes_the_total_whole_frames_over_the_last_intervals(intervals, r):
    n = intervals + 1
    rng = np.random.default_rng(intervals)
    tk = rng.integers(1024, 3000, intervals).astype(np.int64)
    tk[0] += (-int(tk.sum()) - r) % 1024                                                     # the total is r short of whole frames
    cum = np.concatenate([[0], np.cumsum(tk)]).astype(np.int64)
    assert (1024 - int(cum[-1]) % 1024) % 1024 == r
    t2, c2 = TR.align(tk, cum, n)
    k = min(intervals, 64)
    gain = t2 - tk
    assert int(c2[-1]) % 1024 == 0 and int(c2[-1]) == int(cum[-1]) + r and np.array_equal(c2, np.concatenate([[0], np.cumsum(t2)]))
    assert gain.sum() == r and np.all(gain[:intervals - k] == 0) and gain.max() - gain[intervals - k:].min() <= 1
    assert np.all(np.diff(gain[intervals - k:]) <= 0)                                        # the first r % k intervals of the span take the odd ticks
    if intervals >= 64:
        assert gain.max() <= 16
    # the last output row is the final pose at its planned time: u == 0 at src_time n - 1, and the row before it a whole frame earlier
    out_len = int(c2[-1]) // 1024 + 1
    i, u, done = RR.sample_points(c2, np.concatenate([t2, [0]]), 0, n, np.arange(out_len))
    assert done[-1] and not done[:-1].any() and i[-1] == n - 1 and u[-1] == 0.0
    tau_before = (out_len - 2) * 1024
    assert int(c2[-1]) - tau_before == 1024


def test_without_alignment_the_last_row_comes_a_fraction_of_a_frame_after_the_row_before_it():
    c = ti.case(ti.G1, "lens")
    free, snug = ti.reference(ti.G1, "lens", False, False), ti.reference(ti.G1, "lens", False, True)
    assert np.array_equal(free["need"], snug["need"]) and (free["clip_stats"][:, 3] % 1024 != 0).any()
    assert np.all(snug["clip_stats"][:, 3] % 1024 == 0) and np.all(snug["clip_stats"][:, 3] - free["clip_stats"][:, 3] < 1024)
    assert np.array_equal(snug["out_len"], free["out_len"])                                   # the padding fills the last frame, it adds none
    assert (snug["ticks"] - free["ticks"]).max() <= 16 + 1023 * (np.diff(c.offs).min() < 65)
    assert snug["ticks"].max() <= 1024 * c.max_stretch + 1023


# ------------------------------------------------------------------ 3: the cubic resampling
def _poly_clip(n, nq=10, seed=0):
    """Hinges and root position on cubic polynomials of the row index, a constant root quaternion."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)[:, None] / n
    co = rng.uniform(-1, 1, (4, nq))
    q = co[0] + co[1] * t + co[2] * t * t + co[3] * t * t * t
    q[:, 3:7] = [0.5, -0.5, 0.5, 0.5]
    return q, co


def test_a_cubic_polynomial_is_reproduced_in_the_interior():
    """Catmull-Rom tangents are central differences: exact for a quadratic, off by a sixth of the third derivative for a cubic.  So a
    quadratic is reproduced to rounding, and a cubic to rounding once the one term that the tangent errors put through the Hermite
    basis is added: (third derivative / 6) u (1 - u) (1 - 2 u).  Nothing else separates the resampled clip from the polynomial."""
    n = 40
    q, co = _poly_clip(n)
    tk = np.full(n, 1536, dtype=np.int64)
    tk[-1] = 0
    cum = np.concatenate([[0], np.cumsum(tk[:-1])]).astype(np.int64)
    m = int(cum[-1]) // 1024 + 1
    out, st, curved = TR.apply_cubic(q, [0, n], tk, cum, [0, m], m)
    t = st[:, None] / n
    exact = co[0] + co[1] * t + co[2] * t * t + co[3] * t * t * t
    inner = (st >= 1.0) & (st <= n - 2.0)
    cols = [0, 1, 2] + list(range(7, 10))
    assert curved.sum() > 30 and inner.sum() > 45
    u = (st - np.floor(st))[:, None]
    remainder = (co[3] / n ** 3) * u * (1.0 - u) * (1.0 - 2.0 * u)
    assert np.abs(out[inner][:, cols] - (exact + remainder)[inner][:, cols]).max() <= 64 * EPS
    assert np.abs(out[~inner][:, cols] - exact[~inner][:, cols]).max() > 1e-6                 # the end intervals reflect: not exact there
    assert np.array_equal(out[:, 3:7], np.tile(q[0, 3:7], (m, 1)))                            # a constant unit quaternion stays what it is
    quad = q - co[3] * (np.arange(n)[:, None] / n) ** 3
    quad[:, 3:7] = q[:, 3:7]
    out2 = TR.apply_cubic(quad, [0, n], tk, cum, [0, m], m)[0]
    assert np.abs(out2[inner][:, cols] - (co[0] + co[1] * t + co[2] * t * t)[inner][:, cols]).max() <= 64 * EPS


def test_two_rows_give_the_lerp_and_whole_frame_ticks_copy_every_row_bitwise():
    q, _ = _poly_clip(2, seed=1)
    q[1, 3:7] = q[0, 3:7]
    tk, cum = np.array([5000, 0], dtype=np.int64), np.array([0, 5000], dtype=np.int64)
    out, st, curved = TR.apply_cubic(q, [0, 2], tk, cum, [0, 6], 6)
    lerp = RR.apply(q, [0, 2], tk, cum, [0, 6], 6)[0]
    assert curved.tolist() == [False, True, True, True, True, False] and np.abs(out - lerp).max() <= 8 * EPS
    assert np.array_equal(out[0], q[0]) and np.array_equal(out[-1], q[1])
    c = ti.loop_clips()[2][:50]
    tk = np.full(50, 1024, dtype=np.int64)
    tk[-1] = 0
    out, st, curved = TR.apply_cubic(c, [0, 50], tk, np.arange(50, dtype=np.int64) * 1024, [0, 50], 50)
    assert out.tobytes() == np.ascontiguousarray(c).tobytes() and not curved.any() and np.array_equal(st, np.arange(50.0))


def test_the_quaternion_is_flipped_onto_row_i_then_cubed_and_normalised():
    rng = np.random.default_rng(7)
    n = 12
    ang = np.cumsum(rng.uniform(0.05, 0.3, n))
    q = np.zeros((n, 8))
    q[:, 3], q[:, 6] = np.cos(ang / 2), np.sin(ang / 2)
    q[:, 7] = ang
    tk = np.full(n, 2048, dtype=np.int64)
    tk[-1] = 0
    cum = np.concatenate([[0], np.cumsum(tk[:-1])]).astype(np.int64)
    m = int(cum[-1]) // 1024 + 1
    base = TR.apply_cubic(q, [0, n], tk, cum, [0, m], m)[0]
    flipped = q.copy()
    flipped[[0, 4, 5, 9, 11], 3:7] *= -1.0                                                   # the other cover of the same rotations
    got = TR.apply_cubic(flipped, [0, n], tk, cum, [0, m], m)[0]
    sign = np.sign(np.sum(got[:, 3:7] * base[:, 3:7], axis=1))[:, None]
    assert np.abs(got[:, 3:7] * sign - base[:, 3:7]).max() <= 4 * EPS                         # the same rotation, on row i's hemisphere
    assert np.abs(np.linalg.norm(got[:, 3:7], axis=1) - 1.0).max() <= 2 * EPS
    half = np.arctan2(base[:, 6], base[:, 3])
    assert np.abs(2 * half - base[:, 7]).max() < 2e-3                                        # and it follows the hinge that turns with it
    poisoned = q.copy()
    poisoned[5, 4] = np.nan
    out = TR.apply_cubic(poisoned, [0, n], tk, cum, [0, m], m)[0]
    rows = np.flatnonzero(np.isnan(out).any(axis=1))
    # the rows whose stencil reads row 5 -- u != 0 in the intervals 3 .. 6 -- get all four components; row 10 is the copy of row 5
    assert rows.tolist() == [7, 9, 10, 11, 13] and np.isnan(out[[7, 9, 11, 13], 3:7]).all() and np.isnan(out[10]).sum() == 1
    assert np.isfinite(np.delete(out, [3, 4, 5, 6], axis=1)).all()                            # ... and nothing else


# ------------------------------------------------------------------ 4: why a C1 resampler
def test_a_lerp_keeps_the_acceleration_at_the_source_rows_and_the_cubic_does_not():
    """A sine resampled at s = 2, 2.5 and 3: the largest second difference at the output rate times fps^2 falls as a / s for the
    lerp and as a / s^2 for the cubic.  Recorded here (sin(3 pi t) at 30 fps, 120 rows): lerp 44.0, 33.5, 29.4; cubic 22.6, 14.3, 10.1;
    a / s^2 = 22.0, 14.1, 9.8.  (At s = 2.5 the output rows miss the source rows' phase: the lerp's 33.5 is under a / s = 35.2.)"""
    fps, n, amp, om = 30.0, 120, 1.0, 3.0 * np.pi
    t = np.arange(n) / fps
    q = np.zeros((n, 8))
    q[:, 3] = 1.0
    q[:, 7] = amp * np.sin(om * t)
    a0 = np.abs(np.diff(q[:, 7], 2)).max() * fps * fps
    seen = []
    for s in (2.0, 2.5, 3.0):
        tk = np.full(n, int(s * 1024), dtype=np.int64)
        tk[-1] = 0
        cum = np.concatenate([[0], np.cumsum(tk[:-1])]).astype(np.int64)
        m = int(cum[-1]) // 1024 + 1
        lin = RR.apply(q, [0, n], tk, cum, [0, m], m)[0][:, 7]
        cub = TR.apply_cubic(q, [0, n], tk, cum, [0, m], m)[0][:, 7]
        al, ac = np.abs(np.diff(lin, 2)).max() * fps * fps, np.abs(np.diff(cub, 2)).max() * fps * fps   # both over all rows
        seen.append((round(al, 1), round(ac, 1), round(a0 / s ** 2, 1)))
        assert ac < al and ac < 0.5 * (a0 / s + a0 / s ** 2)
        assert al > 0.9 * a0 / s                                                            # the lerp's does fall as a / s only
    print("lerp, cubic, a / s^2:", seen)
    assert seen == [(44.0, 22.6, 22.0), (33.5, 14.3, 14.1), (29.4, 10.1, 9.8)]


# ------------------------------------------------------------------ 5: the loop, restated
def test_the_loop_brings_the_four_g1_clips_under_their_limits():
    """dynamics_reference.Trajectory(G1, seed), seeds 0, 1, 2 and 5, 120 frames at 30 fps, the MJCF torque limits, the defaults
    (0.95 of the limit, window 12, cubic, aligned ends).  Recorded from this run: tau_ratio_max 2.08, 1.70, 1.07, 1.40 going in; at or
    under 1 after 1, 1, 2 and 1 passes, at 0.96, 0.96, 0.95, 0.94 with 147, 137, 128 and 130 rows.  The loop itself goes on while an
    interval needs more than 1 against 0.95 of the limit: 4, 2, 2 and 1 passes, 150, 138, 128 and 130 rows, 0.95, 0.95, 0.95, 0.94.
    This is the condition under which the GPU's end-to-end test may demand convergence."""
    rob, tab, q, offs = ti.loop_clips(quiet=True)
    out, oo, info = TR.loop(rob, tab, q, offs, ti.LOOP_FPS, ti.SCALE, ti.WINDOW, ti.MAX_STRETCH, 4)
    hist, rows = np.array([np.pad(h, (0, 0)) for h in info["history"]]), np.array(info["rows"])
    first = [int(np.argmax(hist[:, s] <= 1.0)) for s in range(5)]
    print("ratios per pass:\n", np.round(hist, 4), "\nrows per pass:\n", rows, "\npasses to <= 1:", first, "passes used:", info["passes"])
    assert np.all(info["after"] <= 1.0) and not info["capped"].any()
    assert np.round(info["before"], 2).tolist() == [2.08, 1.70, 1.07, 1.40, round(float(info["before"][4]), 2)] and info["before"][4] < 0.5
    assert first == [1, 1, 2, 1, 0] and max(first) <= 3
    assert [int(rows[first[s], s]) for s in range(5)] == [147, 137, 128, 130, 40]
    assert np.round([hist[first[s], s] for s in range(4)], 2).tolist() == [0.96, 0.96, 0.95, 0.94]
    assert info["passes"].tolist() == [4, 2, 2, 1, 0] and np.diff(oo).tolist() == [150, 138, 128, 130, 40]
    a = int(oo[4])
    assert out[a:].tobytes() == np.ascontiguousarray(q[int(offs[4]):]).tobytes()             # the quiet clip is copied bit for bit
    for s in range(5):
        assert np.array_equal(out[int(oo[s])], q[int(offs[s])]) and np.array_equal(out[int(oo[s + 1]) - 1], q[int(offs[s + 1]) - 1])


def test_without_alignment_the_clip_end_dominates():
    """Seed 3, one pass against the full limit, window 12, cubic: the abrupt stop of the unaligned end puts the largest torque ratio in
    the last rows; with the alignment the same pass ends at the limit.  Recorded from this run: 2.65 going in; unaligned 4.36 in row
    202 of 204, aligned 1.005."""
    from tests import dynamics_reference as DR
    rob, tab = DR.model(ti.G1)
    q = DR.Trajectory(rob, 3).state([k / ti.LOOP_FPS for k in range(ti.LOOP_FRAMES)])[0]
    offs = np.array([0, ti.LOOP_FRAMES])
    lim = np.asarray(tab.torque_limit)
    full, rest = TR.tau_pair(rob, tab, q, offs, ti.LOOP_FPS)
    res = {}
    for align in (False, True):
        p = TR.plan(full, rest, offs, lim, 1.0, 12, 8.0, None, align)
        oo = TR.lengths_to_offsets(p["out_len"])
        out = TR.apply_cubic(q, offs, p["ticks"], p["cum"], oo, int(oo[-1]))[0]
        t2 = TR.tau_pair(rob, tab, out, oo, ti.LOOP_FPS)[0]
        r = np.where(np.isfinite(lim), np.abs(t2) / lim, 0.0).max(axis=1)
        res[align] = (float(r.max()), int(np.argmax(r)), len(r))
    print("seed 3, before", TR.ratio(full, lim, offs), "after one pass (ratio, row, rows): unaligned", res[False], "aligned", res[True])
    assert res[False][0] > 4.0 and res[False][1] >= res[False][2] - 3 and res[True][0] < 1.01


# ------------------------------------------------------------------ 6: header, exports, binding, layout, streams
def _header():
    with open(os.path.join(ROOT, "include", "gmr_amd.h")) as f:
        return f.read()


def test_the_symbol_is_declared_exported_and_bound():
    from gmr_amd import _native
    src = _header()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint gmr_motion_retime_plan_torque\s*\(gmr_model \*m, const gmr_retime_torque_input \*in\);", code)
    assert re.search(r"^#define GMR_ABI_VERSION 5$", src, flags=re.M) and _native.ABI_VERSION == 5   # an addition
    assert ENTRY in _native.EXPORTS and ENTRY not in stream_prototypes()                     # the stream travels in the struct
    lib = _native.load()
    f = getattr(lib, ENTRY)
    assert f.restype == C.c_int and len(f.argtypes) == 2 and f.argtypes[1]._type_ is _native.RetimeTorqueInput
    assert f(None, C.byref(_native.RetimeTorqueInput())) == -1                               # a null handle is refused before anything else
    assert re.search(r"^ \*   gmr_motion_retime_plan_torque\s+\(no counterpart in the reference\)", src, flags=re.M)
    assert re.search(r"#define GMR_RETIME_INTERP_LINEAR 0\n#define GMR_RETIME_INTERP_CUBIC 1\n", src) and _native.RETIME_INTERP == {"linear": 0, "cubic": 1}
    assert "ticks may then exceed\n * 1024 max_stretch, by at most 1023" in src
    with open(os.path.join(ROOT, "gmr_amd", "csrc", "retime_torque_kernel.hip.h")) as fh:
        k = fh.read()
    assert int(re.search(r"constexpr int kRetimeAlignSpan = (\d+);", k).group(1)) == TR.ALIGN_SPAN == 64


def test_the_struct_layout_equals_the_c_compiler_and_the_listing_in_the_header(tmp_path):
    from gmr_amd import _native
    T, name, size = _native.RetimeTorqueInput, "gmr_retime_torque_input", 144
    fields = [k for k, _ in T._fields_]
    src = _header()
    src = src[src[:src.index("typedef struct " + name)].rindex("Layout (LP64)"):]
    m = re.match(r"Layout \(LP64\): sizeof (\d+); offsets (.*?)\.\s*\*/\s*typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S)
    assert m, "the layout listing in front of " + name
    listing = {k: int(v) for k, v in re.findall(r"([a-z_0-9]+) (\d+)", re.sub(r"\s*\*\s*", " ", m.group(2)))}
    body = re.sub(r"/\*.*?\*/", "", m.group(3), flags=re.S)
    declared = []
    for stmt in body.split(";"):
        declared += re.findall(r"\*?\s*([a-z_0-9]+)\s*(?:,|$)", stmt.strip())
    assert declared == fields
    assert C.sizeof(T) == int(m.group(1)) == size
    assert listing == {k: getattr(T, k).offset for k in fields}
    assert "interp" in [k for k, _ in _native.RetimeApplyInput._fields_] and _native.RetimeApplyInput.interp.offset == 52
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        return   # (no C compiler here: the listing and ctypes agree, which is what the library is built against)
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gmr_amd.h"\nint main(void) {\n'
                    f'  printf("%zu", sizeof({name}));\n'
                    + "".join(f'  printf(" %zu", offsetof({name}, {n}));\n' for n in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", f"-I{ROOT}/include", str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert C.sizeof(T) == got[0] and [getattr(T, n).offset for n in fields] == got[1:]


def test_the_launches_are_on_the_structs_stream_and_nothing_else_is_enqueued():
    problems, syncs = check_api(entries=[ENTRY])
    assert not problems, "\n".join(problems)
    assert syncs == {ENTRY: False}
    us = units()
    r = reachable(us, ENTRY)
    assert "retime_torque_run" in r and "scratch_alloc" not in r and "CallScratch" not in r   # no allocation
    assert sum(len(re.findall(r"\bhipLaunchKernelGGL\s*\(", us[u])) for u in r) == 4
    assert not any(re.search(r"\bhip\w+Async\s*\(", us[u]) for u in r)                         # no copy, no memset
    body = us[ENTRY]
    assert "static_cast<hipStream_t>(in->stream)" in re.sub(r"\s+", "", body)
    assert "hipLaunchKernelGGL" not in body and "hipSetDevice" not in body
    assert body.index("in->n_seq == 0") < body.index("retime_torque_run(")
    run = us["retime_torque_run"]
    order = [run.index(k) for k in ("motion_retime_torque_need_kernel", "motion_retime_ticks_kernel", "motion_retime_scan_kernel", "motion_retime_align_kernel")]
    assert order == sorted(order) and "motion_retime_need_kernel" not in run
    apply = us["retime_apply_run"]                                                           # the cubic is chosen on the host: one launch
    assert "motion_retime_apply_cubic_kernel" in apply and "motion_retime_apply_kernel" in apply and len(re.findall(r"\bhipLaunchKernelGGL\s*\(", apply)) == 1


def test_the_new_kernels_have_no_atomics_and_contraction_is_off_where_floats_are_computed():
    for name, kernels in (("retime_torque_kernel.hip.h", ("motion_retime_torque_need_kernel(RetimeTorqueArgs A)",)),
                          ("retime_kernel.hip.h", ("motion_retime_apply_cubic_kernel(RetimeApplyArgs A)", "retime_cubic(double p0"))):
        with open(os.path.join(ROOT, "gmr_amd", "csrc", name)) as f:
            code = re.sub(r"//.*", "", f.read())
        assert not re.search(r"atomic", code, flags=re.I) and "__shared__" not in code.split("motion_retime_apply_cubic_kernel")[-1]
        for kernel in kernels:
            body = code[code.index(kernel):]
            assert body[:body.index("\n", body.index("{")) + 60].count("#pragma clang fp contract(off)") == 1
    assert code.count("sqrt(") == 1                                                          # the quaternion's norm: one square root


# ------------------------------------------------------------------ 7: the Python layer's checks
def _stand_in(planar=False, nq=10):
    import torch
    return types.SimpleNamespace(device=torch.device("cpu"), nq=nq, cm=types.SimpleNamespace(robot=types.SimpleNamespace(planar_base=planar)))


def test_bad_arguments_raise_before_the_library_is_called():
    torch = pytest.importorskip("torch")
    from gmr_amd.engine import Engine, EngineError
    t = torch.zeros((6, 3), dtype=torch.float64)
    offs, lim = [0, 6], np.ones(3)
    plan = lambda *a, **k: Engine.motion_retime_plan_torque(_stand_in(), *a, **k)   # noqa: E731
    for args, text in [((t, t, offs, lim, 0.0, 12, 8.0), "limit_scale"), ((t, t, offs, lim, 1.5, 12, 8.0), "limit_scale"),
                       ((t, t, offs, lim, np.nan, 12, 8.0), "limit_scale"), ((t, t, offs, lim, 0.95, -1, 8.0), "window"),
                       ((t, t, offs, lim, 0.95, 33, 8.0), "window"), ((t, t, offs, lim, 0.95, 12, 0.5), "max_stretch"),
                       ((t, t, offs, lim, 0.95, 12, 65.0), "max_stretch"), ((t, t, offs, np.ones(4), 0.95, 12, 8.0), "torque_limit"),
                       ((t, t, offs, [1.0, 0.0, 1.0], 0.95, 12, 8.0), "torque_limit"), ((t, t, offs, [1.0, np.nan, 1.0], 0.95, 12, 8.0), "torque_limit")]:
        with pytest.raises(ValueError, match=text):
            plan(*args)
    with pytest.raises(EngineError, match="tau must"):
        plan(t[:, :2], t, offs, lim, 0.95, 12, 8.0)
    with pytest.raises(EngineError, match="tau_static must"):
        plan(t, t[:5], offs, lim, 0.95, 12, 8.0)
    with pytest.raises(EngineError, match="need_floor"):
        plan(t, t, offs, lim, 0.95, 12, 8.0, need_floor=torch.zeros(5, dtype=torch.float64))
    with pytest.raises(EngineError, match="torque_limit"):
        plan(t, t, offs, torch.ones(3, dtype=torch.float32), 0.95, 12, 8.0)
    with pytest.raises(NotImplementedError, match="planar"):
        Engine.motion_retime_plan_torque(_stand_in(planar=True), t, t, offs, lim, 0.95, 12, 8.0)
    q, i64 = torch.zeros((6, 10), dtype=torch.float64), lambda n: torch.zeros(n, dtype=torch.int64)   # noqa: E731
    with pytest.raises(ValueError, match="interp"):
        Engine.motion_retime_apply(_stand_in(), q, offs, {"ticks": i64(6), "cum": i64(6)}, [0, 6], interp="quintic")


def test_the_dataset_layer_and_the_walker_have_the_switch_and_it_is_off_by_default():
    pytest.importorskip("torch")
    import argparse
    import inspect
    import gmr_amd
    from gmr_amd import dataset
    from gmr_amd.scripts import _walk
    sig = inspect.signature(dataset.retime_to_torque_limits).parameters
    assert [sig[k].default for k in ("table", "limit_scale", "velocity_limits", "window", "max_stretch", "passes", "interp")] \
        == [None, 0.95, False, 12, 8.0, 4, "cubic"]
    assert (dataset.RETIME_TORQUE_SCALE, dataset.RETIME_TORQUE_WINDOW, dataset.RETIME_TORQUE_PASSES) == (ti.SCALE, ti.WINDOW, 4)
    assert inspect.signature(dataset.retime_to_limits).parameters["interp"].default == "linear"           # unchanged by default
    assert inspect.signature(gmr_amd.engine.Engine.motion_retime_apply).parameters["interp"].default == "linear"
    assert inspect.signature(dataset.retarget_clips).parameters["retime_torque"].default is None
    assert gmr_amd.retime_to_torque_limits is dataset.retime_to_torque_limits
    doc = dataset.retime_to_torque_limits.__doc__
    assert "not measured on a robot" in doc and "unfiltered" in doc and "unfiltered" in dataset.retarget_clips.__doc__
    planar = types.SimpleNamespace(model=types.SimpleNamespace(planar_base=True))
    with pytest.raises(NotImplementedError, match="planar"):
        dataset.retime_to_torque_limits(planar, None, [0], 30.0)
    ap = argparse.ArgumentParser()
    _walk.add_common_flags(ap)
    assert ap.parse_args([]).retime_to_torque is None                                        # off: nothing existing changes
    assert ap.parse_args(["--retime_to_torque"]).retime_to_torque is True
    assert ap.parse_args(["--retime_to_torque", "0.9"]).retime_to_torque == 0.9
    for argv in (["--retime_to_torque", "0"], ["--retime_to_torque", "1.5"], ["--retime_to_torque", "--robots", "unitree_g1,booster_k1"]):
        with pytest.raises(SystemExit):
            _walk.resolve_track(ap, ap.parse_args(argv))
    src = inspect.getsource(dataset.retarget_clips)
    assert src.index("smooth_qpos(") < src.index("retime_to_limits(") < src.index("retime_to_torque_limits(") < src.index("augment_mirror(")

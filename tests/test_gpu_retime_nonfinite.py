"""Non-finite qpos entries through gmr_motion_retime_plan and gmr_motion_retime_apply: the reach the contract above
gmr_retime_plan_input states, one poisoned element at a time (the poison values of tests/nonfinite_cases.py: +NaN, -NaN, +inf, -inf).

  a hinge entry   makes its two intervals non-finite (need = NaN, counted, stretched as 1) and reaches only the output rows that
                  interpolate its row, in that column.  Where the two intervals' clean stretch is 1 no ticks change at all; where it
                  is above 1 ticks change within 2 W intervals of them and nowhere else
  a root entry    reaches root columns of the output rows that read its row: its own column for the position, the four quaternion
                  columns through the slerp; no need, no ticks
  all             no other clip changes

Two routes: the structural set written from the contract (everything outside it must stay byte for byte what the clean input gives),
and the numpy restatement evaluated on the poisoned input, whose integers the kernels' must equal and whose ~isfinite mask the
kernels' must equal.  Masks only are compared where arithmetic is involved: never NaN against inf, never a NaN's payload or sign.

The case is b's limit (0.6 of the library's top speed, which leaves some intervals of the 130-frame clip alone) with the default
window of 4."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import nonfinite_cases as nc  # noqa: E402
from tests import retime_inputs as ri  # noqa: E402
from tests import retime_reference as RR  # noqa: E402
from tests.test_gpu_dynamics import _bytes  # noqa: E402
from tests.test_gpu_retime import PLAN_KEYS, run  # noqa: E402

ROBOT = "unitree_g1"
W = ri.WINDOW
A, B = int(ri.OFFS[ri.C130]), int(ri.OFFS[ri.C130 + 1])


def case(q=None):
    c = ri.case(ROBOT, "uniform")
    return ri.Case(c.q if q is None else q, c.offs, c.fps, c.vmax, W, c.max_stretch)


@functools.lru_cache(maxsize=None)
def clean():
    return run(ROBOT, case())


@functools.lru_cache(maxsize=None)
def rows():
    """(a row of the 130-frame clip whose two intervals are slow and whose neighbourhood is stretched, the row in front of the clip's
    fastest interval), both away from the clip's ends, from the clean plan."""
    p = clean()[0]
    need, ticks = p["need"], p["ticks"]
    slow = [r for r in range(A + 2 * W + 2, B - 2 * W - 2) if need[r - 1] <= 1.0 and need[r] <= 1.0 and ticks[r - 1] > 1024 and ticks[r] > 1024]
    fast = A + 2 * W + 2 + int(np.argmax(need[A + 2 * W + 2:B - 2 * W - 2]))                 # the fastest interval: its stretch is its window's maximum
    assert slow and need[fast] > 1.0
    return slow[0], fast


def changed(got, base):
    """bool, the elements whose bytes differ."""
    return np.any(_bytes(got).reshape(got.shape + (8,)) != _bytes(base).reshape(base.shape + (8,)), axis=-1)


def readers(p, oo, row):
    """The output rows of the 130-frame clip that read source row ``row``: as x0, or as x1 with u != 0."""
    o0, o1 = int(oo[ri.C130]), int(oo[ri.C130 + 1])
    i, u, _ = RR.sample_points(p["cum"], p["ticks"], A, B, np.arange(o1 - o0))
    r = row - A
    return o0 + np.flatnonzero((i == r) | ((i == r - 1) & (u != 0.0)))


def poisoned(row, col, value):
    q = np.array(case().q)
    q[row, col] = nc.value64(value)
    c = case(q)
    got = run(ROBOT, c)
    ref = RR.retime(c.q, c.offs, c.fps, c.vmax, c.window, c.max_stretch)
    p, out, st, oo = got
    for k in ("ticks", "cum", "out_len", "clip_stats"):                                     # the integers: the restatement's, exactly
        assert np.array_equal(p[k], ref[0][k]), k
    assert np.array_equal(np.isnan(p["need"]), np.isnan(ref[0]["need"])) and np.array_equal(p["need_max"], ref[0]["need_max"])
    assert np.array_equal(oo, ref[3]) and np.array_equal(_bytes(st), _bytes(ref[2]))
    assert np.array_equal(~np.isfinite(out), ~np.isfinite(ref[1]))                          # the restatement's mask
    return got


def other_clips_keep_their_bytes(got, base):
    (p, out, st, oo), (p0, out0, st0, oo0) = got, base
    for s in range(ri.S):
        if s != ri.C130:
            a, b = int(ri.OFFS[s]), int(ri.OFFS[s + 1])
            assert all(np.array_equal(_bytes(p[k][a:b]), _bytes(p0[k][a:b])) for k in ("need", "ticks", "cum"))
            assert all(np.array_equal(_bytes(p[k][s]), _bytes(p0[k][s])) for k in ("out_len", "clip_stats", "need_max"))
            assert np.array_equal(_bytes(out[int(oo[s]):int(oo[s + 1])]), _bytes(out0[int(oo0[s]):int(oo0[s + 1])]))


@pytest.mark.parametrize("value", nc.VALUES)
def test_a_hinge_entry_between_slow_intervals_reaches_the_rows_that_interpolate_its_row_in_that_column(value):
    row = rows()[0]
    base = clean()
    nq = base[1].shape[1]
    for col in (7, nq - 1):
        got = poisoned(row, col, value)
        p, out, st, oo = got
        assert np.flatnonzero(changed(p["need"], base[0]["need"])).tolist() == [row - 1, row] and np.isnan(p["need"][[row - 1, row]]).all()
        assert p["clip_stats"][ri.C130].tolist() == (base[0]["clip_stats"][ri.C130] + [0, 0, 2, 0]).tolist()
        for k in ("ticks", "cum", "out_len", "need_max"):                                   # both stretched as 1 before: no tick changes
            assert np.array_equal(_bytes(p[k]), _bytes(base[0][k])), k
        assert np.array_equal(_bytes(st), _bytes(base[2]))
        ch = changed(out, base[1])
        want = np.zeros(out.shape, bool)
        rd = readers(p, oo, row)
        want[rd, col] = True
        assert len(rd) >= 1 and np.array_equal(ch, want), np.argwhere(ch != want)[:6].tolist()
        assert np.array_equal(~np.isfinite(out), want)
        other_clips_keep_their_bytes(got, base)


@pytest.mark.parametrize("value", ["+nan", "-inf"])
def test_a_hinge_entry_between_fast_intervals_changes_ticks_within_two_windows_only(value):
    row = rows()[1]
    base = clean()
    got = poisoned(row, 7, value)
    p, out, st, oo = got
    assert np.flatnonzero(np.isnan(p["need"])).tolist() == [row - 1, row]
    moved = np.flatnonzero(p["ticks"] != base[0]["ticks"])
    assert moved.size and moved.min() >= row - 1 - 2 * W and moved.max() <= row + 2 * W      # they stretch as 1 now
    assert np.all(p["ticks"][moved] < base[0]["ticks"][moved])
    bad = ~np.isfinite(out)
    assert bad[:, 7].sum() >= 1 and not np.delete(bad, 7, axis=1).any()                      # that column alone
    assert np.array_equal(np.flatnonzero(bad[:, 7]), readers(p, oo, row))
    other_clips_keep_their_bytes(got, base)


@pytest.mark.parametrize("value", nc.VALUES)
def test_a_root_entry_reaches_root_columns_of_the_rows_that_read_its_row_and_no_need(value):
    row = rows()[0]
    base = clean()
    for col in (0, 2, 3, 6):
        got = poisoned(row, col, value)
        p, out, st, oo = got
        assert all(np.array_equal(_bytes(p[k]), _bytes(base[0][k])) for k in PLAN_KEYS)     # the root enters no need
        assert np.array_equal(_bytes(st), _bytes(base[2]))
        ch = changed(out, base[1])
        rd = readers(p, oo, row)
        allowed = np.zeros(out.shape, bool)
        if col < 3:
            allowed[rd, col] = True
            assert np.array_equal(ch, allowed)                                              # a position column stays in its column
        else:
            allowed[np.ix_(rd, range(3, 7))] = True                                         # the slerp mixes the four components ...
            assert ch.any() and not (ch & ~allowed).any()
            copies = [r for r in rd if st[r] == row - A]
            assert all(ch[r].sum() == 1 and ch[r, col] for r in copies)                     # ... a copy does not
        other_clips_keep_their_bytes(got, base)

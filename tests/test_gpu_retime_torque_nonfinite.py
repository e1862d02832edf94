"""Non-finite entries through gmr_motion_retime_plan_torque and the cubic gmr_motion_retime_apply: the reach the contracts above
gmr_retime_torque_input and gmr_retime_plan_input state, one poisoned element at a time (the poison values of
tests/nonfinite_cases.py: +NaN, -NaN, +inf, -inf).

  tau, tau_static  an entry -- of a hinge without a limit too -- makes its row non-finite: its two intervals get need NaN
                   (0x7ff8000000000000), stretch as 1 and are counted, and the row's static_over is 0.  Ticks change only within
                   2 W intervals of them.
  need_floor       an entry that is not < +inf makes its one interval non-finite; -inf is below every need and changes nothing.
  qpos, cubic      an entry reaches the output rows whose four-row stencil reads it, in its column -- in the quaternion all four
                   components -- and nothing else.
  all              no byte of another clip changes.

The rows are at tile edges (rows 63, 64 and 65 of a clip: the 64th row is the need kernel's 65th of tile 0 and lane 0 of tile 1) and
at clip ends.  The integers are the restatement's on the same poisoned input, evaluated on the GPU's own need."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import nonfinite_cases as nc  # noqa: E402
from tests import retime_inputs as ri  # noqa: E402
from tests import retime_reference as RR  # noqa: E402
from tests import retime_torque_inputs as ti  # noqa: E402
from tests import retime_torque_reference as TR  # noqa: E402
from tests.test_gpu_dynamics import _bytes  # noqa: E402
from tests.test_gpu_retime_torque import KEYS, check_plan, gpu_plan, run_apply, run_plan  # noqa: E402

G1 = "unitree_g1"
W = ti.WINDOW
C130 = 8
A, B = int(ti.OFFS[C130]), int(ti.OFFS[C130 + 1])        # the clip of 130 rows
ROWS = {"first": A, "lane63": A + 63, "lane0": A + 64, "lane1": A + 65, "last": B - 1}
NANBITS = 0x7FF8000000000000


def clean():
    return gpu_plan(G1, "lens", True, True)


def poisoned_plan(array, row, col, value):
    c = ti.case(G1, "lens", True, True)
    arrs = {"tau": np.array(c.tau), "tau_static": np.array(c.tau_static), "floor": np.array(c.floor)}
    if array == "floor":
        arrs["floor"][row] = nc.value64(value)
    else:
        arrs[array][row, col] = nc.value64(value)
    c2 = ti.Case(arrs["tau"], arrs["tau_static"], c.offs, c.limit, c.scale, c.window, c.max_stretch, arrs["floor"], True)
    p = run_plan(G1, c2)
    ref = TR.plan(c2.tau, c2.tau_static, c2.offs, c2.limit, c2.scale, c2.window, c2.max_stretch, c2.floor, True)
    check_plan(p, ref, c2, c2.offs, f"{array}[{row}, {col}] = {value}")
    for k in ("ticks", "cum", "out_len", "clip_stats"):                                     # the integers: the restatement's, exactly
        assert np.array_equal(p[k], ref[k]), k
    return p


def other_clips_keep_their_bytes(p, base):
    for s in range(len(ti.OFFS) - 1):
        if s != C130:
            a, b = int(ti.OFFS[s]), int(ti.OFFS[s + 1])
            assert all(np.array_equal(_bytes(p[k][a:b]), _bytes(base[k][a:b])) for k in ("need", "ticks", "cum", "static_over"))
            assert all(np.array_equal(_bytes(p[k][s]), _bytes(base[k][s])) for k in ("out_len", "clip_stats", "need_max"))


@pytest.mark.parametrize("value", nc.VALUES)
@pytest.mark.parametrize("where", sorted(ROWS))
def test_an_entry_of_tau_or_tau_static_makes_its_rows_two_intervals_non_finite(where, value):
    row, base = ROWS[where], clean()
    c = ti.case(G1, "lens", True, True)
    free = int(np.flatnonzero(np.isinf(c.limit))[0])                                         # a hinge without a limit: "any entry"
    for array, col in (("tau", 3), ("tau_static", 28), ("tau", free)):
        p = poisoned_plan(array, row, col, value)
        want = [r for r in (row - 1, row) if A <= r < B - 1]
        changed = np.flatnonzero(p["need"].view(np.uint64) != base["need"].view(np.uint64))
        assert changed.tolist() == want and p["need"][want].view(np.uint64).tolist() == [NANBITS] * len(want)
        assert p["clip_stats"][C130, 2] == base["clip_stats"][C130, 2] + len(want)
        so_changed = np.flatnonzero(p["static_over"] != base["static_over"])
        assert set(so_changed.tolist()) <= {row} and p["static_over"][row] == 0
        moved = np.flatnonzero(p["ticks"] != base["ticks"])
        lo, hi = min(want) - 2 * W, max(want) + 2 * W
        tail = np.arange(max(A, B - 1 - 64), B - 1)                                          # (the alignment spreads a changed total over the last 64)
        assert all((lo <= r <= hi) or r in tail for r in moved.tolist())
        other_clips_keep_their_bytes(p, base)


@pytest.mark.parametrize("value", nc.VALUES)
def test_an_entry_of_the_floor_makes_its_one_interval_non_finite_unless_it_is_minus_infinity(value):
    base = clean()
    for row in (ROWS["lane63"], ROWS["lane0"], A, B - 2):
        p = poisoned_plan("floor", row, None, value)
        nan = np.flatnonzero(np.isnan(p["need"]))
        if value == "-inf":
            assert nan.size == 0 and p["clip_stats"][C130, 2] == 0                            # below every need: the torque need stands
            assert p["need"][row] >= 0.0 and np.array_equal(np.delete(p["need"], row), np.delete(base["need"], row))
        else:
            assert nan.tolist() == [row] and p["need"].view(np.uint64)[row] == NANBITS and p["clip_stats"][C130, 2] == 1
        assert np.array_equal(p["static_over"], base["static_over"])
        other_clips_keep_their_bytes(p, base)
    p = poisoned_plan("floor", B - 1, None, value)                                           # the last row's floor belongs to no interval
    assert all(np.array_equal(_bytes(p[k]), _bytes(base[k])) for k in KEYS)


# ------------------------------------------------------------------ a poisoned qpos row through the cubic stencil
QA, QB = int(ri.OFFS[ri.C130]), int(ri.OFFS[ri.C130 + 1])


@functools.lru_cache(maxsize=None)
def clean_apply():
    c = ri.case(G1, "uniform")
    p, _, _, oo, _ = ri.reference(G1, "uniform")
    out, st = run_apply(G1, c, p, oo)
    return c, p, oo, out, st


def stencil_readers(p, oo, row):
    """The output rows of the 130-frame clip whose stencil reads source row ``row``: the copies of it, and the rows with u != 0 in the
    intervals row - 2 .. row + 1 (a reflected end reads its two inner rows only)."""
    o0, o1 = int(oo[ri.C130]), int(oo[ri.C130 + 1])
    n = QB - QA
    i, u, done = RR.sample_points(p["cum"], p["ticks"], QA, QB, np.arange(o1 - o0))
    r = row - QA
    turn = ~done & (u != 0.0)
    lo, hi = np.where(i > 0, i - 1, i), np.where(i + 2 < n, i + 2, i + 1)
    return o0 + np.flatnonzero(np.where(turn, (lo <= r) & (r <= hi), i == r))


@pytest.mark.parametrize("value", nc.VALUES)
@pytest.mark.parametrize("where", ["first", "second", "lane63", "lane0", "last"])
def test_a_qpos_entry_reaches_the_rows_whose_stencil_reads_it(where, value):
    c, p, oo, out0, st0 = clean_apply()
    row = {"first": QA, "second": QA + 1, "lane63": QA + 63, "lane0": QA + 64, "last": QB - 1}[where]
    for col in (1, 4, 7, c.q.shape[1] - 1):
        q = np.array(c.q)
        q[row, col] = nc.value64(value)
        out, st = run_apply(G1, ri.Case(q, c.offs, c.fps, c.vmax, c.window, c.max_stretch), p, oo)
        ref = TR.apply_cubic(q, c.offs, p["ticks"], p["cum"], oo, int(oo[-1]))[0]
        assert np.array_equal(_bytes(st), _bytes(st0))
        bad = ~np.isfinite(out)
        assert np.array_equal(bad, ~np.isfinite(ref))                                        # the restatement's mask
        rd = stencil_readers(p, oo, row)
        allowed = np.zeros(out.shape, bool)
        if 3 <= col < 7:
            allowed[np.ix_(rd, range(3, 7))] = True                                          # the norm mixes the four components ...
            copies = [r for r in rd if st[r] == row - QA]
            assert all(bad[r].sum() == 1 and bad[r, col] for r in copies)                    # ... a copy does not
            curved = [r for r in rd if r not in copies]
            assert all(bad[r, 3:7].all() for r in curved)
        else:
            allowed[rd, col] = True
            assert np.array_equal(bad, allowed)
        assert len(rd) >= 1 and bad.any() and not (bad & ~allowed).any()
        same = np.all(_bytes(out).reshape(out.shape + (8,)) == _bytes(out0).reshape(out0.shape + (8,)), axis=-1)
        assert not (~same & ~allowed).any()                                                  # everything else keeps its bytes: no other clip changes

"""Non-finite qpos entries through gmr_motion_compose: the reach the contract above gmr_compose_input states, one poisoned element at
a time (the poison values of tests/nonfinite_cases.py: +NaN, -NaN, +inf, -inf).

  a hinge entry                  reaches only the output rows that read its row, in that column
  a root entry, no anchor row    reaches root columns of the output rows that read it
  a root entry of an anchor row  reaches root columns of that segment (for the previous segment's anchor row: of the next one) and of
                                 the later segments of the same output clip
  all                            no other output clip changes, and no hinge column is affected by a root

Two routes: the structural set written from the contract (everything outside it must stay byte for byte what the clean input gives),
and the numpy restatement evaluated on the poisoned input, whose ~isfinite mask the kernel's must equal.  Masks only are compared
where arithmetic is involved: never NaN against inf, never a NaN's payload or sign.

The plan is case c of tests/test_gpu_compose.py: output clip 0 chains the clips of 63, 64, 65, 130 frames and 40 frames of the first
with blends of 8; output clip 1 reads 60 frames of the 130-frame clip and 30 of the 65-frame one."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import compose_inputs as ci  # noqa: E402
from tests import compose_reference as CR  # noqa: E402
from tests import nonfinite_cases as nc  # noqa: E402
from tests.test_gpu_dynamics import _bytes  # noqa: E402
from tests.test_gpu_compose import gpu, run  # noqa: E402

NAME = "blend8"
A64 = int(ci.OFFS[ci.C64])          # the 64-frame clip is segment 1 of output clip 0 and of nothing else
MIDDLE = A64 + 30                   # read by one output row, outside every overlap
IN_BLEND = A64 + 2                  # read by one output row of the overlap with segment 0 (no anchor: that is row 4)
ANCHOR = A64 + 4                    # segment 1's anchor row
ANCHOR_PREV = int(ci.OFFS[ci.C63]) + 63 - 8 + 4   # segment 0's row of the same anchor pair
ROBOTS = ci.ROBOTS


def changed(got, base):
    """[rows, nq] bool: the elements whose bytes differ."""
    return np.any(_bytes(got).reshape(got.shape + (8,)) != _bytes(base).reshape(base.shape + (8,)), axis=-1)


def check(robot, row, col, value, allowed):
    q, plan = ci.case(robot, NAME)
    q = np.array(q)
    q[row, col] = nc.value64(value)
    (got, T), (base, T0), (ref, T_ref) = run(robot, q, plan), gpu(robot, NAME), CR.compose(plan, q)
    ch = changed(got, base)
    what = f"{robot} row {row} col {col} {value}"
    assert ch.any() and not (ch & ~allowed).any(), f"{what}: changed outside the contract's reach at {np.argwhere(ch & ~allowed)[:4].tolist()}"
    assert np.array_equal(~np.isfinite(got), ~np.isfinite(ref)), what                       # the restatement's mask
    assert np.array_equal(~np.isfinite(T), ~np.isfinite(T_ref)), what
    a, b = int(plan.out_offsets[1]), int(plan.out_offsets[2])
    assert np.array_equal(_bytes(got[a:b]), _bytes(base[a:b])), what                        # the other output clip keeps its bytes
    assert np.array_equal(_bytes(T[5:]), _bytes(T0[5:])), what
    return got, ch, T, T0, plan


def rows_mask(robot, rows, cols):
    plan = ci.case(robot, NAME)[1]
    m = np.zeros((plan.n_out_frames, gpu(robot, NAME)[0].shape[1]), bool)
    m[np.ix_(rows, cols)] = True
    return m


@pytest.mark.parametrize("value", nc.VALUES)
@pytest.mark.parametrize("robot", ROBOTS)
def test_a_hinge_entry_reaches_the_rows_that_read_its_row_in_that_column(robot, value):
    plan = ci.case(robot, NAME)[1]
    nq = gpu(robot, NAME)[0].shape[1]
    for row in (MIDDLE, IN_BLEND, ANCHOR, A64 + 60):                                        # (the last: read into segment 2's overlap)
        readers = ci.readers(plan, row)
        assert len(readers) == 1
        for col in (7, nq - 1):
            got, ch, T, T0, _ = check(robot, row, col, value, rows_mask(robot, readers, [col]))
            assert ch.sum() == 1 and np.array_equal(_bytes(T), _bytes(T0))
            if row == MIDDLE:                                                               # a copy: the same bits
                assert np.array_equal(_bytes(got[readers[0], col]), _bytes(np.float64(nc.value64(value))))


@pytest.mark.parametrize("value", nc.VALUES)
@pytest.mark.parametrize("robot", ROBOTS)
def test_a_root_entry_of_a_row_that_is_no_anchor_reaches_root_columns_of_the_rows_that_read_it(robot, value):
    plan = ci.case(robot, NAME)[1]
    for row in (MIDDLE, IN_BLEND):
        readers = ci.readers(plan, row)
        for col in (0, 1, 2, 3, 6):
            got, ch, T, T0, _ = check(robot, row, col, value, rows_mask(robot, readers, range(7)))
            assert np.array_equal(_bytes(T), _bytes(T0))                                    # no placement changes
            if col == 2:
                assert ch.sum() == 1                                                        # z is copied (blended with z alone) and enters nothing else
            elif col < 2 and row == MIDDLE:
                assert not ch[:, 2:7].any()                                                 # xy stay among themselves
            elif row == MIDDLE:
                assert not ch[:, :3].any()                                                  # and so does the quaternion


@pytest.mark.parametrize("value", nc.VALUES)
@pytest.mark.parametrize("robot", ROBOTS)
def test_a_root_entry_of_an_anchor_row_reaches_root_columns_of_its_segment_and_the_later_ones(robot, value):
    plan = ci.case(robot, NAME)[1]
    later = list(range(int(plan.seg_out[1]), int(plan.out_offsets[1])))                     # segment 1's rows and everything behind them in clip 0
    for row in (ANCHOR, ANCHOR_PREV):
        for col in (0, 1, 3, 5):
            got, ch, T, T0, _ = check(robot, row, col, value, rows_mask(robot, later, range(7)))
            assert np.array_equal(_bytes(T[0]), _bytes(T0[0])) and changed(T, T0)[1:5].any(axis=1).all()   # T_1 .. T_4 of the chain
            assert ch[later].any(axis=1).sum() >= len(later) - 8                            # every placed row behind the overlap is reached
        one = ci.readers(plan, row)
        got, ch, T, T0, _ = check(robot, row, 2, value, rows_mask(robot, one, [2]))          # z enters no placement
        assert ch.sum() == 1 and np.array_equal(_bytes(T), _bytes(T0))

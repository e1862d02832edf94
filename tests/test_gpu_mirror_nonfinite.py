"""Non-finite qpos entries through gmr_motion_mirror: the reach the contract above gmr_mirror_input states, one poisoned element at a
time (the poison values of tests/nonfinite_cases.py: +NaN, -NaN, +inf, -inf).

  GMR_MIRROR_WORLD       the entry reaches exactly the output element it is copied to, as the same bits (negated where the column is).
  GMR_MIRROR_CLIP_START  a root entry of a clip's first row reaches root columns of that clip's rows only; a root entry of another
                         row reaches root columns of that row only; a hinge entry reaches exactly the element it is copied to.
  both                   hinge columns are never affected by the root, and no other clip changes.

Two routes: the structural set written from the contract (everything outside it must stay byte for byte what the clean input gives),
and the numpy definition evaluated on the poisoned input, whose ~isfinite mask the kernel's must equal.  Masks only are compared
where arithmetic is involved: never NaN against inf, never a NaN's payload or sign."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import mirror_inputs as mi  # noqa: E402
from tests import mirror_reference as MR  # noqa: E402
from tests import nonfinite_cases as nc  # noqa: E402
from tests.test_gpu_dynamics import _bytes  # noqa: E402
from tests.test_gpu_mirror import gpu, run  # noqa: E402

CLIP = 5                      # 63 frames: rows 10 .. 72
A, B = int(mi.OFFS[CLIP]), int(mi.OFFS[CLIP + 1])
LATER = A + 17
ROBOTS = ["unitree_g1", "booster_k1"]


def changed(got, base):
    """[N, nq] bool: the elements whose bytes differ."""
    return np.any(_bytes(got).reshape(got.shape + (8,)) != _bytes(base).reshape(base.shape + (8,)), axis=-1)


def poisoned(robot, row, col, value):
    q = np.array(mi.qpos(robot))
    q[row, col] = nc.value64(value)
    return q


def reference(robot, q, about):
    return MR.world_clips(mi.plan(robot), q, mi.OFFS) if about == "world" else MR.clip_start(mi.plan(robot), q, mi.OFFS)


def check(robot, about, row, col, value, allowed):
    q = poisoned(robot, row, col, value)
    got, base, ref = run(robot, q, mi.OFFS, about), gpu(robot, about), reference(robot, q, about)
    ch = changed(got, base)
    what = f"{robot} {about} row {row} col {col} {value}"
    assert ch.any() and not (ch & ~allowed).any(), f"{what}: changed outside the contract's reach at {np.argwhere(ch & ~allowed)[:4].tolist()}"
    assert np.array_equal(~np.isfinite(got), ~np.isfinite(ref)), what                       # the definition's mask
    assert np.array_equal(_bytes(got[:, 7:]), _bytes(ref[:, 7:])), what                     # the hinge columns: copies, bit for bit
    return got, ref, ch


@pytest.mark.parametrize("value", nc.VALUES)
@pytest.mark.parametrize("robot", ROBOTS)
def test_world_mode_reaches_exactly_the_element_the_entry_is_copied_to(robot, value):
    plan, nq = mi.plan(robot), mi.plan(robot).nq
    for row in (A, LATER):
        for col in (0, 1, 3, 6, 7, nq - 1):
            dst = col if col < 7 else int(np.flatnonzero(plan.col_src == col)[0])
            allowed = np.zeros((mi.N, nq), bool)
            allowed[row, dst] = True
            got, ref, ch = check(robot, "world", row, col, value, allowed)
            assert ch.sum() == 1 and np.array_equal(_bytes(got), _bytes(ref))               # the same bits, negated where the column is


@pytest.mark.parametrize("value", nc.VALUES)
@pytest.mark.parametrize("robot", ROBOTS)
def test_clip_start_first_row_root_entry_reaches_root_columns_of_its_clip_only(robot, value):
    nq = mi.plan(robot).nq
    allowed = np.zeros((mi.N, nq), bool)
    allowed[A:B, :7] = True
    for col in (0, 1, 3, 5):
        got, ref, ch = check(robot, "start", A, col, value, allowed)
        assert ch[A:B, :7].any(axis=1).all()                                                # every row of the clip is reached
    one = np.zeros((mi.N, nq), bool)
    one[A, 2] = True                                                                        # z is copied and enters nothing else
    got, ref, ch = check(robot, "start", A, 2, value, one)
    assert np.array_equal(_bytes(got[A, 2]), _bytes(ref[A, 2]))


@pytest.mark.parametrize("value", nc.VALUES)
@pytest.mark.parametrize("robot", ROBOTS)
def test_clip_start_later_row_root_entry_reaches_root_columns_of_its_row_only(robot, value):
    nq = mi.plan(robot).nq
    allowed = np.zeros((mi.N, nq), bool)
    allowed[LATER, :7] = True
    for col in (0, 1, 2, 4, 6):
        got, ref, ch = check(robot, "start", LATER, col, value, allowed)
        if col < 2:
            assert not ch[LATER, 2:7].any()                                                 # xy stay among themselves
        elif col == 2:
            assert ch.sum() == 1
        else:
            assert not ch[LATER, :3].any()                                                  # and so does the quaternion


@pytest.mark.parametrize("value", nc.VALUES)
@pytest.mark.parametrize("robot", ROBOTS)
def test_clip_start_hinge_entry_reaches_exactly_the_element_it_is_copied_to(robot, value):
    plan, nq = mi.plan(robot), mi.plan(robot).nq
    for row in (A, LATER):
        for col in (7, nq - 1):
            allowed = np.zeros((mi.N, nq), bool)
            allowed[row, int(np.flatnonzero(plan.col_src == col)[0])] = True
            got, ref, ch = check(robot, "start", row, col, value, allowed)
            assert ch.sum() == 1

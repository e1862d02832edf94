"""Non-finite qpos entries through gmr_motion_transitions: the reach the contract above gmr_transitions_input states, one poisoned
element at a time (the poison values of tests/nonfinite_cases.py: +NaN, -NaN, +inf, -inf).

  an entry of row k of clip s   reaches the points and (m, q) of that row, the (M, V) of the windows of clip s that contain it, the
                                 dense costs of the sources of clip s whose windows contain it (whole rows) and of the target frames
                                 of clip s whose windows contain it (whole columns), and the best frames of those sources; the best
                                 frame of another source may move only within target clip s
  the root (x, y) of a clip's    reaches every row of that clip in the same way
  first row
  all                            no other byte changes

Two routes: the structural set written from the contract (everything outside it must stay byte for byte what the clean input gives),
and the numpy restatement evaluated on the kernel's own poisoned points, which the kernel's costs and best frames must equal, a NaN
for a NaN.  The case is the main comparison of tests/test_gpu_transitions.py at L = 8."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import nonfinite_cases as nc  # noqa: E402
from tests import transitions_inputs as ti  # noqa: E402
from tests import transitions_reference as TR  # noqa: E402
from tests.test_gpu_dynamics import _bytes  # noqa: E402
from tests.test_gpu_transitions import main_case, run  # noqa: E402

L = 8
CLIP = 7            # the 65-frame clip
FRAME = 30


def changed(got, base):
    return np.any(_bytes(got).reshape(got.shape + (got.itemsize,)) != _bytes(base).reshape(base.shape + (base.itemsize,)), axis=-1)


def check(robot, frames, col, value, poison_frame):
    """Poison (clip CLIP, frame poison_frame, column col); ``frames``: the frames of the clip the contract lets it reach."""
    q, offs = ti.library(robot, L)
    ids, w = ti.all_bodies(robot)
    a, T = int(offs[CLIP]), int(offs[CLIP + 1] - offs[CLIP])
    q = np.array(q)
    q[a + poison_frame, col] = nc.value64(value)
    got, mt = run(robot, q, offs, ids, w, L, min_gap=L)
    base = main_case(robot, L)[0]
    what = f"{robot} frame {poison_frame} col {col} {value}"
    frames = np.asarray(sorted(frames))
    windows = np.unique(np.concatenate([np.arange(max(f - L + 1, 0), min(f, T - L) + 1) for f in frames]))
    # the structural route
    ch = changed(got["points"], base["points"])
    assert ch.any(), what
    assert not np.delete(ch, a + frames, axis=0).any(), what                                  # points: the reached rows only
    chm = changed(got["moments"], base["moments"])
    ok = np.zeros(chm.shape, bool)
    ok[a + frames, :3] = True
    ok[a + windows, 3:] = True
    assert not (chm & ~ok).any(), what
    u0, c0 = int(mt.src_offsets[CLIP]), int(mt.dst_offsets[CLIP])
    chc = changed(got["cost_out"], base["cost_out"])
    okc = np.zeros(chc.shape, bool)
    okc[u0 + windows, :] = True
    okc[:, c0 + windows] = True
    assert chc.any() and not (chc & ~okc).any(), f"{what}: costs changed outside the contract's reach at {np.argwhere(chc & ~okc)[:4].tolist()}"
    for k in ("best_cost", "best_frame"):
        chb = changed(got[k], base[k])
        okb = np.zeros(chb.shape, bool)
        okb[u0 + windows, :] = True
        okb[:, CLIP] = True
        assert not (chb & ~okb).any(), (what, k)
    # the restatement on the kernel's own points: a NaN for a NaN, every other byte
    dense, best, frame = TR.search(got["points"], mt.weights, offs, L, mt.src_clips, mt.src_offsets, 1, mt.dst_clips, mt.dst_offsets, L)
    assert np.array_equal(np.isnan(got["cost_out"]), np.isnan(dense)), what
    assert np.array_equal(got["cost_out"], dense, equal_nan=True) and np.array_equal(got["best_cost"], best) and np.array_equal(got["best_frame"], frame), what
    assert not np.isnan(got["best_cost"]).any()                                              # the minimum skips a NaN
    return got, mt, windows


@pytest.mark.parametrize("value", nc.VALUES)
@pytest.mark.parametrize("robot", ti.ROBOTS)
def test_an_entry_reaches_its_row_and_the_windows_that_contain_it(robot, value):
    for col in (2, 0, 4, 7, 10):                                                             # root z, root x, a quaternion entry, two hinges with bodies below them
        got, mt, windows = check(robot, [FRAME], col, value, FRAME)
        assert windows.tolist() == list(range(FRAME - L + 1, FRAME + 1))
        u0 = int(mt.src_offsets[CLIP])
        assert not np.isfinite(got["cost_out"][u0 + windows][:, :8]).any()                    # (the first target clip with frames: every pair is reached)
    check(robot, [0], 7, value, 0)                                                          # a hinge of the first row: no further than that row
    check(robot, [64], 2, value, 64)                                                         # the last row: one window


@pytest.mark.parametrize("value", nc.VALUES)
@pytest.mark.parametrize("robot", ti.ROBOTS)
def test_the_root_xy_of_a_clips_first_row_reaches_the_whole_clip(robot, value):
    for col in (0, 1):
        got, mt, windows = check(robot, range(65), col, value, 0)
        u0 = int(mt.src_offsets[CLIP])
        assert np.all(got["best_frame"][u0:u0 + 58, :] == -1) and np.all(got["best_frame"][:, CLIP] == -1)
        offs = ti.library(robot, L)[1]
        assert not np.isfinite(got["points"][int(offs[CLIP]):int(offs[CLIP + 1]), :, col]).any()

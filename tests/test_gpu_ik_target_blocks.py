"""Target blocks: the plain instances of the IK kernel prepare the targets of four frames in one pass, lane 16 j + s the
slot s of frame kf + j, and every instance prepares a slot with one pinned function (``target_prep_slot``).  Neither may change a
bit: every comparison here is ``torch.equal`` on qpos, the solve words and ``frames_done``, against the generic instance (one frame
per pass) and against the bits of the parent commit (``tests/golden/ik_g1_smplx_parent_bits.npz``, ``tools/record_ik_bits.py``).

Robot ``unitree_g1`` / ``smplx``; clips from ``synth.synth_clips``, half of them ``hard=True``.  Which instance a launch took is read
from the ``GMR_DEBUG_PLAN`` line; ``GMR_AMD_GENERIC_SHAPE`` is read at model creation, hence a fresh Engine per setting.
"""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gmr_amd import _native, synth  # noqa: E402
from gmr_amd.engine import Engine, EngineGroup  # noqa: E402
from gmr_amd.schedule import make_items  # noqa: E402
from tests.util import compiled  # noqa: E402

SHAPED = "IkShapeG1Smplx"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ik_g1_smplx_parent_bits.npz")
RAGGED = [1, 2, 3, 4, 5, 7, 8, 9, 13, 40]  # every remainder of a block of four, blocks of one to ten


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cm():
    return compiled("smplx", "unitree_g1")


@pytest.fixture
def run(monkeypatch, capfd, dev, cm):
    """run(generic_shape, fn, balance="0", slice_len=None) -> (fn(engine)'s result, [kind, instance] of every IK launch it made)."""
    monkeypatch.setenv("GMR_DEBUG_PLAN", "1")

    def go(generic_shape, fn, balance="0", slice_len=None):
        monkeypatch.setenv("GMR_AMD_GENERIC_SHAPE", "1" if generic_shape else "0")
        monkeypatch.setenv("GMR_AMD_BALANCE", balance)
        if slice_len is None:
            monkeypatch.delenv("GMR_AMD_BALANCE_SLICE", raising=False)
        else:
            monkeypatch.setenv("GMR_AMD_BALANCE_SLICE", str(slice_len))
        eng = Engine(cm, 0)
        capfd.readouterr()
        res = fn(eng)
        torch.cuda.synchronize()
        launches = re.findall(r"gmr: ik launch: (\w+) instance (\w+)", capfd.readouterr().err)
        assert eng.sliced_timeouts == 0
        eng.close()
        return res, launches
    return go


def _clips(cm, lengths, seeds=(41, 42), dtype=np.float32):
    """len(lengths) clips, the first half easy and the rest hard, clip c cut to its first lengths[c] frames: numpy (pos, quat), the
    slot columns and the clip offsets."""
    n, T = len(lengths), max(lengths)
    pe, qe, names, _, _ = synth.synth_clips(cm, n - n // 2, T, seed=seeds[0], hard=False, dtype=dtype)
    ph, qh, names_h, _, _ = synth.synth_clips(cm, n // 2, T, seed=seeds[1], hard=True, dtype=dtype)
    assert names == names_h
    keep = np.concatenate([np.arange(c * T, c * T + ln) for c, ln in enumerate(lengths)])
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return np.concatenate([pe, ph])[keep], np.concatenate([qe, qh])[keep], cm.slot_columns(names), offs


def _solver(dev, pos, quat, sc, items, qpos_init=None):
    pos, quat = torch.from_numpy(pos).to(dev), torch.from_numpy(quat).to(dev)
    qi = None if qpos_init is None else torch.from_numpy(qpos_init).to(dev)

    def solve(eng):
        fd = torch.full((len(items),), -1, dtype=torch.int32, device=dev)
        q, it, _ = eng.ik_solve(pos, quat, sc, items, qpos_init=qi, frames_done=fd, launch_order=None)
        return q, it, fd
    return solve


def _same(a, b):
    for x, y, what in zip(a, b, ("qpos", "solve words", "frames_done")):
        assert torch.equal(x, y), what


def test_ragged_blocks_whole_clip(run, dev, cm):
    """Clips of 1 .. 40 frames in one batch, whole-clip launch: last blocks of one, two, three and four frames."""
    pos, quat, sc, offs = _clips(cm, RAGGED)
    solve = _solver(dev, pos, quat, sc, make_items(offs))

    def solve_and_lds(eng):
        assert 0 < eng.info.lds_bytes <= 20480, eng.info.lds_bytes  # the ring of four images fits: still eight wavefronts per CU, two per SIMD
        return solve(eng)

    shaped, how_s = run(False, solve_and_lds)
    generic, how_g = run(True, solve)
    assert how_s == [("solve", SHAPED)] and how_g == [("solve", "generic")]
    assert not torch.isnan(generic[0]).any() and np.array_equal(generic[2].cpu().numpy(), RAGGED)
    assert int((generic[1] & 0x3fffffff).max()) > 2  # the hard clips iterate: not a trivial comparison
    _same(shaped, generic)


def test_ragged_blocks_at_slice_ends(run, dev, cm):
    """2 x 2 clips of 23 frames cut into slices of 1, 3, 4, 5 and 8 frames: a slice starts its own blocks at its first frame, and its
    last block ends with the slice (slice 8: the 7-frame last slice has a block of three)."""
    pos, quat, sc, offs = _clips(cm, [23] * 4)
    solve = _solver(dev, pos, quat, sc, make_items(offs))
    whole, how = run(True, solve)
    assert how == [("solve", "generic")] and not torch.isnan(whole[0]).any()
    for slice_len in (1, 3, 4, 5, 8):
        sliced, how = run(False, solve, balance="1", slice_len=slice_len)
        assert how == [("sliced", SHAPED)], slice_len
        _same(sliced, whole)


@pytest.mark.parametrize("poisoned", [1, 0])
def test_neighbours_do_not_leak(run, dev, cm, poisoned):
    """Two clips of 6 frames, adjacent in the key-point arrays: the block that holds the last two frames of the first clip must not
    read the second clip's rows, nor the other way round.  One clip's rows are NaN: the other clip's output does not change, the
    poisoned clip's frames carry the non-finite bit."""
    pos, quat, sc, offs = _clips(cm, [6, 6])
    items = make_items(offs)
    clean, how = run(False, _solver(dev, pos, quat, sc, items))
    assert how == [("solve", SHAPED)]
    pos2, quat2 = pos.copy(), quat.copy()
    pos2[6 * poisoned:6 * poisoned + 6] = np.nan
    quat2[6 * poisoned:6 * poisoned + 6] = np.nan
    dirty, how = run(False, _solver(dev, pos2, quat2, sc, items))
    assert how == [("solve", SHAPED)]
    mine = slice(6 * (1 - poisoned), 6 * (1 - poisoned) + 6)
    theirs = slice(6 * poisoned, 6 * poisoned + 6)
    assert not torch.isnan(clean[0]).any()
    assert torch.equal(clean[0][mine], dirty[0][mine]) and torch.equal(clean[1][mine], dirty[1][mine])
    assert bool(((dirty[1][theirs] >> 31) & 1).all()) and not bool(((dirty[1][mine] >> 31) & 1).any())
    generic, _ = run(True, _solver(dev, pos2, quat2, sc, items))
    assert torch.equal(dirty[1], generic[1]) and torch.equal(dirty[0][mine], generic[0][mine])


@pytest.mark.parametrize("case", ["height_scale", "init_row", "frame_begin", "columns"])
def test_per_item_inputs(run, dev, cm, case):
    """What a block reads per item and per lane: the clip's height factor, the caller's start rows, a first frame that is no multiple
    of four in the key-point arrays, and float32 input whose slot columns are not the identity."""
    lengths = [9, 6, 11, 7]
    pos, quat, sc, offs = _clips(cm, lengths)
    items, qi = make_items(offs), None
    if case == "height_scale":
        items = make_items(offs, height_scales=[0.85, 1.0, 1.1, 0.93])
    elif case == "init_row":
        rng = np.random.default_rng(7)
        qi = np.tile(np.asarray(cm.robot.qpos0, dtype=np.float64), (len(lengths), 1))
        qi[:, 7:] += rng.uniform(-0.05, 0.05, size=qi[:, 7:].shape)
        qi[:, :2] += rng.uniform(-0.2, 0.2, size=(len(lengths), 2))
        items["init_row"] = np.arange(len(lengths))
    elif case == "frame_begin":  # every item leaves out its clip's first frames: begins 3, 10, 17, 27
        items["frame_begin"] += [3, 1, 2, 1]
        items["n_out"] -= [3, 1, 2, 1]
        assert np.all(items["frame_begin"] % 4 != 0)
    elif case == "columns":  # the bodies in another order, with two unused columns in front
        rng = np.random.default_rng(8)
        perm = rng.permutation(pos.shape[1])
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(perm))
        pad_p, pad_q = np.full((pos.shape[0], 2, 3), 7.0, np.float32), np.tile(np.float32([0.5, 0.5, 0.5, 0.5]), (pos.shape[0], 2, 1))
        pos, quat = np.concatenate([pad_p, pos[:, perm]], 1), np.concatenate([pad_q, quat[:, perm]], 1)
        sc = (inv[np.asarray(sc)] + 2).astype(np.int32)
        assert not np.array_equal(sc, np.arange(len(sc)))
    solve = _solver(dev, pos, quat, sc, items, qi)
    shaped, how_s = run(False, solve)
    generic, how_g = run(True, solve)
    assert how_s == [("solve", SHAPED)] and how_g == [("solve", "generic")]
    assert np.array_equal(generic[2].cpu().numpy(), items["n_out"])
    covered = np.concatenate([np.arange(b, b + n) for b, n in zip(items["frame_begin"], items["n_out"])])
    assert not torch.isnan(generic[0][covered]).any()
    for a, b in zip(shaped[:2], generic[:2]):
        assert torch.equal(a[covered], b[covered])
    assert torch.equal(shaped[2], generic[2])


def test_probe_instance(run, dev, cm):
    """plan_order with 5 probe frames on the ragged batch.  The probe's costs are not returned, its order is: items by
    cost x frames / probed frames, most expensive first, in 4096 buckets.  The cost of an item is the number of solves of its first
    frames, which the solve reports (and which is equal under both settings, test_ragged_blocks_whole_clip), so the order each
    setting plans must be the one those costs imply -- the same costs under both settings."""
    pos, quat, sc, offs = _clips(cm, RAGGED)
    items = make_items(offs)
    tp, tq = torch.from_numpy(pos).to(dev), torch.from_numpy(quat).to(dev)
    pf = 5

    def plan(eng):
        return eng.plan_order(tp, tq, sc, items, probe_frames=pf), eng.ik_solve(tp, tq, sc, items, launch_order=None)[1]

    for generic_shape in (False, True):
        name = "generic" if generic_shape else SHAPED
        (order, it), how = run(generic_shape, plan)
        assert how == [("probe", name), ("solve", name)]
        order, it = order.cpu().numpy(), it.cpu().numpy() & 0x3fffffff
        assert np.array_equal(np.sort(order), np.arange(len(items)))
        probed = np.minimum(pf, RAGGED)
        cost = np.array([it[offs[c]:offs[c] + probed[c]].sum() for c in range(len(RAGGED))])
        key = cost.astype(np.float32) * np.asarray(RAGGED, np.float32) / probed.astype(np.float32)
        bucket = 4095 - np.minimum(4095, (key * (np.float32(4095.0) / key.max())).astype(np.int32))
        assert len(set(bucket.tolist())) >= 8  # the order is (all but) determined by the costs
        assert np.all(np.diff(bucket[order]) >= 0)


def test_bits_of_the_parent_commit(run, dev, cm):
    """The recorded bits of the commit before target_prep_slot (3 easy + 3 hard clips of 40 frames, the generator and seeds of
    tools/record_ik_bits.py): the shaped, the generic, the sliced (slice 5) and the group-of-one launch all reproduce them."""
    g = np.load(GOLDEN)
    assert len(str(g["commit"])) >= 7
    n_each, T = int(g["n_each"]), int(g["frames"])
    pe, qe, names, _, _ = synth.synth_clips(cm, n_each, T, seed=int(g["seeds"][0]), hard=False, dtype=np.float32)
    ph, qh, _, _, _ = synth.synth_clips(cm, n_each, T, seed=int(g["seeds"][1]), hard=True, dtype=np.float32)
    pos, quat, sc = np.concatenate([pe, ph]), np.concatenate([qe, qh]), cm.slot_columns(names)
    items = make_items(np.arange(2 * n_each + 1, dtype=np.int64) * T)
    want_q, want_it = torch.from_numpy(g["qpos"]).to(dev), torch.from_numpy(g["iters"]).to(dev)
    solve = _solver(dev, pos, quat, sc, items)
    for generic_shape, balance, slice_len, how_want in ((False, "0", None, ("solve", SHAPED)), (True, "0", None, ("solve", "generic")),
                                                        (False, "1", 5, ("sliced", SHAPED))):
        (q, it, _), how = run(generic_shape, solve, balance=balance, slice_len=slice_len)
        assert how == [how_want]
        assert torch.equal(q, want_q) and torch.equal(it, want_it), how_want
    grp = EngineGroup([cm], 0)
    q, it = grp.ik_solve([(torch.from_numpy(pos).to(dev), torch.from_numpy(quat).to(dev), sc, items)])[0][:2]
    torch.cuda.synchronize()
    assert torch.equal(q, want_q) and torch.equal(it, want_it), "group of one"
    grp.close()

"""Shared stage tables: the shaped IK instances read a stage's tables (task bodies, slots, composites, the resolved
composite-plan addresses) once per work item -- per slice in the sliced launch -- and exchange the two tables' weight pairs at every
stage boundary, instead of loading all of it at the top of every stage; their solves also read ``tol``, ``max_iter`` and ``limit_gain``
once at the top instead of in front of each use.  No floating-point statement moved, so every comparison here
is ``torch.equal`` on qpos, the solve words and ``frames_done``: against the generic instance, which still reads its tables per stage,
and against the recorded bits of an earlier commit (``tests/golden/ik_g1_smplx_parent_bits.npz``, read only).

Robot ``unitree_g1`` / ``smplx``; clips of 1, 2, 3, 5 and 40 frames from ``synth.synth_clips`` with the seeds of
tests/test_gpu_ik_target_blocks.py, once easy and once hard (two frames are the least that exercise the exchange back to table 0 at the
top of a frame; the hard clips have stages of several solves and an active working set).  The reference is computed once per module.
"""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gmr_amd import synth  # noqa: E402
from gmr_amd.engine import Engine  # noqa: E402
from gmr_amd.schedule import make_items  # noqa: E402
from tests.util import compiled  # noqa: E402

SHAPED = "IkShapeG1Smplx"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ik_g1_smplx_parent_bits.npz")
LENGTHS = [1, 2, 3, 5, 40]
SEEDS = (41, 42)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cm():
    return compiled("smplx", "unitree_g1")


def _launch(cm, fn, generic_shape=False, balance="0", slice_len=None, taper=None):
    """fn(engine)'s result and the (kind, instance, rest of the line) of every IK launch it made, under one setting of the library's
    switches (read at model creation and per call: a fresh Engine, the environment put back afterwards)."""
    env = dict(GMR_DEBUG_PLAN="1", GMR_AMD_GENERIC_SHAPE="1" if generic_shape else "0", GMR_AMD_BALANCE=balance,
               GMR_AMD_BALANCE_SLICE=None if slice_len is None else str(slice_len), GMR_AMD_BALANCE_TAPER=None if taper is None else str(taper))
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        eng = Engine(cm, 0)
        res = fn(eng)
        torch.cuda.synchronize()
        assert eng.sliced_timeouts == 0
        eng.close()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return res


@pytest.fixture
def run(capfd, cm):
    def go(fn, **kw):
        capfd.readouterr()
        res = _launch(cm, fn, **kw)
        return res, re.findall(r"gmr: ik launch: (\w+) instance (\w+)(.*)", capfd.readouterr().err)
    return go


@pytest.fixture(scope="module")
def batch(cm, dev):
    """The ten clips (lengths LENGTHS easy, then LENGTHS hard) on the device, their items, and the generic instance's whole-clip result."""
    lengths, T = LENGTHS + LENGTHS, max(LENGTHS)
    pe, qe, names, _, _ = synth.synth_clips(cm, len(LENGTHS), T, seed=SEEDS[0], hard=False, dtype=np.float32)
    ph, qh, names_h, _, _ = synth.synth_clips(cm, len(LENGTHS), T, seed=SEEDS[1], hard=True, dtype=np.float32)
    assert names == names_h
    keep = np.concatenate([np.arange(c * T, c * T + ln) for c, ln in enumerate(lengths)])
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    pos, quat = torch.from_numpy(np.concatenate([pe, ph])[keep]).to(dev), torch.from_numpy(np.concatenate([qe, qh])[keep]).to(dev)
    sc, items = cm.slot_columns(names), make_items(offs)

    def solve(eng):
        fd = torch.full((len(items),), -1, dtype=torch.int32, device=dev)
        q, it, _ = eng.ik_solve(pos, quat, sc, items, frames_done=fd, launch_order=None)
        return q, it, fd

    want = _launch(cm, solve, generic_shape=True)
    assert not torch.isnan(want[0]).any() and np.array_equal(want[2].cpu().numpy(), lengths)
    solves = (want[1] & 0x3fffffff).cpu().numpy()
    assert solves.min() >= 2 and solves.max() > 4  # two stages in every frame; the hard clips iterate
    return dict(pos=pos, quat=quat, sc=sc, items=items, offs=offs, lengths=lengths, solve=solve, want=want)


def _same(a, b):
    for x, y, what in zip(a, b, ("qpos", "solve words", "frames_done")):
        assert torch.equal(x, y), what


def test_whole_clips(run, batch):
    got, how = run(batch["solve"])
    assert [h[:2] for h in how] == [("solve", SHAPED)]
    _same(got, batch["want"])


@pytest.mark.parametrize("taper", [0, 1], ids=["uniform", "tapered"])
@pytest.mark.parametrize("slice_len", [1, 3, 4, 5])
def test_slices(run, batch, slice_len, taper):
    """Every slice rebuilds the per-item state (tables, both weight pairs in table-0 order, plan addresses) before its first frame:
    40 frames in slices of 1, 3, 4 and 5, uniform and with the last slice_len frames tapered down to one-frame slices."""
    got, how = run(batch["solve"], balance="1", slice_len=slice_len, taper=taper)
    assert [h[:2] for h in how] == [("sliced", SHAPED)]
    tapered = ", no taper" not in how[0][2]
    assert tapered == (taper == 1), how  # (a one-frame slice "tapers" to itself: 1)
    _same(got, batch["want"])


def test_probe(run, batch):
    """The probe's shaped instance shares ik_body: plan_order with 5 probe frames.  Its costs are not returned, its order is -- items
    by cost x frames / probed frames in 4096 buckets, most expensive first -- and an item's cost is the number of solves of its first
    frames, which the solve reports and which is equal under both settings (test_whole_clips).  So both settings must plan an order
    that those costs imply: the same costs."""
    items, offs, lengths, pf = batch["items"], batch["offs"], batch["lengths"], 5

    def plan(eng):
        return eng.plan_order(batch["pos"], batch["quat"], batch["sc"], items, probe_frames=pf)

    it = (batch["want"][1] & 0x3fffffff).cpu().numpy()
    probed = np.minimum(pf, lengths)
    cost = np.array([it[offs[c]:offs[c] + probed[c]].sum() for c in range(len(lengths))])
    key = cost.astype(np.float32) * np.asarray(lengths, np.float32) / probed.astype(np.float32)
    bucket = 4095 - np.minimum(4095, (key * (np.float32(4095.0) / key.max())).astype(np.int32))
    assert len(set(bucket.tolist())) >= 5  # five lengths: the order is largely determined by the costs
    for generic_shape in (False, True):
        order, how = run(plan, generic_shape=generic_shape)
        assert [h[:2] for h in how] == [("probe", "generic" if generic_shape else SHAPED)]
        order = order.cpu().numpy()
        assert np.array_equal(np.sort(order), np.arange(len(items)))
        assert np.all(np.diff(bucket[order]) >= 0), (generic_shape, order, bucket)


def test_recorded_bits(run, cm, dev):
    """3 easy + 3 hard clips of 40 frames (the generator and seeds of tools/record_ik_bits.py): the whole-clip and a tapered sliced
    launch of the shaped instance reproduce the recorded bits exactly."""
    g = np.load(GOLDEN)
    n_each, T = int(g["n_each"]), int(g["frames"])
    pe, qe, names, _, _ = synth.synth_clips(cm, n_each, T, seed=int(g["seeds"][0]), hard=False, dtype=np.float32)
    ph, qh, _, _, _ = synth.synth_clips(cm, n_each, T, seed=int(g["seeds"][1]), hard=True, dtype=np.float32)
    pos, quat = torch.from_numpy(np.concatenate([pe, ph])).to(dev), torch.from_numpy(np.concatenate([qe, qh])).to(dev)
    sc, items = cm.slot_columns(names), make_items(np.arange(2 * n_each + 1, dtype=np.int64) * T)
    want_q, want_it = torch.from_numpy(g["qpos"]).to(dev), torch.from_numpy(g["iters"]).to(dev)
    solve = lambda eng: eng.ik_solve(pos, quat, sc, items, launch_order=None)[:2]  # noqa: E731
    for kw, kind in ((dict(), "solve"), (dict(balance="1", slice_len=4, taper=1), "sliced")):
        (q, it), how = run(solve, **kw)
        assert [h[:2] for h in how] == [(kind, SHAPED)]
        assert torch.equal(q, want_q) and torch.equal(it, want_it), kind

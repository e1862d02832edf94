"""Control code of the solve loop ("Control code of the solve"): in the plain shaped IK instances the structured QP sets its
start point and working set with selects instead of a nest of branches, the task block's store region (lanes 0..2 of every quad) is
entered from a literal lane mask, and the integrate step compares its two dof-kind predicates where it uses them.  None of it is
arithmetic, so every comparison here is ``torch.equal`` on qpos, the solve words and ``frames_done``: against the generic instance, whose
code did not change, and against the recorded bits of an earlier commit (``tests/golden/ik_g1_smplx_parent_bits.npz``, read only).

Robot ``unitree_g1`` / ``smplx``, float32 key-points, through the ``Engine`` calls of tests/test_gpu_ik_stage_shared.py: clips of 1, 2,
3, 5 and 40 frames from ``synth.synth_clips`` with that test's seeds, easy and hard, and the six recorded clips of 40 frames; whole
clips, slices of 1, 3, 4 and 5 frames with and without taper, the probe's order.  The generic instance runs in a fresh ``Engine`` of this
process under ``GMR_AMD_GENERIC_SHAPE=1`` (the switch is read at model creation), as in tests/test_gpu_ik_shapes.py,
tests/test_gpu_ik_target_blocks.py and tests/test_gpu_ik_stage_shared.py.  Both references are computed once per module.

Every arm of the QP entry is reached.  ``status == 1 / 2`` carried into a solve, and with it the working-set path (about 4 % of the
benchmark's solves): the third recorded hard clip ends 39 of its 40 frames with a hinge exactly on a bound of its joint range, checked
against the CPU oracle's solution when this test was written and asserted below from the recorded qpos, so the test fails if that
stops.  ``lo > 0`` / ``hi < 0`` with a free dof: clips that start from a caller's row with hinges outside their ranges
(test_start_outside_the_range; asserted from the start rows).
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
SENTINEL = -777.25  # what the output rows hold before a launch that must leave some of them alone


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cm():
    return compiled("smplx", "unitree_g1")


def _launch(cm, fn, generic_shape=False, balance="0", slice_len=None, taper=None):
    """fn(engine)'s result under one setting of the library's switches (read at model creation and per call: a fresh Engine, the
    environment put back afterwards)."""
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


def _solver(dev, pos, quat, sc, items):
    def solve(eng):
        fd = torch.full((len(items),), -1, dtype=torch.int32, device=dev)
        q, it, _ = eng.ik_solve(pos, quat, sc, items, frames_done=fd, launch_order=None)
        return q, it, fd
    return solve


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
    solve = _solver(dev, pos, quat, sc, items)
    want = _launch(cm, solve, generic_shape=True)
    assert not torch.isnan(want[0]).any() and np.array_equal(want[2].cpu().numpy(), lengths)
    solves = (want[1] & 0x3fffffff).cpu().numpy()
    assert solves.min() >= 2 and solves.max() > 4  # two stages in every frame; the hard clips iterate
    return dict(pos=pos, quat=quat, sc=sc, items=items, offs=offs, lengths=lengths, solve=solve, want=want)


@pytest.fixture(scope="module")
def recorded(cm, dev):
    """The 3 easy + 3 hard clips of 40 frames of tools/record_ik_bits.py on the device, and their recorded qpos and solve words."""
    g = np.load(GOLDEN)
    n_each, T = int(g["n_each"]), int(g["frames"])
    pe, qe, names, _, _ = synth.synth_clips(cm, n_each, T, seed=int(g["seeds"][0]), hard=False, dtype=np.float32)
    ph, qh, _, _, _ = synth.synth_clips(cm, n_each, T, seed=int(g["seeds"][1]), hard=True, dtype=np.float32)
    pos, quat = torch.from_numpy(np.concatenate([pe, ph])).to(dev), torch.from_numpy(np.concatenate([qe, qh])).to(dev)
    sc, items = cm.slot_columns(names), make_items(np.arange(2 * n_each + 1, dtype=np.int64) * T)
    lengths = torch.full((2 * n_each,), T, dtype=torch.int32, device=dev)
    want = (torch.from_numpy(g["qpos"]).to(dev), torch.from_numpy(g["iters"]).to(dev), lengths)
    return dict(solve=_solver(dev, pos, quat, sc, items), want=want, qpos=g["qpos"], frames=T)


def _same(a, b):
    for x, y, what in zip(a, b, ("qpos", "solve words", "frames_done")):
        assert torch.equal(x, y), what


def test_working_set_path_is_reached(cm, recorded):
    """Some recorded row ends with a limited hinge on a bound of its range: its solves pinned that dof, i.e. went through the QP's
    working-set entry (status != 0), the block the selects replace.  (G1's hinges: 29, all limited.)"""
    r = cm.robot
    jt, lim, adr, rng = np.asarray(r.jnt_type), np.asarray(r.jnt_limited).astype(bool), np.asarray(r.qpos_adr), np.asarray(r.jnt_range)
    hinge = np.where((jt == 1) & lim & (adr >= 7))[0]
    assert len(hinge) == 29
    q = recorded["qpos"][:, adr[hinge]]
    on_bound = (q == rng[hinge, 0]) | (q == rng[hinge, 1])
    per_clip = on_bound.any(axis=1).reshape(-1, recorded["frames"]).sum(axis=1)
    assert per_clip.max() >= 10, per_clip  # (39 of the 40 frames of the last hard clip when this was written)
    assert per_clip[:len(per_clip) // 2].sum() == 0, per_clip  # the easy clips stay inside their ranges: both kinds of solve are compared


def test_whole_clips(run, batch, recorded):
    for data in (batch, recorded):
        got, how = run(data["solve"])
        assert [h[:2] for h in how] == [("solve", SHAPED)]
        _same(got, data["want"])


def test_generic_instance_equals_recorded_bits(run, recorded):
    """The reference of the other tests, itself against the record: the generic instance's code is the parent's, line for line."""
    got, how = run(recorded["solve"], generic_shape=True)
    assert [h[:2] for h in how] == [("solve", "generic")]
    _same(got, recorded["want"])


@pytest.mark.parametrize("taper", [0, 1], ids=["uniform", "tapered"])
@pytest.mark.parametrize("slice_len", [1, 3, 4, 5])
def test_slices(run, batch, recorded, slice_len, taper):
    """Every slice rebuilds the per-item state before its first frame and resumes the QP's working set of every lane from its
    predecessor's record: 40 frames in slices of 1, 3, 4 and 5, uniform and with the last slice_len frames tapered."""
    for data in (batch, recorded):
        got, how = run(data["solve"], balance="1", slice_len=slice_len, taper=taper)
        assert [h[:2] for h in how] == [("sliced", SHAPED)]
        assert (", no taper" not in how[0][2]) == (taper == 1), how  # (a one-frame slice "tapers" to itself: 1)
        _same(got, data["want"])


def test_probe(run, batch):
    """The probe's shaped instance shares ik_body.  Its costs are not returned, its order is -- items by cost x frames / probed frames in
    4096 buckets, most expensive first -- and an item's cost is the number of solves of its first frames, which the solve reports and
    which is equal under both settings (test_whole_clips).  So both settings must plan an order that those costs imply."""
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


@pytest.mark.parametrize("sliced", [False, True], ids=["whole", "sliced"])
def test_empty_and_one_frame_items(run, cm, dev, sliced):
    """Items of 1, 0, 1, 0 and 2 frames over key-point rows laid out as five clips of two frames (easy, hard, hard, easy, hard).  The
    rows no item covers are NaN in the input and hold a sentinel in the output arrays: an empty item solves nothing, reports
    frames_done = 0 and its start state (its final row is qpos0), a one-frame item writes its row and nothing beside it, and the
    covered rows, the start rows and the final rows are the generic instance's, bit for bit -- with the neighbours clean or poisoned."""
    n, T = 5, 2
    pe, qe, names, _, _ = synth.synth_clips(cm, n, T, seed=SEEDS[0], hard=False, dtype=np.float32)
    ph, qh, _, _, _ = synth.synth_clips(cm, n, T, seed=SEEDS[1], hard=True, dtype=np.float32)
    hard = np.repeat([False, True, True, False, True], T)[:, None, None]
    pos, quat = np.where(hard, ph, pe), np.where(hard, qh, qe)
    n_out = np.array([1, 0, 1, 0, 2])
    items = make_items(np.arange(n + 1, dtype=np.int64) * T, track=True)
    assert len(items) == n
    items["n_out"] = n_out
    covered = np.concatenate([np.arange(c * T, c * T + k) for c, k in enumerate(n_out)])
    bare = np.setdiff1d(np.arange(n * T), covered)
    pos_p, quat_p = pos.copy(), quat.copy()
    pos_p[bare], quat_p[bare] = np.nan, np.nan
    sc = cm.slot_columns(names)

    def solver(p, q):
        tp, tq = torch.from_numpy(p).to(dev), torch.from_numpy(q).to(dev)

        def solve(eng):
            out = torch.full((n * T, eng.nq), SENTINEL, dtype=torch.float64, device=dev)
            it = torch.full((n * T,), -5, dtype=torch.int32, device=dev)
            fd = torch.full((n,), -1, dtype=torch.int32, device=dev)
            out, it, fin = eng.ik_solve(tp, tq, sc, items, n_final=2 * n, out=out, iters=it, frames_done=fd, launch_order=None)
            return out, it, fd, fin
        return solve

    kw = dict(balance="1", slice_len=1, taper=0) if sliced else dict()
    want, how = run(solver(pos, quat), generic_shape=True, **kw)
    assert [h[:2] for h in how] == [("sliced" if sliced else "solve", "generic")]
    assert np.array_equal(want[2].cpu().numpy(), n_out)
    assert not torch.isnan(want[0][covered]).any() and int((want[1][covered] & 0x3fffffff).min()) >= 2
    qpos0 = torch.from_numpy(np.asarray(cm.robot.qpos0, dtype=np.float64)).to(dev)
    for c in np.where(n_out == 0)[0]:
        assert torch.equal(want[3][c], qpos0)  # the final state of an empty item is its start state
    for p, q in ((pos, quat), (pos_p, quat_p)):
        got, how = run(solver(p, q), **kw)
        assert [h[:2] for h in how] == [("sliced" if sliced else "solve", SHAPED)]
        assert torch.equal(got[2], want[2])
        assert torch.equal(got[0][covered], want[0][covered]) and torch.equal(got[1][covered], want[1][covered])
        assert bool((got[0][bare] == SENTINEL).all()) and bool((got[1][bare] == -5).all())  # the rows beside stay as they were
        assert not bool(((got[1][covered] >> 31) & 1).any())  # no frame saw a poisoned row
        assert torch.equal(got[3][:n], want[3][:n])  # final rows
        started = np.where(n_out > 0)[0]
        assert torch.equal(got[3][n + started], want[3][n + started])  # start rows (written by the first output frame)


@pytest.mark.parametrize("sliced", [False, True], ids=["whole", "sliced"])
def test_start_outside_the_range(run, cm, dev, sliced):
    """The two arms of the QP entry that pin a FREE dof: a dof enters its first solve with status 0 and a violated bound -- below its
    range ``lo = -gain (q - lower) > 0``, above it ``hi = gain (upper - q) < 0`` -- when the clip starts from a caller's row outside
    the joint ranges.  Four clips of 3, 5, 2 and 4 frames (two easy, two hard); in every start row three limited hinges sit 0.2 rad
    below their range and three others 0.2 rad above it (asserted here from the rows).  Shaped against generic, bit for bit."""
    lengths, T = [3, 5, 2, 4], 5
    pe, qe, names, _, _ = synth.synth_clips(cm, 2, T, seed=SEEDS[0], hard=False, dtype=np.float32)
    ph, qh, _, _, _ = synth.synth_clips(cm, 2, T, seed=SEEDS[1], hard=True, dtype=np.float32)
    keep = np.concatenate([np.arange(c * T, c * T + ln) for c, ln in enumerate(lengths)])
    pos, quat = torch.from_numpy(np.concatenate([pe, ph])[keep]).to(dev), torch.from_numpy(np.concatenate([qe, qh])[keep]).to(dev)
    items = make_items(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64))
    items["init_row"] = np.arange(len(lengths))
    r = cm.robot
    jt, lim, adr, rng = np.asarray(r.jnt_type), np.asarray(r.jnt_limited).astype(bool), np.asarray(r.qpos_adr), np.asarray(r.jnt_range)
    hinge = np.where((jt == 1) & lim & (adr >= 7))[0]
    qi = np.tile(np.asarray(r.qpos0, dtype=np.float64), (len(lengths), 1))
    pick = np.random.default_rng(11)
    for c in range(len(lengths)):
        six = pick.choice(hinge, size=6, replace=False)
        qi[c, adr[six[:3]]] = rng[six[:3], 0] - 0.2
        qi[c, adr[six[3:]]] = rng[six[3:], 1] + 0.2
    below, above = qi[:, adr[hinge]] < rng[hinge, 0], qi[:, adr[hinge]] > rng[hinge, 1]
    assert np.all(below.sum(axis=1) == 3) and np.all(above.sum(axis=1) == 3)
    qinit, sc = torch.from_numpy(qi).to(dev), cm.slot_columns(names)

    def solve(eng):
        fd = torch.full((len(items),), -1, dtype=torch.int32, device=dev)
        q, it, _ = eng.ik_solve(pos, quat, sc, items, qpos_init=qinit, frames_done=fd, launch_order=None)
        return q, it, fd

    kw = dict(balance="1", slice_len=2, taper=0) if sliced else dict()
    want, how = run(solve, generic_shape=True, **kw)
    assert [h[:2] for h in how] == [("sliced" if sliced else "solve", "generic")]
    assert not torch.isnan(want[0]).any() and np.array_equal(want[2].cpu().numpy(), lengths)
    q1 = want[0][np.cumsum([0] + lengths[:-1])].cpu().numpy()[:, adr[hinge]]  # every clip's first frame: the solver moved the six dofs back in
    assert np.all(q1[below] > qi[:, adr[hinge]][below]) and np.all(q1[above] < qi[:, adr[hinge]][above])
    got, how = run(solve, **kw)
    assert [h[:2] for h in how] == [("sliced" if sliced else "solve", SHAPED)]
    _same(got, want)

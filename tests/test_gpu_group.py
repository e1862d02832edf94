"""Multi-robot batch retargeting on the GPU: group chunking (EngineGroup.ik_solve_chunked), the cost-ordered group launch
(gmr_group_plan_order / gmr_group_ik_solve_ordered), the host-side refusals of group batches with state rows, and the public
MultiRobotRetargeting class against one GeneralMotionRetargeting per robot."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gmr_amd import synth  # noqa: E402
from gmr_amd.schedule import make_items, plan_walks  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402
from tests.util import compiled  # noqa: E402

ROBOTS = ["unitree_g1", "booster_t1", "stanford_toddy", "fourier_n1", "engineai_pm01"]  # BASELINE config 4
MASK = 0x3FFFFFFF


def _group(robots=ROBOTS):
    from gmr_amd.engine import EngineGroup
    return EngineGroup([compiled("smplx", r) for r in robots], 0)


def _shared_input(n_clips, T, seed=61):
    """One human input for every robot (G1's synthetic clips: the five config-4 robots read the same 14 bodies)."""
    g1 = compiled("smplx", "unitree_g1")
    pos, quat, names, offs, _ = synth.synth_clips(g1, n_clips, T, seed=seed, hard=True, dtype=np.float32)
    return pos, quat, names, np.asarray(offs, dtype=np.int64)


def _hinge_limits(cm):
    r = cm.robot
    hb = sorted(r.hinge_bodies(), key=lambda b: r.qpos_adr[b])
    lim = np.array(r.jnt_range, dtype=np.float64)[hb]
    return lim[:, 0], lim[:, 1]


def _check_invariants(cm, q, iters, n_frames):
    """test_gpu_configs' invariants: no QP cap, solve counts in [2, 22], finite, hinges inside their ranges, unit root quaternion."""
    it = iters & MASK
    assert int((iters >> 30).sum().item()) == 0, "a QP hit its iteration cap"
    assert int(it.min().item()) >= 2 and int(it.max().item()) <= 22
    assert q.shape == (n_frames, cm.robot.nq) and bool(torch.isfinite(q).all().item())
    lo, hi = _hinge_limits(cm)
    lo_t, hi_t = torch.from_numpy(lo).to(q.device), torch.from_numpy(hi).to(q.device)
    hinges = q[:, 7:]
    assert float((lo_t - hinges).max().item()) <= 1e-9 and float((hinges - hi_t).max().item()) <= 1e-9
    assert float((q[:, 3:7].norm(dim=1) - 1.0).abs().max().item()) < 1e-12


def test_group_chunked_equals_member_chunked_bitwise():
    grp = _group()
    pos, quat, names, offs = _shared_input(16, 400)
    tp, tq = torch.from_numpy(pos).to(grp.device), torch.from_numpy(quat).to(grp.device)
    cols = [compiled("smplx", r).slot_columns(names) for r in ROBOTS]
    res = grp.ik_solve_chunked([(tp, tq, c, offs) for c in cols], 16, 24)
    whole = grp.ik_solve([(tp, tq, c, make_items(offs)) for c in cols])
    torch.cuda.synchronize()
    for r, eng, c, (q, it, info), (qw, itw) in zip(ROBOTS, grp.engines, cols, res, whole):
        q1, it1, info1 = eng.ik_solve_chunked(tp, tq, c, offs, 16, 24)
        assert torch.equal(q, q1) and torch.equal(it, it1), r
        assert info == info1 and info["chunks"] == 16 * 25, (r, info, info1)
        assert float((q - qw).abs().max().item()) < 1e-7, r
        assert torch.equal(it & MASK, itw & MASK), r
        cm = compiled("smplx", r)
        q_ref, it_ref, _ = Oracle(cm.blob).ik_solve(pos[:150], quat[:150], c, make_items([0, 150]))
        assert np.abs(q[:150].cpu().numpy() - q_ref).max() < 1e-6, r
        assert np.array_equal(it[:150].cpu().numpy() & MASK, it_ref), r
    grp.close()


def test_config4_full_size_auto_chunked():
    """5 robots x 64 clips x 1000 frames (bench.py's heterogeneous inputs) with chunk="auto": chunks over all members' clips."""
    grp = _group()
    dev = grp.device
    offs = np.arange(65, dtype=np.int64) * 1000
    batches = []
    for r in ROBOTS:
        cm = compiled("smplx", r)
        pos, quat, names, _, _ = synth.synth_clips(cm, 8, 1000, seed=41, hard=True, dtype=np.float32)
        rep = lambda a: torch.from_numpy(a).to(dev).repeat(8, 1, 1)  # noqa: E731
        batches.append((rep(pos), rep(quat), cm.slot_columns(names), offs))
    res = grp.ik_solve_chunked(batches, "auto", 0)
    chunk, burn_in = grp.last_chunk
    assert chunk > 0 and burn_in > 0
    whole = grp.ik_solve([(b[0], b[1], b[2], make_items(offs)) for b in batches])
    torch.cuda.synchronize()
    for r, (q, it, info), (qw, itw) in zip(ROBOTS, res, whole):
        cm = compiled("smplx", r)
        _check_invariants(cm, q, it, 64000)
        assert info["chunks"] == 64 * -(-1000 // chunk) and info["passes"] == 1
        assert float((q - qw).abs().max().item()) < 1e-7, r
        assert torch.equal(it & MASK, itw & MASK), r
    grp.close()


def test_ordered_group_launch_is_bitwise_the_array_order():
    from gmr_amd.engine import EngineError
    grp = _group()
    pos, quat, names, offs = _shared_input(12, 200, seed=62)
    tp, tq = torch.from_numpy(pos).to(grp.device), torch.from_numpy(quat).to(grp.device)
    cols = [compiled("smplx", r).slot_columns(names) for r in ROBOTS]
    # a member without work and members of unequal batch size
    cut = [None, 4, 12, 1, 7]
    batches = [None if k is None else (tp[:offs[k]], tq[:offs[k]], c, make_items(offs[:k + 1])) for k, c in zip(cut, cols)]
    total = sum(0 if k is None else k for k in cut)
    order = grp.plan_order(batches, probe_frames=8)
    assert order.dtype == torch.int32 and order.numel() == total
    assert sorted(order.cpu().tolist()) == list(range(total))
    ref = grp.ik_solve(batches)
    got = grp.ik_solve(batches, launch_order=order)
    rev = grp.ik_solve(batches, launch_order=torch.arange(total - 1, -1, -1, dtype=torch.int32, device=grp.device))
    torch.cuda.synchronize()
    assert ref[0] == (None, None) and got[0] == (None, None)
    for a, b, c in zip(ref[1:], got[1:], rev[1:]):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    # launch_order="auto" where the policy probes: 5 x 512 clips x 300 frames, more items than wavefront slots
    g1 = compiled("smplx", "unitree_g1")
    bp, bq, bnames, boffs = synth.synth_clips_torch(g1, np.full(512, 300), seed=63, device=grp.device, hard=True)
    boffs = np.asarray(boffs, dtype=np.int64)
    big = [(bp, bq, compiled("smplx", r).slot_columns(bnames), make_items(boffs)) for r in ROBOTS]
    assert grp.engines[0]._probe_frames(np.concatenate([b[3] for b in big])) > 0
    ref = grp.ik_solve(big)
    got = grp.ik_solve(big, launch_order="auto")
    torch.cuda.synchronize()
    for a, b in zip(ref, got):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # walks cannot be probed: gmr_group_plan_order says GMR_EINVAL
    items = make_items(offs, chunk=50, burn_in=10, track=True)
    walks = plan_walks(items, offs, 50)
    qf = torch.zeros((2 * len(items), grp.engines[1].nq), dtype=torch.float64, device=grp.device)
    wb = [None, {"pos": tp, "quat": tq, "slot_col": cols[1], "items": walks, "qpos_init": qf, "qpos_final": qf}, None, None, None]
    with pytest.raises(EngineError, match="gmr_group_plan_order: invalid argument"):
        grp.plan_order(wb)
    grp.close()


def test_group_refuses_bad_state_rows_before_any_launch():
    from gmr_amd.engine import EngineError
    grp = _group(ROBOTS[:2])
    pos, quat, names, offs = _shared_input(4, 100, seed=64)
    tp, tq = torch.from_numpy(pos).to(grp.device), torch.from_numpy(quat).to(grp.device)
    sc = compiled("smplx", ROBOTS[1]).slot_columns(names)
    nq = grp.engines[1].nq
    items = make_items(offs, chunk=25, burn_in=10, track=True)
    walks = plan_walks(items, offs, 25)
    n = len(items)
    out = torch.full((len(pos), nq), 7.0, dtype=torch.float64, device=grp.device)

    def batch(**kw):
        return [None, dict({"pos": tp, "quat": tq, "slot_col": sc, "out": out}, **kw)]
    qf = torch.zeros((2 * n, nq), dtype=torch.float64, device=grp.device)
    with pytest.raises(EngineError, match="member 1: init_row outside qpos_init"):
        grp.ik_solve(batch(items=walks, qpos_init=qf[:3], qpos_final=qf))
    with pytest.raises(EngineError, match="member 1: final_row outside qpos_final"):
        grp.ik_solve(batch(items=walks, qpos_init=qf, qpos_final=qf[:n]))
    with pytest.raises(EngineError, match="member 1: final_row outside qpos_final"):
        grp.ik_solve(batch(items=items, n_final=n))  # burn rows need 2 n
    with pytest.raises(EngineError, match="member 1: init_row outside qpos_init"):
        grp.ik_solve(batch(items=walks, qpos_final=qf))   # a walk without its start states
    with pytest.raises(EngineError, match="member 1: final_row outside qpos_final"):
        grp.ik_solve(batch(items=walks, qpos_init=qf))    # ... or without its final states
    with pytest.raises(EngineError, match="plain per-clip items"):
        grp.ik_solve([None, (tp, tq, sc, walks)])         # a tuple batch carries no state arrays
    plain = [None, (tp, tq, sc, make_items(offs))]
    with pytest.raises(EngineError, match="launch_order"):
        grp.ik_solve(plain, launch_order=torch.arange(3, dtype=torch.int32, device=grp.device))
    with pytest.raises(EngineError, match="launch_order"):
        grp.ik_solve(plain, launch_order=torch.arange(4, dtype=torch.int64, device=grp.device))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all().item())  # nothing was launched
    grp.close()


def _same(a, b, bitwise):
    if bitwise:
        return np.array_equal(a, b) if isinstance(a, np.ndarray) else torch.equal(a, b)
    d = np.abs(a - b).max() if isinstance(a, np.ndarray) else float((a - b).abs().max().item())
    return d < 1e-6


@pytest.mark.parametrize("chunk", [0, 16])
def test_multi_robot_retarget_batch_equals_one_retargeter_per_robot(chunk):
    from gmr_amd import GeneralMotionRetargeting, MultiRobotRetargeting
    mr = MultiRobotRetargeting("smplx", ROBOTS, device=0)
    assert mr.robots == ROBOTS and len(mr.engines) == 5
    assert set(mr.ik_columns) == set().union(*[compiled("smplx", r).slot_names for r in ROBOTS])
    pos, quat, names, offs = _shared_input(4, 120, seed=65)
    heights = [1.6, 1.75, 1.9, 1.8]
    # numpy input with more columns than the robots read: narrowed on the host
    xpos = np.concatenate([pos, pos[:, :3] + 0.5], axis=1)
    xquat = np.concatenate([quat, quat[:, :3]], axis=1)
    xnames = list(names) + ["extra_a", "extra_b", "extra_c"]
    tp, tq = torch.from_numpy(pos).cuda(), torch.from_numpy(quat).cuda()
    got_np, it_np = mr.retarget_batch(xpos, xquat, xnames, seq_offsets=offs, chunk=chunk, burn_in=24, human_heights=heights, return_iters=True)
    got_t = mr.retarget_batch(tp, tq, names, seq_offsets=offs, chunk=chunk, burn_in=24, human_heights=heights)
    assert isinstance(got_np["unitree_g1"], np.ndarray) and isinstance(got_t["unitree_g1"], torch.Tensor)
    for r, eng in zip(ROBOTS, mr.engines):
        one = GeneralMotionRetargeting("smplx", r, device=0)
        bitwise = one._engine.info.reserved[0] == eng.info.reserved[0]  # the group kept the member's own QP back end
        assert bitwise  # (true for the five config-4 robots)
        ref_np, rit = one.retarget_batch(xpos, xquat, xnames, seq_offsets=offs, chunk=chunk, burn_in=24, human_heights=heights, return_iters=True)
        ref_t = one.retarget_batch(tp, tq, names, seq_offsets=offs, chunk=chunk, burn_in=24, human_heights=heights)
        assert _same(got_np[r], ref_np, bitwise) and np.array_equal(it_np[r], rit), r
        assert _same(got_t[r], ref_t, bitwise), r
        assert mr.last_chunk_info[r] == one.last_chunk_info, r
    mr.close()


def test_multi_robot_planar_base_layout():
    from gmr_amd import GeneralMotionRetargeting, MultiRobotRetargeting
    robots = ["unitree_g1", "galaxea_r1pro"]
    mr = MultiRobotRetargeting("smplx", robots, device=0)
    pos, quat, names, offs = _shared_input(3, 90, seed=66)
    got = mr.retarget_batch(pos, quat, names, seq_offsets=offs)
    for r, eng in zip(robots, mr.engines):
        one = GeneralMotionRetargeting("smplx", r, device=0)
        ref = one.retarget_batch(pos, quat, names, seq_offsets=offs)
        assert got[r].shape == ref.shape, r
        assert _same(got[r], ref, one._engine.info.reserved[0] == eng.info.reserved[0]), r
    assert mr.models[1].planar_base and got["galaxea_r1pro"].shape == (270, mr.engines[1].nq - 4)  # [x, y, yaw, hinges]
    mr.close()

"""The per-solve step cap (``gmr_model_set_step_cap``; ``use_velocity_limit`` / ``velocity_limits`` of the retargeters) on the GPU.

Reference: tests/step_cap_reference.py -- the oracle's frame loop with the box intersected with the cap between ``build_qp`` and
``box_qp`` (tests/test_step_cap_host.py shows it is the oracle itself when the cap is +inf).  mink's ``VelocityLimit`` is not
available, so the capped result is pinned by that definition.  Tolerance as in test_gpu_parity.py for the same robots: 1e-6
(rad / m) with identical solve counts.

Every clip starts from ``qpos0``, which is what makes the cap bind; each case first shows on the CPU that the cap is active, that
the capped result is not the uncapped one, and that no stopping decision of the reference is a near tie.
"""
import functools
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gmr_amd import synth  # noqa: E402
from gmr_amd.engine import Engine, EngineError, IKParams  # noqa: E402
from gmr_amd.model import compile_model, resolve_velocity_limits, step_cap  # noqa: E402
from gmr_amd.schedule import make_items  # noqa: E402
from oracle.oracle import IKParams as OParams, Oracle  # noqa: E402
from tests.step_cap_reference import retarget_clips  # noqa: E402
from tests.util import compiled, quat_angle  # noqa: E402

SEED, CLIPS, FRAMES = 32, 3, 6
DENSE = "booster_t1"  # every registry robot takes the structured QP by itself: the dense box_qp path is GMR_AMD_GENERIC_QP=1 on this one
CASES = [("unitree_g1", "structured"), (DENSE, "generic"), ("galaxea_r1pro", "structured")]
INPUTS = [(np.float32, 0), (np.float32, 1), (np.float64, 0), (np.float64, 1)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    return torch.device("cuda", 0)


def _capped_cm(robot, use=True, limits=None):
    base = compiled("smplx", robot)
    return compile_model(base.robot, base.config, None, velocity_limits=resolve_velocity_limits(base.robot, use, limits))


def _qpos_diff(a, b):
    return max(np.abs(a[:, :3] - b[:, :3]).max(), quat_angle(a[:, 3:7], b[:, 3:7]).max(), np.abs(a[:, 7:] - b[:, 7:]).max())


def _check_preconditions(capped, uncapped, offs):
    """The inputs can tell a kernel that applies the cap from one that ignores it, and the reference's solve counts are stable."""
    for s in range(len(offs) - 1):
        a, b = int(offs[s]), int(offs[s + 1])
        assert sum(sum(f) for f in capped.active[a:b]) >= 1, f"clip {s}: the cap never binds"
        assert np.abs(capped.qpos[a:b] - uncapped.qpos[a:b]).max() > 1e-3, f"clip {s}: capped == uncapped"
    assert capped.margins.min() > 1e-6, capped.margins.min()


@functools.lru_cache(maxsize=None)
def _case(robot, dtype, otg, limits=None):
    """Inputs, cap and the CPU reference (capped and uncapped) of one case; computed once, shared, never modified."""
    cm = _capped_cm(robot, True, limits)
    pos, quat, names, offs, _ = synth.synth_clips(cm, CLIPS, FRAMES, seed=SEED, hard=True, dtype=dtype)
    sc = cm.slot_columns(names)
    orc = Oracle(cm.blob)
    prm = OParams(offset_to_ground=otg)
    ref = retarget_clips(cm, pos, quat, sc, offs, cap=cm.step_cap, params=prm, orc=orc)
    un = retarget_clips(cm, pos, quat, sc, offs, cap=None, params=prm, orc=orc)
    _check_preconditions(ref, un, offs)
    return cm, pos, quat, names, sc, offs, ref, un


def _solve(eng, pos, quat, sc, offs, dev, otg=0, **kw):
    q, it, _ = eng.ik_solve(torch.from_numpy(pos).to(dev), torch.from_numpy(quat).to(dev), sc, make_items(offs), params=IKParams(offset_to_ground=otg),
                            **{"launch_order": None, **kw})
    torch.cuda.synchronize()
    return q.cpu().numpy(), it.cpu().numpy()


def _assert_step_bound(cm, q, it, offs):
    """|q_k - q_{k-1}| <= solves_k * cap for every hinge and frame (q_{-1} = qpos0): holds whatever the reference says."""
    cap = cm.step_cap[6:]
    solves = (it & 0x3FFFFFFF).astype(np.float64)
    for s in range(len(offs) - 1):
        a, b = int(offs[s]), int(offs[s + 1])
        prev = np.concatenate([cm.robot.qpos0[None, 7:], q[a:b - 1, 7:]])
        step = np.abs(q[a:b, 7:] - prev)
        bound = solves[a:b, None] * cap[None, :] + 1e-12
        assert np.all(step <= bound), (s, float((step - bound).max()))


@pytest.mark.parametrize("dtype,otg", INPUTS)
@pytest.mark.parametrize("robot,qp", CASES)
def test_capped_solve_matches_the_reference(robot, qp, dtype, otg, dev, monkeypatch):
    monkeypatch.setenv("GMR_AMD_GENERIC_QP", "1" if qp == "generic" else "0")
    cm, pos, quat, names, sc, offs, ref, un = _case(robot, dtype, otg)
    eng = Engine(cm, 0)
    assert (eng.info.reserved[0] == 0) == (qp == "generic")  # core size of the structured layout, 0 = the dense box_qp
    assert np.array_equal(eng.step_cap, cm.step_cap)
    q, it = _solve(eng, pos, quat, sc, offs, dev, otg)
    d = _qpos_diff(q, ref.qpos)
    print(f"{robot} {qp} {np.dtype(dtype).name} otg={otg}: max |kernel - reference| = {d:.3e}, cap active in {ref.cap_active_solves()} of {int(ref.solves.sum())} solves, "
          f"capped vs uncapped {np.abs(ref.qpos - un.qpos).max():.3f} rad")
    assert (it >> 30).max() == 0, "a QP hit its iteration cap or a frame is non-finite"
    assert np.array_equal(it, ref.solves)
    assert d < 1e-6, d
    _assert_step_bound(cm, q, it, offs)
    if robot == "galaxea_r1pro":  # the null dofs and the untasked wheels stay where they are
        assert np.all(q[:, 2] == cm.robot.body_pos[0, 2]) and not q[:, 4:6].any()
    eng.close()


def test_a_looser_cap_binds_in_some_solves_only(dev):
    """60 rad/s on every hinge: the cap is active at the start of a clip and inactive once the robot has caught up."""
    cm, pos, quat, names, sc, offs, ref, un = _case("unitree_g1", np.float32, 0, 60.0)
    n_active = ref.cap_active_solves()
    assert 0 < n_active < int(ref.solves.sum())
    eng = Engine(cm, 0)
    q, it = _solve(eng, pos, quat, sc, offs, dev)
    assert np.array_equal(it, ref.solves) and _qpos_diff(q, ref.qpos) < 1e-6
    _assert_step_bound(cm, q, it, offs)
    eng.close()


def test_no_cap_null_cap_and_infinite_cap_are_one_result(dev, capfd, monkeypatch):
    """A model that never had a cap, one with set_step_cap(NULL), one with an all-inf cap (which runs the new code on the generic
    instance) and one whose cap was set and taken away again: bitwise equal qpos and solve counts."""
    monkeypatch.setenv("GMR_DEBUG_PLAN", "1")
    cm, pos, quat, names, sc, offs, ref, _ = _case("unitree_g1", np.float32, 0)
    plain = compiled("smplx", "unitree_g1")
    launches = lambda: re.findall(r"gmr: ik launch: (\w+) instance (\w+)", capfd.readouterr().err)  # noqa: E731
    for otg, dt in ((0, np.float32), (1, np.float64)):
        p, qd = pos.astype(dt), quat.astype(dt)
        never, null, inf, back = (Engine(plain, 0) for _ in range(4))
        null.set_step_cap(None)
        inf.set_step_cap(np.full(plain.robot.nv, np.inf))
        capfd.readouterr()
        q0, it0 = _solve(never, p, qd, sc, offs, dev, otg)
        first = launches()
        q1, it1 = _solve(null, p, qd, sc, offs, dev, otg)
        assert launches() == first
        q2, it2 = _solve(inf, p, qd, sc, offs, dev, otg)
        assert launches() == [("solve", "generic")]
        if otg == 0:
            assert first == [("solve", "IkShapeG1Smplx")]  # the uncapped plain launch is still the shaped instance
        back.set_step_cap(cm.step_cap)
        qc, itc = _solve(back, p, qd, sc, offs, dev, otg)
        assert launches() == [("solve", "generic")]
        assert np.abs(qc - q0).max() > 1e-3  # the cap did something ...
        back.set_step_cap(None)
        assert np.isinf(back.step_cap).all()
        q3, it3 = _solve(back, p, qd, sc, offs, dev, otg)
        assert launches() == first  # ... and is gone
        for q, it in ((q1, it1), (q2, it2), (q3, it3)):
            assert np.array_equal(q, q0) and np.array_equal(it, it0)
        for e in (never, null, inf, back):
            e.close()


def test_group_members_keep_their_own_caps(dev):
    """Two robots with different caps and one without, in one launch: each member equals its own single-model launch bit for bit."""
    from gmr_amd.multi_robot import MultiRobotRetargeting
    robots = ["unitree_g1", "booster_t1", "engineai_pm01"]
    mr = MultiRobotRetargeting("smplx", robots, velocity_limits={"unitree_g1": 3 * np.pi, "booster_t1": {"Left_Knee_Pitch": 4.0, "Right_Knee_Pitch": 4.0, "Waist": 30.0}})
    assert mr.velocity_limits["engineai_pm01"] is None and set(mr.velocity_limits["booster_t1"]) == {"Left_Knee_Pitch", "Right_Knee_Pitch", "Waist"}
    caps = [e.step_cap for e in mr.engines]
    assert np.isfinite(caps[0]).sum() == 29 and np.isfinite(caps[1]).sum() == 3 and np.isinf(caps[2]).all()
    batches, singles = [], []
    for r, cm, eng in zip(robots, mr._cms, mr.engines):
        pos, quat, names, offs, _ = synth.synth_clips(cm, CLIPS, FRAMES, seed=SEED, hard=True, dtype=np.float32)
        sc = cm.slot_columns(names)
        tp, tq = torch.from_numpy(pos).to(dev), torch.from_numpy(quat).to(dev)
        batches.append((tp, tq, sc, make_items(offs)))
        singles.append(eng.ik_solve(tp, tq, sc, make_items(offs), launch_order=None)[:2])  # the member's own launch, on its own handle
        if cm.step_cap is not None:  # ... which is the capped solve of the reference
            orc = Oracle(cm.blob)
            ref = retarget_clips(cm, pos, quat, sc, offs, cap=cm.step_cap, orc=orc)
            un = retarget_clips(cm, pos, quat, sc, offs, cap=None, orc=orc)
            _check_preconditions(ref, un, offs)
            q, it = singles[-1][0].cpu().numpy(), singles[-1][1].cpu().numpy()
            assert np.array_equal(it, ref.solves) and _qpos_diff(q, ref.qpos) < 1e-6, r
    got = mr.group.ik_solve(batches)
    torch.cuda.synchronize()
    for r, (q, it), (q1, it1) in zip(robots, got, singles):
        assert torch.equal(q, q1) and torch.equal(it, it1), r
    order = mr.group.plan_order(batches, probe_frames=2)
    for (q, it), (q1, it1) in zip(mr.group.ik_solve(batches, launch_order=order), singles):
        assert torch.equal(q, q1) and torch.equal(it, it1)
    mr.close()


def test_ordered_launch_equals_the_unordered_capped_solve(dev):
    """gmr_ik_plan_order + gmr_ik_solve_ordered under a cap: the probe runs capped too (costs = the capped solve counts)."""
    cm, pos, quat, names, sc, offs, ref, _ = _case("unitree_g1", np.float32, 0)
    eng = Engine(cm, 0)
    q0, it0 = _solve(eng, pos, quat, sc, offs, dev)
    tp, tq = torch.from_numpy(pos).to(dev), torch.from_numpy(quat).to(dev)
    order = eng.plan_order(tp, tq, sc, make_items(offs), probe_frames=2)
    o = order.cpu().numpy()
    assert np.array_equal(np.sort(o), np.arange(CLIPS))
    cost = ref.solves.reshape(CLIPS, FRAMES)[:, :2].sum(1)
    assert cost[o[0]] == cost.max() and cost[o[-1]] == cost.min()  # most expensive first, by the capped counts
    q1, it1 = _solve(eng, pos, quat, sc, offs, dev, launch_order=order)
    assert np.array_equal(q1, q0) and np.array_equal(it1, it0)
    assert np.array_equal(it0, ref.solves)
    eng.close()


@pytest.mark.parametrize("limits", [None, 100.0])
def test_chunked_solve_equals_the_sequential_capped_solve(limits, dev):
    """One 96-frame clip at an arbitrary heading in chunks of 16 with a burn-in of 4, verified: chunk items, speculative starts and
    verification walks all run under the cap.  3 pi rad/s: the robot lags its targets throughout, so no speculative chunk start is
    adopted; 100 rad/s: the cap binds in the first frames only."""
    from gmr_amd import GeneralMotionRetargeting as GMR
    g = GMR("smplx", "unitree_g1", use_velocity_limit=limits is None, velocity_limits=limits)
    cm = g._cm
    pos, quat, names, offs = synth.synth_clips_torch(cm, [96], 6, "cpu", hard=True, yaw0=np.pi)
    pos, quat = pos.numpy(), quat.numpy()
    sc = cm.slot_columns(names)
    orc = Oracle(cm.blob)
    ref = retarget_clips(cm, pos, quat, sc, offs, cap=cm.step_cap, orc=orc)
    _check_preconditions(ref, retarget_clips(cm, pos, quat, sc, offs, cap=None, orc=orc), offs)
    q_seq, it_seq = g.retarget_batch(pos, quat, names, seq_offsets=offs, return_iters=True)
    q_chk, it_chk = g.retarget_batch(pos, quat, names, seq_offsets=offs, chunk=16, burn_in=4, verify=True, return_iters=True)
    print(f"limits {limits}: chunk info {g.last_chunk_info}, max |chunked - sequential| = {np.abs(q_chk - q_seq).max():.3e}")
    assert np.array_equal(it_seq, ref.solves) and _qpos_diff(q_seq, ref.qpos) < 1e-6
    assert np.array_equal(it_chk, it_seq)
    assert np.abs(q_chk - q_seq).max() < 1e-6  # chunk boundaries are adopted at 1e-7 (Engine.ik_solve_chunked); as test_gpu_configs.py
    _assert_step_bound(cm, q_chk, it_chk, offs)


@pytest.mark.parametrize("persistent_ms", [0, 200])
def test_live_session_equals_the_batch(persistent_ms, dev):
    """retarget(frame) frame by frame == retarget_batch of the same frames, through one launch per frame and through the resident
    wavefront (gmr_session_set_persistent).  As in the uncapped session tests a launch per frame re-reads its state and may differ in
    the last bit; solve counts are equal."""
    from gmr_amd import GeneralMotionRetargeting as GMR
    cm, pos, quat, names, sc, offs, ref, un = _case("unitree_g1", np.float64, 1)
    g = GMR("smplx", "unitree_g1", use_velocity_limit=True, persistent_session_ms=persistent_ms)
    assert g.use_velocity_limit and g.velocity_limits == cm.velocity_limits
    T = int(offs[1])
    q_batch, it_batch = g.retarget_batch(pos[:T], quat[:T], names, offset_to_ground=True, return_iters=True)
    assert np.array_equal(it_batch, ref.solves[:T]) and _qpos_diff(q_batch, ref.qpos[:T]) < 1e-6
    for f in range(T):
        q = g.retarget({n: (pos[f, i], quat[f, i]) for i, n in enumerate(names)}, offset_to_ground=True)
        assert np.abs(q - q_batch[f]).max() < 1e-9 and g.last_num_solves == it_batch[f], f
    assert np.abs(q - un.qpos[T - 1]).max() > 1e-3  # not the uncapped answer
    # a session keeps the cap it was created under; a second object without the switch is uncapped
    g0 = GMR("smplx", "unitree_g1", persistent_session_ms=persistent_ms)
    q0 = g0.retarget({n: (pos[0, i], quat[0, i]) for i, n in enumerate(names)}, offset_to_ground=True)
    assert np.abs(q0 - un.qpos[0]).max() < 1e-6
    g.setup_retarget_configuration()   # closes the sessions (parks a resident wavefront)
    g0.setup_retarget_configuration()


def test_session_copies_the_cap_at_create(dev):
    cm, pos, quat, names, sc, offs, ref, un = _case("unitree_g1", np.float64, 0)
    eng = Engine(cm, 0)
    s = eng.session(sc, pos.shape[1], IKParams(), dtype=np.float64)
    eng.set_step_cap(None)  # no launch in flight; the session is unaffected
    for f in range(2):
        q, n = s.step(pos[f], quat[f])
        assert np.abs(q - ref.qpos[f]).max() < 1e-6 and (n & 0x3FFFFFFF) == ref.solves[f]
    s2 = eng.session(sc, pos.shape[1], IKParams(), dtype=np.float64)
    q, n = s2.step(pos[0], quat[0])
    assert np.abs(q - un.qpos[0]).max() < 1e-6 and (n & 0x3FFFFFFF) == un.solves[0]
    s.close(); s2.close(); eng.close()


@pytest.mark.parametrize("robot", ["unitree_g1", "galaxea_r1pro"])
def test_invalid_caps_are_refused_and_the_cap_reads_back(robot, dev):
    cm = compiled("smplx", robot)
    eng = Engine(cm, 0)
    nv = cm.robot.nv
    assert np.isinf(eng.step_cap).all()  # the state after create
    good = np.full(nv, np.inf)
    good[6:] = np.linspace(0.01, 0.5, nv - 6)
    eng.set_step_cap(good)
    assert np.array_equal(eng.step_cap, good)
    for bad_value in (np.nan, 0.0, -0.1, -np.inf):
        bad = good.copy()
        bad[nv - 1] = bad_value
        with pytest.raises(EngineError):
            eng.set_step_cap(bad)
    for root_dof in range(6):  # a planar base's x, y, yaw and its three null dofs too
        bad = good.copy()
        bad[root_dof] = 0.1
        with pytest.raises(EngineError):
            eng.set_step_cap(bad)
    with pytest.raises(ValueError):
        eng.set_step_cap(good[:-1])
    assert np.array_equal(eng.step_cap, good)  # a refused call changes nothing
    eng.set_step_cap(None)
    assert np.isinf(eng.step_cap).all()
    eng.close()

"""The tracking export (gmr_motion_track / gmr_group_motion_track) on the GPU, against the contract in include/gmr_amd.h:
the resampled float64 arrays against a numpy restatement of the definition and scipy's Slerp, the float32 world body poses bit
for bit against Engine.fk on the call's own resampled outputs, the velocities against numpy restatements built from the call's
own outputs, the group and multi-robot forms, the refusals, and the two flags of the dataset scripts end to end.

The ragged set asks for clips of 0, 1, 2, 3, 61, 62, 63, 64, 65, 124 and 125 output frames (the edges of the 62-frame tile, the
one- and two-frame stencils) and four 5-frame clips in a row; the source length of each is found with track_plan.  At 30 -> 50
(ratio 0.6) a clip of T frames yields floor((T-1) / 0.6 + 1e-6) + 1 frames, which never is 3, 5, 63, 65 or 125: there the
clip takes the next length that exists (4, 6, 64, 66, 126).  At 30 -> 30 and 120 -> 50 every length is met exactly.  The clips
are concatenated, so the tile edges fall inside clips and between them either way."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gmr_amd import synth  # noqa: E402
from gmr_amd.schedule import track_plan  # noqa: E402
from tests.util import compiled  # noqa: E402

WANTED = [0, 1, 2, 3, 61, 62, 63, 64, 65, 124, 125, 5, 5, 5, 5]
RATES = [(30.0, 30.0), (30.0, 50.0), (120.0, 50.0)]
ROBOTS = ["unitree_g1", "stanford_toddy"]
F64 = ("root_pos", "root_rot", "joint_pos", "root_lin_vel", "root_ang_vel", "joint_vel")
F32 = ("body_pos_w", "body_quat_w", "body_lin_vel_w", "body_ang_vel_w")
_GMR, _CASES = {}, {}


def _gmr(robot):
    from gmr_amd import GeneralMotionRetargeting
    if robot not in _GMR:
        _GMR[robot] = GeneralMotionRetargeting("smplx", robot, device=0)
    return _GMR[robot]


def _ragged(fps_in, fps_out, wanted=WANTED):
    """Source offsets of clips whose planned output lengths are `wanted` (each the smallest existing length >= the wanted one)."""
    lens = []
    for m in wanted:
        T = 0
        while m > 0 and int(track_plan([0, T], fps_in, fps_out)[0][-1]) < m:
            T += 1
        lens.append(T)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _smooth_qpos(robot, offs, seed):
    """Per clip a random walk (steps <= 0.05 rad, <= 0.02 m, quaternion components <= 0.02 then renormalised) from a random start:
    hinges within the joint ranges, unit root quaternions (wxyz), root positions around a standing height."""
    cm = compiled("smplx", robot)
    r = cm.robot
    rng = np.random.default_rng(seed)
    hb = sorted(r.hinge_bodies(), key=lambda b: r.qpos_adr[b])
    lim = np.array(r.jnt_range, dtype=np.float64)[hb]
    lo = np.where(lim[:, 0] < lim[:, 1], lim[:, 0], -1.0)
    hi = np.where(lim[:, 0] < lim[:, 1], lim[:, 1], 1.0)
    q = np.empty((int(offs[-1]), r.nq))
    for s in range(len(offs) - 1):
        a, b = int(offs[s]), int(offs[s + 1])
        T = b - a
        if T == 0:
            continue
        pos = rng.normal(size=3) * [2.0, 2.0, 0.2] + [0.0, 0.0, 0.8] + np.cumsum(rng.uniform(-0.02, 0.02, size=(T, 3)), axis=0)
        w = rng.normal(size=4)
        w = w / np.linalg.norm(w) + np.cumsum(rng.uniform(-0.02, 0.02, size=(T, 4)), axis=0)
        dof = rng.uniform(lo, hi) + np.cumsum(rng.uniform(-0.05, 0.05, size=(T, len(hb))), axis=0)
        q[a:b, :3] = pos
        q[a:b, 3:7] = w / np.linalg.norm(w, axis=1, keepdims=True)
        q[a:b, 7:] = np.clip(dof, lo, hi)
    return q


def _case(robot, rates):
    """One call per (robot, rates), shared by the tests below: (qpos, source offsets, MotionTrack as host arrays, device result)."""
    key = (robot, rates)
    if key not in _CASES:
        offs = _ragged(*rates)
        q = _smooth_qpos(robot, offs, seed=ROBOTS.index(robot) * 10 + RATES.index(rates) if robot in ROBOTS else 99)
        tr = _gmr(robot)._engine.motion_track(torch.from_numpy(q).cuda(), offs, rates[0], rates[1])
        _CASES[key] = (q, offs, {k: v.cpu().numpy() for k, v in tr.items()}, tr)
    return _CASES[key]


# ------------------------------------------------------------------ the definition, restated in float64 numpy
def _plan_ref(offs, out_offs, ratio):
    """Global source rows i0, i1 and the weight a of every output frame."""
    i0s, i1s, As = [], [], []
    for s in range(len(offs) - 1):
        T, M = int(offs[s + 1] - offs[s]), int(out_offs[s + 1] - out_offs[s])
        u = np.arange(M, dtype=np.float64) * ratio[s]
        i0 = np.minimum(np.floor(u).astype(np.int64), T - 1)
        i1 = np.minimum(i0 + 1, T - 1)
        i0s.append(offs[s] + i0)
        i1s.append(offs[s] + i1)
        As.append(np.where(i1 > i0, u - i0, 0.0))
    return np.concatenate(i0s), np.concatenate(i1s), np.concatenate(As)


def _slerp_ref(q0, q1, a):
    d = np.sum(q0 * q1, axis=1)
    q1 = np.where(d[:, None] < 0, -q1, q1)
    d = np.abs(d)
    om = np.arccos(np.minimum(d, 1.0))
    small = om < 1e-8
    so = np.where(small, 1.0, np.sin(om))
    w0 = np.where(small, 1.0 - a, np.sin((1.0 - a) * om) / so)
    w1 = np.where(small, a, np.sin(a * om) / so)
    r = w0[:, None] * q0 + w1[:, None] * q1
    r = r / np.sqrt(np.sum(r * r, axis=1))[:, None]
    return np.where(a[:, None] == 0, q0, r)


def _resample_ref(q, offs, out_offs, ratio):
    i0, i1, a = _plan_ref(offs, out_offs, ratio)
    x0, x1 = q[i0], q[i1]
    lerp = np.where(a[:, None] == 0, x0, x0 + a[:, None] * (x1 - x0))
    rot = _slerp_ref(x0[:, [4, 5, 6, 3]], x1[:, [4, 5, 6, 3]], a)
    return lerp[:, :3], rot, lerp[:, 7:], (i0, i1, a)


def _stencil(out_offs, fps_out):
    """Global rows of k-1 / k+1 clamped to the clip, and h."""
    km, kp = [], []
    for s in range(len(out_offs) - 1):
        a, M = int(out_offs[s]), int(out_offs[s + 1] - out_offs[s])
        k = np.arange(M)
        km.append(a + np.maximum(k - 1, 0))
        kp.append(a + np.minimum(k + 1, M - 1))
    km, kp = np.concatenate(km), np.concatenate(kp)
    return km, kp, (kp - km) * (1.0 / fps_out)


def _lin_vel_ref(x, km, kp, h):
    x = x.astype(np.float64)
    hh = h.reshape((-1,) + (1,) * (x.ndim - 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(hh == 0, 0.0, (x[kp] - x[km]) / hh)


def _ang_vel_ref(qt, km, kp, h):
    """rotvec(q[kp] (x) conj(q[km])) / h for xyzw quaternions [..., 4]."""
    p, q = qt[kp].astype(np.float64), qt[km].astype(np.float64)
    pv, pw, qv, qw = p[..., :3], p[..., 3:], q[..., :3], q[..., 3:]
    w = pw * qw + np.sum(pv * qv, axis=-1, keepdims=True)
    v = qw * pv - pw * qv - np.cross(pv, qv)
    neg = w < 0
    w, v = np.where(neg, -w, w), np.where(neg, -v, v)
    n = np.sqrt(np.sum(v * v, axis=-1, keepdims=True))
    with np.errstate(divide="ignore", invalid="ignore"):
        rv = np.where(n > 1e-12, v * (2.0 * np.arctan2(n, w) / n), 2.0 * v)
        hh = h.reshape((-1,) + (1,) * (rv.ndim - 1))
        return np.where(hh == 0, 0.0, rv / hh)


def _report(tag, worst):
    print(f"[motion_track] {tag}: " + ", ".join(f"{k}={v:.3e}" for k, v in worst.items()))


# ------------------------------------------------------------------ checks 1 - 5
@pytest.mark.parametrize("robot", ROBOTS)
def test_equal_rates_copy_the_qpos_columns(robot):
    q, offs, got, tr = _case(robot, RATES[0])
    assert np.array_equal(tr.out_offsets, offs)
    assert np.array_equal(got["root_pos"], q[:, :3]) and np.array_equal(got["root_rot"], q[:, [4, 5, 6, 3]])
    assert np.array_equal(got["joint_pos"], q[:, 7:])
    assert all(got[k].dtype == np.float64 for k in F64) and all(got[k].dtype == np.float32 for k in F32)


@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("robot", ROBOTS)
def test_resampled_arrays_match_the_definition_and_scipy(robot, rates):
    from scipy.spatial.transform import Rotation as R, Slerp
    q, offs, got, tr = _case(robot, rates)
    out_offs, ratio = track_plan(offs, *rates)
    assert np.array_equal(tr.out_offsets, out_offs) and got["root_pos"].shape == (int(out_offs[-1]), 3)
    if rates != RATES[1]:
        assert np.diff(out_offs).tolist() == WANTED  # the wanted lengths, met exactly
    else:
        assert np.diff(out_offs).tolist() == [0, 1, 2, 4, 61, 62, 64, 64, 66, 124, 126, 6, 6, 6, 6]  # (see the module docstring)
    rp, rr, jp, (i0, i1, a) = _resample_ref(q, offs, out_offs, ratio)
    worst = {"root_pos": np.abs(got["root_pos"] - rp).max(), "root_rot": np.abs(got["root_rot"] - rr).max(),
             "joint_pos": np.abs(got["joint_pos"] - jp).max()}
    # against scipy, by geodesic angle
    ang = 0.0
    for s in range(len(offs) - 1):
        T, (oa, ob) = int(offs[s + 1] - offs[s]), (int(out_offs[s]), int(out_offs[s + 1]))
        if ob == oa:
            continue
        mine = R.from_quat(got["root_rot"][oa:ob])
        src = q[offs[s]:offs[s + 1]][:, [4, 5, 6, 3]]
        if T == 1:
            want = R.from_quat(src[[0] * (ob - oa)])
        else:
            want = Slerp(np.arange(T, dtype=np.float64), R.from_quat(src))(np.minimum(np.arange(ob - oa) * ratio[s], T - 1.0))
        ang = max(ang, float((mine * want.inv()).magnitude().max()))
    worst["slerp_vs_scipy_rad"] = ang
    _report(f"{robot} {rates[0]:g}->{rates[1]:g} resample", worst)
    assert worst["root_pos"] <= 1e-12 and worst["root_rot"] <= 1e-12 and worst["joint_pos"] <= 1e-12
    assert ang <= 1e-12
    # the indices and the weight agree exactly: a lerp without contraction is then the same float64 operation on both sides
    assert np.array_equal(got["root_pos"], rp) and np.array_equal(got["joint_pos"], jp)
    assert np.array_equal(got["root_rot"][a == 0], q[i0[a == 0]][:, [4, 5, 6, 3]])


@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("robot", ROBOTS)
def test_world_body_poses_are_engine_fk_of_the_resampled_outputs(robot, rates):
    q, offs, got, tr = _case(robot, rates)
    bp, br = _gmr(robot)._engine.fk(tr["root_pos"].to(torch.float32), tr["root_rot"].to(torch.float32), tr["joint_pos"].to(torch.float32),
                                    want_rot=True)
    assert np.array_equal(got["body_pos_w"], bp.cpu().numpy()) and np.array_equal(got["body_quat_w"], br.cpu().numpy())


@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("robot", ROBOTS)
def test_velocities_match_the_definition_on_the_calls_own_outputs(robot, rates):
    q, offs, got, tr = _case(robot, rates)
    fps_out = rates[1]
    out_offs = tr.out_offsets
    km, kp, h = _stencil(out_offs, fps_out)
    M = np.diff(out_offs)
    want = {"root_lin_vel": _lin_vel_ref(got["root_pos"], km, kp, h), "joint_vel": _lin_vel_ref(got["joint_pos"], km, kp, h),
            "root_ang_vel": _ang_vel_ref(got["root_rot"], km, kp, h),
            "body_lin_vel_w": _lin_vel_ref(got["body_pos_w"], km, kp, h), "body_ang_vel_w": _ang_vel_ref(got["body_quat_w"], km, kp, h)}
    worst = {}
    for k in ("root_lin_vel", "joint_vel", "root_ang_vel"):
        err = np.abs(got[k] - want[k])
        bound = 1e-12 * np.abs(want[k]) + 1e-12 * fps_out
        worst[k] = float((err / bound).max())  # in units of the bound
        worst[k + "_abs"] = float(err.max())
    for k in ("body_lin_vel_w", "body_ang_vel_w"):
        w32 = want[k].astype(np.float32)
        err = np.abs(got[k].astype(np.float64) - want[k])
        bound = 2.0 * np.spacing(np.abs(w32)).astype(np.float64) + 1e-6 * fps_out
        worst[k] = float((err / bound).max())
        worst[k + "_ulp"] = float((np.abs(got[k].astype(np.float64) - w32.astype(np.float64)) / np.spacing(np.abs(w32))).max())
    _report(f"{robot} {rates[0]:g}->{rates[1]:g} velocities (fraction of the bound)", worst)
    for k in ("root_lin_vel", "joint_vel", "root_ang_vel", "body_lin_vel_w", "body_ang_vel_w"):
        assert worst[k] <= 1.0, (k, worst)
    # a clip of one output frame: zeros everywhere
    for s in np.nonzero(M == 1)[0]:
        for k in want:
            assert not got[k][out_offs[s]].any(), (k, s)
    # one-sided differences at both ends of every longer clip, from rows of the clip itself (the four 5-frame clips sit in a
    # row: a difference that reached across a boundary would pick up the jump to the next clip's independent start)
    dt = 1.0 / fps_out
    for s in np.nonzero(M >= 2)[0]:
        a, b = int(out_offs[s]), int(out_offs[s + 1])
        for k, src in (("root_lin_vel", "root_pos"), ("joint_vel", "joint_pos")):
            assert np.allclose(got[k][a], (got[src][a + 1] - got[src][a]) / dt, rtol=1e-12, atol=1e-12 * fps_out)
            assert np.allclose(got[k][b - 1], (got[src][b - 1] - got[src][b - 2]) / dt, rtol=1e-12, atol=1e-12 * fps_out)
    assert M[-4:].tolist() == ([6] * 4 if rates == RATES[1] else [5] * 4)


def test_hands_model_fits_in_lds():
    """52 bodies: the largest tile.  Resampled arrays against the definition, body poses against Engine.fk, once."""
    robot, rates = "unitree_g1_with_hands", RATES[1]
    q, offs, got, tr = _case(robot, rates)
    out_offs, ratio = track_plan(offs, *rates)
    rp, rr, jp, _ = _resample_ref(q, offs, out_offs, ratio)
    assert np.array_equal(got["root_pos"], rp) and np.array_equal(got["joint_pos"], jp) and np.abs(got["root_rot"] - rr).max() <= 1e-12
    bp, br = _gmr(robot)._engine.fk(tr["root_pos"].to(torch.float32), tr["root_rot"].to(torch.float32), tr["joint_pos"].to(torch.float32),
                                    want_rot=True)
    assert got["body_pos_w"].shape[1] == 52
    assert np.array_equal(got["body_pos_w"], bp.cpu().numpy()) and np.array_equal(got["body_quat_w"], br.cpu().numpy())
    km, kp, h = _stencil(out_offs, rates[1])
    want = _ang_vel_ref(got["body_quat_w"], km, kp, h)
    bound = 2.0 * np.spacing(np.abs(want.astype(np.float32))).astype(np.float64) + 1e-6 * rates[1]
    assert (np.abs(got["body_ang_vel_w"] - want) <= bound).all()


# ------------------------------------------------------------------ group and multi-robot forms
def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a)


def test_group_motion_track_equals_the_single_calls():
    from gmr_amd import MultiRobotRetargeting
    robots = ["unitree_g1", "stanford_toddy", "booster_t1"]
    mr = MultiRobotRetargeting("smplx", robots, device=0)
    offs = [_ragged(30.0, 50.0), _ragged(30.0, 50.0, wanted=[7, 0, 130, 1, 62]), np.array([0, 0], dtype=np.int64)]
    fps_in = [30.0, [30.0, 30.0, 60.0, 30.0, 120.0], 30.0]
    qs = [torch.from_numpy(_smooth_qpos(r, o, seed=40 + i)).cuda() for i, (r, o) in enumerate(zip(robots, offs))]
    got = mr.group.motion_track([(q, o, f) for q, o, f in zip(qs, offs, fps_in)], 50.0)
    for i, r in enumerate(robots):
        one = _gmr(r)._engine.motion_track(qs[i], offs[i], fps_in[i], 50.0)
        assert np.array_equal(got[i].out_offsets, one.out_offsets)
        assert _same({k: v.cpu().numpy() for k, v in got[i].items()}, {k: v.cpu().numpy() for k, v in one.items()}), r
    assert got[2]["root_pos"].shape == (0, 3)  # the member without frames did no work
    none = mr.group.motion_track([None, (qs[1], offs[1], fps_in[1]), None], 50.0)
    assert none[0] is None and none[2] is None
    assert _same({k: v.cpu().numpy() for k, v in none[1].items()}, {k: v.cpu().numpy() for k, v in got[1].items()})
    mr.close()


def test_multi_robot_tracking_from_qpos_equals_the_dataset_call():
    from gmr_amd import MultiRobotRetargeting, dataset
    robots = ["unitree_g1", "stanford_toddy"]
    mr = MultiRobotRetargeting("smplx", robots, device=0)
    offs = _ragged(30.0, 50.0, wanted=[0, 1, 63, 5, 5, 70])
    fps = [30.0, 30.0, 30.0, 60.0, 30.0, 120.0]
    qpos = {r: torch.from_numpy(_smooth_qpos(r, offs, seed=60 + i)).cuda() for i, r in enumerate(robots)}
    got = mr.tracking_from_qpos(qpos, offs, fps, 50.0)
    assert list(got) == robots
    out_offs = track_plan(offs, fps, 50.0)[0]
    for r in robots:
        ref = dataset.tracking_from_qpos(_gmr(r), qpos[r], offs, fps, 50.0)
        assert len(got[r]) == len(ref) == len(offs) - 1
        for s, (m, w) in enumerate(zip(got[r], ref)):
            assert m.keys() == w.keys() and set(dataset.TRACK_ARRAYS) < set(m)
            assert m["fps"] == w["fps"] == 50.0 and m["quat_order"] == "xyzw"
            assert m["body_names"] == w["body_names"] == list(_gmr(r).model.body_names)
            assert m["joint_names"] == w["joint_names"] and len(m["joint_names"]) == m["joint_pos"].shape[1]
            for k in dataset.TRACK_ARRAYS:
                assert np.array_equal(m[k], w[k]) and m[k].dtype == w[k].dtype and m[k].shape[0] == out_offs[s + 1] - out_offs[s], (r, s, k)
    mr.close()


# ------------------------------------------------------------------ refusals
def test_track_refusals():
    import ctypes as C
    from gmr_amd import GeneralMotionRetargeting, MultiRobotRetargeting, _native, dataset
    from gmr_amd.engine import EngineError
    offs = np.array([0, 10], dtype=np.int64)
    # a planar base: the library's unsupported error from the engine, NotImplementedError from the dataset layer
    planar = GeneralMotionRetargeting("smplx", "galaxea_r1pro", device=0)
    eng = planar._engine
    qp = torch.zeros((10, eng.nq), dtype=torch.float64, device="cuda")
    qp[:, 3] = 1.0
    with pytest.raises(EngineError, match="not supported"):
        eng.motion_track(qp, offs, 30.0, 50.0)
    with pytest.raises(NotImplementedError):
        dataset.tracking_from_qpos(planar, qp, offs, 30.0, 50.0)
    mr = MultiRobotRetargeting("smplx", ["unitree_g1", "galaxea_r1pro"], device=0)
    with pytest.raises(NotImplementedError):
        mr.tracking_from_qpos({"unitree_g1": torch.zeros((10, mr.engines[0].nq), dtype=torch.float64, device="cuda"), "galaxea_r1pro": qp},
                              offs, 30.0, 50.0)
    mr.close()
    # rates that are not positive: the invalid-argument error, from the engine and from the library itself
    q, offs, got, tr = _case("unitree_g1", RATES[1])
    eng = _gmr("unitree_g1")._engine
    qd = torch.from_numpy(q).cuda()
    for fin, fout in ((30.0, 0.0), (30.0, -50.0), (0.0, 50.0)):
        with pytest.raises(EngineError, match="invalid argument"):
            eng.motion_track(qd, offs, fin, fout)
    out_offs, ratio = track_plan(offs, 30.0, 50.0)
    ti = _native.TrackInput()
    ti.qpos, ti.n_frames, ti.n_seq = qd.data_ptr(), int(offs[-1]), len(offs) - 1
    ti.seq_offsets, ti.out_offsets, ti.ratio = offs.ctypes.data, out_offs.ctypes.data, ratio.ctypes.data
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for fps_out, rat in ((0.0, ratio), (-1.0, ratio), (50.0, np.where(np.arange(len(ratio)) == 2, 0.0, ratio))):
        rat = np.ascontiguousarray(rat)
        ti.fps_out, ti.ratio = fps_out, rat.ctypes.data
        assert eng._lib.gmr_motion_track(eng._h, C.byref(ti), stream) == -1
    bad = out_offs.copy()
    bad[1] = 3  # output frames for the clip without source frames
    ti.fps_out, ti.ratio, ti.out_offsets = 50.0, ratio.ctypes.data, bad.ctypes.data
    assert eng._lib.gmr_motion_track(eng._h, C.byref(ti), stream) == -1
    # argument checks of the wrapper
    with pytest.raises(EngineError):
        eng.motion_track(qd.to(torch.float32), offs, 30.0, 50.0)
    with pytest.raises(ValueError):
        eng.motion_track(qd, offs[:-1], 30.0, 50.0)
    # without the bodies: no body tensors, the rest bit for bit
    lean = eng.motion_track(qd, offs, 30.0, 50.0, bodies=False)
    assert set(lean) == set(F64)
    for k in F64:
        assert np.array_equal(lean[k].cpu().numpy(), got[k]), k
    # caller-owned outputs, a subset: only those are written, with the same values
    mine = {"joint_vel": torch.zeros_like(tr["joint_vel"]), "body_quat_w": torch.zeros_like(tr["body_quat_w"])}
    res = eng.motion_track(qd, offs, 30.0, 50.0, out=mine)
    assert set(res) == set(mine) and res["joint_vel"] is mine["joint_vel"]
    assert np.array_equal(mine["joint_vel"].cpu().numpy(), got["joint_vel"]) and np.array_equal(mine["body_quat_w"].cpu().numpy(), got["body_quat_w"])


# ------------------------------------------------------------------ the dataset scripts
def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_dataset_script_track_flags_end_to_end(tmp_path):
    from gmr_amd import dataset
    from gmr_amd.scripts import smplx_to_robot_dataset
    from gmr_amd.smplx_adapter import iter_joint_batches
    dev = torch.device("cuda", 0)
    g1 = compiled("smplx", "unitree_g1")
    pos, quat, names, offs = synth.synth_clips_torch(g1, np.array([60, 45, 70]), seed=9, device=dev, yaw0=0.5, dtype=torch.float64)
    src = str(tmp_path / "in")
    os.makedirs(src)
    synth.write_smplx_joint_files(src, pos, quat, names, offs, fps=30.0, heights=[1.7, 1.6, 1.8])
    plain, with_trk, trk = str(tmp_path / "plain"), str(tmp_path / "with"), str(tmp_path / "trk")
    base = ["--src_folder", src, "--robot", "unitree_g1", "--num_cpus", "2", "--hard_motions"]
    assert smplx_to_robot_dataset.main(base + ["--tgt_folder", plain]) == 0
    assert smplx_to_robot_dataset.main(base + ["--tgt_folder", with_trk, "--track_fps", "50", "--track_folder", trk]) == 0
    # the pickles are those of a run without the flags
    assert _tree(plain) == _tree(with_trk) and len(_tree(plain)) == 3
    for f in _tree(plain):
        assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(with_trk, f), "rb").read(), f
    assert _tree(trk) == [f.replace(".pkl", ".npz") for f in _tree(plain)]
    # the .npz files are tracking_from_qpos of the same solved qpos
    g = _gmr("unitree_g1")
    files = sorted(os.path.join(src, f) for f in os.listdir(src))
    (batch,) = list(iter_joint_batches(files, batch_files=1024, device=0, threads=2, columns=g.ik_columns, skip_errors=True))
    qpos = g.retarget_batch(batch.pos, batch.quat, batch.body_names, seq_offsets=batch.seq_offsets, human_heights=batch.human_heights)
    want = dataset.tracking_from_qpos(g, qpos, batch.seq_offsets, batch.fps, 50.0)
    by_name = {os.path.splitext(os.path.basename(f))[0]: w for f, w in zip(batch.files, want)}
    for f in _tree(trk):
        got, w = dataset.load_tracking(os.path.join(trk, f)), by_name[os.path.splitext(os.path.basename(f))[0]]
        assert set(got) == set(w) and got["fps"] == 50.0 and got["body_names"] == w["body_names"] and got["joint_names"] == w["joint_names"]
        for k in dataset.TRACK_ARRAYS:
            assert np.array_equal(got[k], w[k]) and got[k].dtype == w[k].dtype, (f, k)
    # the multi-robot form puts each robot's files below its own folder
    mt, mtrk = str(tmp_path / "multi"), str(tmp_path / "multi_trk")
    assert smplx_to_robot_dataset.main(["--src_folder", src, "--robots", "unitree_g1,booster_t1", "--num_cpus", "2", "--hard_motions",
                                        "--tgt_folder", mt, "--track_fps", "50", "--track_folder", mtrk]) == 0
    assert _tree(mtrk) == [f.replace(".pkl", ".npz") for f in _tree(mt)] and len(_tree(mtrk)) == 6
    for f in _tree(trk):
        a, b = dataset.load_tracking(os.path.join(trk, f)), dataset.load_tracking(os.path.join(mtrk, "unitree_g1", f))
        assert all(np.array_equal(a[k], b[k]) for k in dataset.TRACK_ARRAYS), f

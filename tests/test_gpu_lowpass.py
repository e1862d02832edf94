"""The zero-phase Butterworth low-pass of the tracking export (``gmr_track_input.lowpass_hz``, the contract in include/gmr_amd.h)
on the GPU, against its numpy restatement (tests/lowpass_reference.py) fed with the library's own coefficients and against
scipy.signal.filtfilt.

The clips cover the lengths at which the kernel takes another path: none, one frame (a copy), fewer frames than the padding
(e = T - 1), the padding itself and one beside it (9, 10, 11), the row-prefetch depth 16 and its neighbours, two batches and one
row, and 300 frames; they alternate between 30 and 120 fps.

Measured on one MI355X (ROCm 7), both robots, both cutoffs: quaternion components against the restatement 0 (bit for bit),
everything against scipy at most 2.04e-14 (G1 with hands, 3 Hz)."""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
signal = pytest.importorskip("scipy.signal")
pytestmark = pytest.mark.gpu

from gmr_amd import synth  # noqa: E402
from gmr_amd.schedule import track_plan  # noqa: E402
from tests import lowpass_reference as ref  # noqa: E402
from tests.util import compiled  # noqa: E402

ROBOTS = ["unitree_g1", "unitree_g1_with_hands"]
LENGTHS = [0, 1, 2, 3, 9, 10, 11, 15, 16, 17, 33, 64, 65, 300]
OFFS = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
FPS = np.array([30.0, 120.0] * (len(LENGTHS) // 2))
CUTOFFS = [6.0, 3.0]
FPS_OUT = 50.0
QUAT_BOUND = 4.5e-16   # two ulps of a component of a unit quaternion; 0 is expected
SCIPY_BOUND = 1e-11
_GMR, _QPOS, _REF = {}, {}, {}


def _gmr(robot):
    from gmr_amd import GeneralMotionRetargeting
    if robot not in _GMR:
        _GMR[robot] = GeneralMotionRetargeting("smplx", robot, device=0)
    return _GMR[robot]


def _noisy_qpos(robot, offs=OFFS, seed=0):
    """tests/test_gpu_motion_track.py::_smooth_qpos (per clip a random walk from a random start: steps <= 0.05 rad, <= 0.02 m,
    quaternion components <= 0.02) plus 0.01 of white noise; the root quaternion renormalised, a third of its rows negated."""
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
    q += 0.01 * rng.normal(size=q.shape)
    q[:, 3:7] /= np.linalg.norm(q[:, 3:7], axis=1, keepdims=True)
    neg = rng.random(q.shape[0]) < 1.0 / 3.0
    q[neg, 3:7] = -q[neg, 3:7]
    return q


def _qpos(robot):
    if robot not in _QPOS:
        q = _noisy_qpos(robot, seed=ROBOTS.index(robot))
        _QPOS[robot] = (q, torch.from_numpy(q).cuda())
    return _QPOS[robot]


def _restated(robot, fc):
    """The restatement with the library's coefficients, fs = ratio * fps_out per clip: computed once, never changed."""
    if (robot, fc) not in _REF:
        fs = track_plan(OFFS, FPS, FPS_OUT)[1] * FPS_OUT
        assert np.array_equal(fs, FPS)  # (so smooth_qpos, which runs at fps_out = fps, uses the same coefficients)
        out = ref.filter_qpos(_qpos(robot)[0], OFFS, fs, fc)
        out.setflags(write=False)
        _REF[(robot, fc)] = out
    return _REF[(robot, fc)]


def _host(tr):
    return {k: v.cpu().numpy() for k, v in tr.items()}


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k], equal_nan=True) and a[k].dtype == b[k].dtype for k in a)


def _scipy_qpos(q, fc):
    out = np.empty_like(q)
    for s, T in enumerate(LENGTHS):
        a, b = int(OFFS[s]), int(OFFS[s + 1])
        x = q[a:b].copy()
        x[:, 3:7] = ref.sign_continuous(x[:, 3:7])
        if T >= 2:
            bb, aa = signal.butter(2, 2 * fc / FPS[s])
            x = signal.filtfilt(bb, aa, x, axis=0, padlen=min(9, T - 1))
        x[:, 3:7] /= np.linalg.norm(x[:, 3:7], axis=1, keepdims=True)
        out[a:b] = x
    return out


# ------------------------------------------------------------------ 1: the filtered qpos
@pytest.mark.parametrize("fc", CUTOFFS)
@pytest.mark.parametrize("robot", ROBOTS)
def test_smooth_qpos_matches_the_restatement_and_scipy(robot, fc):
    from gmr_amd import dataset
    q, qd = _qpos(robot)
    got = dataset.smooth_qpos(_gmr(robot), qd, OFFS, FPS, fc)
    assert got.shape == qd.shape and got.dtype == torch.float64 and got.device == qd.device
    got = got.cpu().numpy()
    want = _restated(robot, fc)
    rest = [c for c in range(q.shape[1]) if c < 3 or c >= 7]
    quat_err = np.abs(got[:, 3:7] - want[:, 3:7]).max()
    scipy_err = np.abs(got - _scipy_qpos(q, fc)).max()
    print(f"{robot} fc {fc}: quaternion vs restatement {quat_err:.3g}, everything vs scipy {scipy_err:.3g}")
    assert np.array_equal(got[:, rest], want[:, rest])
    assert quat_err <= QUAT_BOUND
    assert scipy_err <= SCIPY_BOUND
    assert np.abs(np.linalg.norm(got[:, 3:7], axis=1) - 1.0).max() <= 4.5e-16
    for s in range(len(LENGTHS)):  # sign-continuous within every clip
        qq = got[OFFS[s]:OFFS[s + 1], 3:7]
        assert np.all(np.sum(qq[:-1] * qq[1:], axis=1) > 0)
    # off: a copy
    assert torch.equal(dataset.smooth_qpos(_gmr(robot), qd, OFFS, FPS, None), qd)


# ------------------------------------------------------------------ 2, 3: the export
@pytest.mark.parametrize("fc", CUTOFFS)
@pytest.mark.parametrize("robot", ROBOTS)
def test_filtered_export_equals_the_export_of_the_filtered_qpos(robot, fc):
    eng = _gmr(robot)._engine
    q, qd = _qpos(robot)
    got = eng.motion_track(qd, OFFS, FPS, FPS_OUT, lowpass_hz=fc)
    want = eng.motion_track(torch.from_numpy(np.array(_restated(robot, fc))).cuda(), OFFS, FPS, FPS_OUT, lowpass_hz=0.0)
    assert np.array_equal(got.out_offsets, want.out_offsets) and len(got) == 10
    got, want = _host(got), _host(want)
    for k in got:
        assert np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype, k
    plain = _host(eng.motion_track(qd, OFFS, FPS, FPS_OUT))
    assert not np.array_equal(plain["joint_vel"], got["joint_vel"])  # (the filter did something)


@pytest.mark.parametrize("robot", ROBOTS)
def test_cutoff_zero_is_the_call_without_it(robot):
    eng = _gmr(robot)._engine
    _, qd = _qpos(robot)
    plain = _host(eng.motion_track(qd, OFFS, FPS, FPS_OUT))
    assert _same(_host(eng.motion_track(qd, OFFS, FPS, FPS_OUT, lowpass_hz=0.0)), plain)
    assert _same(_host(eng.motion_track(qd, OFFS, FPS, FPS_OUT, lowpass_hz=-0.0)), plain)


# ------------------------------------------------------------------ 4: non-finite input
def test_a_nan_spoils_its_column_of_its_clip_and_nothing_else():
    from gmr_amd import dataset
    robot, fc = "unitree_g1", 6.0
    g = _gmr(robot)
    q, qd = _qpos(robot)
    clean = dataset.smooth_qpos(g, qd, OFFS, FPS, fc).cpu().numpy()
    sa, sb = LENGTHS.index(33), LENGTHS.index(300)   # a hinge of one clip, a quaternion component of another
    bad = q.copy()
    bad[OFFS[sa] + 20, 7 + 11] = np.nan
    bad[OFFS[sb] + 150, 5] = np.nan
    got = dataset.smooth_qpos(g, torch.from_numpy(bad).cuda(), OFFS, FPS, fc).cpu().numpy()
    spoiled = np.zeros(q.shape, dtype=bool)
    spoiled[OFFS[sa]:OFFS[sa + 1], 7 + 11] = True
    spoiled[OFFS[sb]:OFFS[sb + 1], 3:7] = True
    assert np.array_equal(~np.isfinite(got), spoiled)
    assert np.array_equal(got[~spoiled], clean[~spoiled])
    # ... and the export of it: the other clips' outputs are those of the clean run
    eng = g._engine
    a = eng.motion_track(torch.from_numpy(bad).cuda(), OFFS, FPS, FPS_OUT, lowpass_hz=fc)
    b = _host(eng.motion_track(qd, OFFS, FPS, FPS_OUT, lowpass_hz=fc))
    oo = a.out_offsets
    a = _host(a)
    keep = np.ones(int(oo[-1]), dtype=bool)
    for s in (sa, sb):
        keep[oo[s]:oo[s + 1]] = False
    for k in a:
        assert np.array_equal(a[k][keep], b[k][keep]), k
    assert not np.isfinite(a["joint_pos"][oo[sa]:oo[sa + 1], 11]).any() and np.isfinite(np.delete(a["joint_pos"], 11, axis=1)).all()
    assert not np.isfinite(a["root_rot"][oo[sb]:oo[sb + 1]]).any() and np.isfinite(a["root_pos"]).all()


# ------------------------------------------------------------------ 5: group and multi-robot forms
def test_group_and_multi_robot_forms_equal_the_single_calls():
    from gmr_amd import MultiRobotRetargeting, dataset
    mr = MultiRobotRetargeting("smplx", ROBOTS, device=0)
    qd = [_qpos(r)[1] for r in ROBOTS]
    got = mr.group.motion_track([(q, OFFS, FPS) for q in qd], FPS_OUT, lowpass_hz=CUTOFFS)
    for i, r in enumerate(ROBOTS):
        one = _gmr(r)._engine.motion_track(qd[i], OFFS, FPS, FPS_OUT, lowpass_hz=CUTOFFS[i])
        assert np.array_equal(got[i].out_offsets, one.out_offsets)
        assert _same(_host(got[i]), _host(one)), r
    # one filtered member beside one that is not, and one value for all
    mixed = mr.group.motion_track([(q, OFFS, FPS) for q in qd], FPS_OUT, lowpass_hz=[0.0, 3.0])
    assert _same(_host(mixed[0]), _host(_gmr(ROBOTS[0])._engine.motion_track(qd[0], OFFS, FPS, FPS_OUT)))
    assert _same(_host(mixed[1]), _host(got[1]))
    both = mr.group.motion_track([(q, OFFS, FPS) for q in qd], FPS_OUT, lowpass_hz=6.0)
    assert _same(_host(both[0]), _host(got[0]))
    tracks = mr.tracking_from_qpos(dict(zip(ROBOTS, qd)), OFFS, FPS, FPS_OUT, lowpass_hz=6.0)
    for i, r in enumerate(ROBOTS):
        want = dataset.tracking_from_qpos(_gmr(r), qd[i], OFFS, FPS, FPS_OUT, lowpass_hz=6.0)
        assert len(tracks[r]) == len(want) == len(LENGTHS)
        for m, w in zip(tracks[r], want):
            for k in dataset.TRACK_ARRAYS:
                assert np.array_equal(m[k], w[k]) and m[k].dtype == w[k].dtype, (r, k)
        oo = both[i].out_offsets
        assert np.array_equal(np.concatenate([m["joint_vel"] for m in want]), _host(both[i])["joint_vel"]) and oo[-1] > 0
    mr.close()


# ------------------------------------------------------------------ 6: refusals
def test_lowpass_refusals():
    from gmr_amd import MultiRobotRetargeting, _native, dataset
    from gmr_amd.engine import EngineError
    g = _gmr("unitree_g1")
    eng = g._engine
    _, qd = _qpos("unitree_g1")
    for bad in (15.0, -1.0, float("nan")):  # 15 Hz: Nyquist of the 30 fps clips
        with pytest.raises((EngineError, ValueError)):
            eng.motion_track(qd, OFFS, FPS, FPS_OUT, lowpass_hz=bad)
        with pytest.raises((EngineError, ValueError)):
            dataset.smooth_qpos(g, qd, OFFS, FPS, bad)
    with pytest.raises((EngineError, ValueError), match="clip 2"):  # clip 0 is at 30 fps too, but has no frames
        eng.motion_track(qd, OFFS, FPS, FPS_OUT, lowpass_hz=15.0)
    out_offs, ratio = track_plan(OFFS, FPS, FPS_OUT)
    ti = _native.TrackInput()
    ti.qpos, ti.n_frames, ti.n_seq = qd.data_ptr(), int(OFFS[-1]), len(OFFS) - 1
    ti.seq_offsets, ti.out_offsets, ti.ratio, ti.fps_out = OFFS.ctypes.data, out_offs.ctypes.data, ratio.ctypes.data, FPS_OUT
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = eng._lib
    for bad, word in ((15.0, "clip 2"), (20.0, "clip 2"), (-1.0, "lowpass_hz"), (float("nan"), "lowpass_hz"), (float("inf"), "lowpass_hz")):
        ti.lowpass_hz = bad
        assert lib.gmr_motion_track(eng._h, C.byref(ti), stream) == -1
        assert word in lib.gmr_last_error(eng._h).decode(), (bad, lib.gmr_last_error(eng._h))
    # in a group the message names the member as well
    mr = MultiRobotRetargeting("smplx", ROBOTS, device=0)
    inputs = (_native.TrackInput * 2)()
    inputs[1] = ti
    inputs[1].qpos, inputs[1].lowpass_hz = _qpos(ROBOTS[1])[1].data_ptr(), 15.0
    assert lib.gmr_group_motion_track(mr.group._g, inputs, stream) == -1
    msg = lib.gmr_group_last_error(mr.group._g).decode()
    assert "member 1" in msg and "clip 2" in msg
    mr.close()
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 7: the motion library
def test_motion_library_filters_once_at_construction():
    from gmr_amd import dataset
    g = _gmr("unitree_g1")
    q, qd = _qpos("unitree_g1")
    lib = dataset.MotionLibrary(g, qd, OFFS, FPS, lowpass_hz=6.0)
    smoothed = dataset.smooth_qpos(g, qd, OFFS, FPS, 6.0)
    want = dataset.MotionLibrary(g, smoothed, OFFS, FPS)
    assert torch.equal(lib.qpos, smoothed) and not torch.equal(lib.qpos, qd)
    gen = torch.Generator(device="cuda").manual_seed(3)
    ids = lib.sample_ids(257, generator=gen)
    times = lib.sample_times(ids, generator=gen)
    a, b = lib.query(ids, times, dtype=torch.float64), want.query(ids, times, dtype=torch.float64)
    assert _same(_host(a), _host(b))
    # from motion dicts (xyzw root_rot) as well
    motions = [{"fps": float(FPS[s]), "root_pos": q[OFFS[s]:OFFS[s + 1], :3], "root_rot": q[OFFS[s]:OFFS[s + 1], [4, 5, 6, 3]],
                "dof_pos": q[OFFS[s]:OFFS[s + 1], 7:]} for s in range(len(LENGTHS)) if LENGTHS[s] > 0]
    fm = dataset.MotionLibrary.from_motions(g, motions, lowpass_hz=6.0)
    assert torch.equal(fm.qpos, smoothed)


# ------------------------------------------------------------------ 8: stream order with the filter on
def FilteredTrack(v):
    """The gmr_motion_track case of the stream-order tests with the filter on (also run by tests/test_gpu_guard_band.py)."""
    from tests.test_gpu_stream_order import MotionCase

    class FilteredTrack(MotionCase):
        def __init__(self, v):
            super().__init__(v, "track", False)
            self.launches = 2

        def fill(self, st, b, decoy):
            super().fill(st, b, decoy)
            for i in range(len(self.engines)):
                st["inp"][i].lowpass_hz = 3.0 if decoy else 6.0

    return FilteredTrack(v)


def test_late_producer_with_the_filter_on():
    from tests import stream_order as so
    from tests.test_gpu_stream_order import DEV, MotionCase

    case = FilteredTrack(0)
    ser = so.serial_answers(case, DEV())
    assert ser["deterministic"]
    for k in ("dev_decoy", "host_decoy"):
        assert not so.same(ser[k], ser["true"]), k
    plain = so.serial_answers(MotionCase(0, "track", False), DEV())
    assert not so.same(plain["true"], ser["true"])  # (the filter is on)
    spin_ms = so.spin_ms_for(ser["ms"])
    r = so.run_late(case, DEV(), int(spin_ms / so.calibrate_spin()["ms_per_cycle"]))
    print(f"serial {ser['ms']:.3f} ms, spin {spin_ms:.1f} ms, issue took {r['issue_ms']:.3f} ms, returned before producer: {r['returned_before_producer']}")
    assert not r["vacuous"], "the producer had finished before the call was issued: the run proves nothing"
    assert so.same(r["answer"], ser["true"]), f"differs from the serial answer in {so.differing(r['answer'], ser['true'])}"
    assert r["returned_before_producer"]


# ------------------------------------------------------------------ 9: the dataset script
def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_dataset_script_lowpass_flag_end_to_end(tmp_path):
    import pickle
    from gmr_amd import dataset
    from gmr_amd.scripts import smplx_to_robot_dataset
    from gmr_amd.smplx_adapter import iter_joint_batches
    dev = torch.device("cuda", 0)
    g1 = compiled("smplx", "unitree_g1")
    pos, quat, names, offs = synth.synth_clips_torch(g1, np.array([40, 25]), seed=9, device=dev, yaw0=0.5, dtype=torch.float64)
    src = str(tmp_path / "in")
    os.makedirs(src)
    synth.write_smplx_joint_files(src, pos, quat, names, offs, fps=30.0, heights=[1.7, 1.6])
    out, trk = str(tmp_path / "out"), str(tmp_path / "trk")
    assert smplx_to_robot_dataset.main(["--src_folder", src, "--robot", "unitree_g1", "--num_cpus", "2", "--hard_motions", "--tgt_folder", out,
                                        "--track_fps", "50", "--track_folder", trk, "--lowpass_hz", "6"]) == 0
    assert len(_tree(out)) == 2 and _tree(trk) == [f.replace(".pkl", ".npz") for f in _tree(out)]
    g = _gmr("unitree_g1")
    files = sorted(os.path.join(src, f) for f in os.listdir(src))
    (batch,) = list(iter_joint_batches(files, batch_files=1024, device=0, threads=2, columns=g.ik_columns, skip_errors=True))
    qpos = g.retarget_batch(batch.pos, batch.quat, batch.body_names, seq_offsets=batch.seq_offsets, human_heights=batch.human_heights)
    smoothed = dataset.smooth_qpos(g, qpos, batch.seq_offsets, batch.fps, 6.0)
    assert not torch.equal(smoothed, qpos)
    tracks = dataset.tracking_from_qpos(g, smoothed, batch.seq_offsets, batch.fps, 50.0)
    motions = dataset.motions_from_qpos(g, smoothed, batch.seq_offsets, batch.fps)
    stem = lambda f: os.path.splitext(os.path.basename(f))[0]  # noqa: E731
    track_of = {stem(f): w for f, w in zip(batch.files, tracks)}
    motion_of = {stem(f): w for f, w in zip(batch.files, motions)}
    for f in _tree(trk):
        got, w = dataset.load_tracking(os.path.join(trk, f)), track_of[stem(f)]
        for k in dataset.TRACK_ARRAYS:
            assert np.array_equal(got[k], w[k]) and got[k].dtype == w[k].dtype, (f, k)
    for f in _tree(out):
        with open(os.path.join(out, f), "rb") as fh:
            got = pickle.load(fh)
        w = motion_of[stem(f)]
        assert set(got) == set(w)
        for k in ("root_pos", "root_rot", "dof_pos", "local_body_pos"):
            assert np.array_equal(got[k], w[k]), (f, k)

"""The dataset epilogue kernel (gmr_motion_epilogue / gmr_group_motion_epilogue) on the GPU: bit identity with the single-robot
post-processing (dataset.motions_from_qpos: two FK launches and torch ops) for every free-joint robot, in group form, end to end
through MultiRobotRetargeting.retarget_clips, against the oracle, the refusals, and the --robots flag of the dataset scripts."""
import io
import os
import pickle

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gmr_amd import synth  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402
from tests.util import compiled  # noqa: E402

FREE = ["unitree_g1", "unitree_g1_with_hands", "booster_t1", "stanford_toddy", "fourier_n1", "engineai_pm01", "kuavo_s45",
        "hightorque_hi", "booster_k1"]
CONFIG4 = ["unitree_g1", "booster_t1", "stanford_toddy", "fourier_n1", "engineai_pm01"]
KEYS = ("root_pos", "root_rot", "dof_pos", "local_body_pos")
_GMR = {}


def _gmr(robot):
    from gmr_amd import GeneralMotionRetargeting
    if robot not in _GMR:
        _GMR[robot] = GeneralMotionRetargeting("smplx", robot, device=0)
    return _GMR[robot]


def _random_qpos(robot, offs, seed):
    """Hinges uniform within the joint ranges, unit root quaternions (wxyz), root positions around a standing height."""
    cm = compiled("smplx", robot)
    r = cm.robot
    rng = np.random.default_rng(seed)
    N = int(offs[-1])
    hb = sorted(r.hinge_bodies(), key=lambda b: r.qpos_adr[b])
    lim = np.array(r.jnt_range, dtype=np.float64)[hb]
    lo = np.where(lim[:, 0] < lim[:, 1], lim[:, 0], -1.0)
    hi = np.where(lim[:, 0] < lim[:, 1], lim[:, 1], 1.0)
    q = np.empty((N, r.nq))
    q[:, :3] = rng.normal(size=(N, 3)) * [2.0, 2.0, 0.2] + [0.0, 0.0, 0.8]
    w = rng.normal(size=(N, 4))
    q[:, 3:7] = w / np.linalg.norm(w, axis=1, keepdims=True)
    q[:, 7:] = rng.uniform(lo, hi, size=(N, len(hb)))
    return torch.from_numpy(q).cuda()


RAGGED = np.array([0, 37, 37, 101, 330, 331, 500], dtype=np.int64)  # an empty clip, lengths off the 64-frame tile, one over several tiles


def _same_arrays(a, b):
    return all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in KEYS)


@pytest.mark.parametrize("ground", [0.0, 0.05])
@pytest.mark.parametrize("height,origin", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("robot", FREE)
def test_engine_motion_epilogue_bitwise_equals_dataset_path(robot, height, origin, ground):
    from gmr_amd import dataset
    g = _gmr(robot)
    eng = g._engine
    q = _random_qpos(robot, RAGGED, seed=FREE.index(robot) * 4 + 2 * height + origin)
    ref = dataset.motions_from_qpos(g, q, RAGGED, 30, height_adjust=height, root_origin_offset=origin, ground_offset=ground)
    mz = torch.empty(len(RAGGED) - 1, dtype=torch.float32, device=q.device)
    got = eng.motion_epilogue(q, RAGGED, height_adjust=height, root_origin_offset=origin, ground_offset=ground, min_z=mz)
    got = [t.cpu().numpy() for t in got]
    for s in range(len(RAGGED) - 1):
        a, b = RAGGED[s], RAGGED[s + 1]
        for k, arr in zip(KEYS, got):
            assert np.array_equal(arr[a:b], ref[s][k]) and arr.dtype == ref[s][k].dtype, (robot, s, k)
    q32 = q.to(torch.float32)
    want = eng.fk_min_height(q32[:, :3].contiguous(), q[:, [4, 5, 6, 3]].to(torch.float32), q32[:, 7:].contiguous(), RAGGED)
    assert np.array_equal(mz.cpu().numpy(), want.cpu().numpy())


def _mr(robots):
    from gmr_amd import MultiRobotRetargeting
    return MultiRobotRetargeting("smplx", robots, device=0)


def _pickle_bytes(motion):
    from gmr_amd import dataset
    if dataset.fast_pickle_ok():
        return b"".join(bytes(p) for p in dataset.motion_stream(motion))
    f = io.BytesIO()
    pickle.dump(motion, f)
    return f.getvalue()


@pytest.mark.parametrize("robots,offs", [
    (CONFIG4, RAGGED),
    (CONFIG4, np.arange(0, 64 * 1000 + 1, 1000, dtype=np.int64)),          # config 4: 64 clips x 1000 frames per robot
    (["unitree_g1_with_hands", "booster_k1"], RAGGED),                     # the largest tree next to a small one in one grid
])
def test_group_motions_from_qpos_equal_single_robot_path(robots, offs):
    from gmr_amd import dataset
    mr = _mr(robots)
    qpos = {r: _random_qpos(r, offs, seed=11 + i) for i, r in enumerate(robots)}
    fps = [30 + (s % 3) * 30 for s in range(len(offs) - 1)]
    got = mr.motions_from_qpos(qpos, offs, fps, ground_offset=0.05)
    assert list(got) == robots
    for r in robots:
        ref = dataset.motions_from_qpos(_gmr(r), qpos[r], offs, fps, ground_offset=0.05)
        assert len(got[r]) == len(ref)
        for s, (m, w) in enumerate(zip(got[r], ref)):
            assert m.keys() == w.keys() and m["fps"] == w["fps"] and m["link_body_list"] == w["link_body_list"]
            assert _same_arrays(m, w), (r, s)
            if s < 3:
                assert _pickle_bytes(m) == _pickle_bytes(w) and pickle.dumps(m) == pickle.dumps(w), (r, s)
    mr.close()


@pytest.mark.parametrize("chunk", [0, "auto"])
def test_multi_robot_retarget_clips_equal_dataset_retarget_clips(chunk):
    from gmr_amd import dataset
    g1 = compiled("smplx", "unitree_g1")
    pos, quat, names, offs, _ = synth.synth_clips(g1, 3, 150, seed=21, hard=True, dtype=np.float32)
    offs = np.asarray(offs, dtype=np.int64)
    heights = [1.6, 1.8, 1.75]
    fps = [30, 60, 30]
    mr = _mr(CONFIG4)
    got = mr.retarget_clips(pos, quat, names, offs, fps=fps, human_heights=heights, chunk=chunk)
    for r in CONFIG4:
        ref = dataset.retarget_clips(_gmr(r), pos, quat, names, offs, fps=fps, human_heights=heights, chunk=chunk)
        for m, w in zip(got[r], ref):
            assert m["fps"] == w["fps"] and _same_arrays(m, w), r
    mr.close()


def test_group_epilogue_matches_oracle_fk():
    """Independent of the existing path: the oracle's FK with the identity root (local_body_pos) and the real root (height)."""
    offs = np.array([0, 70, 150], dtype=np.int64)
    mr = _mr(CONFIG4)
    qpos = {r: _random_qpos(r, offs, seed=31 + i) for i, r in enumerate(CONFIG4)}
    got = mr.motions_from_qpos(qpos, offs, 30)
    for r in CONFIG4:
        orc = Oracle(compiled("smplx", r).blob)
        qa = qpos[r].cpu().numpy()
        for s, m in enumerate(got[r]):
            a, b = offs[s], offs[s + 1]
            q = qa[a:b]
            root_rot = q[:, [4, 5, 6, 3]]
            ident = np.tile(np.array([[0, 0, 0, 1]], np.float32), (b - a, 1))
            local, _ = orc.fk_kin(np.zeros((b - a, 3), np.float32), ident, q[:, 7:].astype(np.float32), want_rot=False)
            body, _ = orc.fk_kin(q[:, :3].astype(np.float32), root_rot.astype(np.float32), q[:, 7:].astype(np.float32), want_rot=False)
            root_pos = q[:, :3].copy()
            root_pos[:, 2] -= float(body[..., 2].min())
            root_pos[:, :2] -= root_pos[0, :2]
            assert np.abs(m["root_pos"] - root_pos).max() < 5e-6, r
            assert np.array_equal(m["root_rot"], root_rot) and np.array_equal(m["dof_pos"], q[:, 7:])
            assert np.abs(m["local_body_pos"] - local).max() < 5e-6, r
    mr.close()


def test_epilogue_refusals(monkeypatch):
    from gmr_amd.engine import EngineError
    offs = np.array([0, 10], dtype=np.int64)
    # a planar-base member: NotImplementedError before any launch
    mr = _mr(["unitree_g1", "galaxea_r1pro"])

    def boom(*a, **k):
        raise AssertionError("launched")
    monkeypatch.setattr(mr.group, "motion_epilogue", boom)
    q = {"unitree_g1": torch.zeros((10, mr.engines[0].nq), dtype=torch.float64, device="cuda"),
         "galaxea_r1pro": torch.zeros((10, mr.engines[1].nq), dtype=torch.float64, device="cuda")}
    with pytest.raises(NotImplementedError):
        mr.motions_from_qpos(q, offs, 30)
    with pytest.raises(NotImplementedError):
        mr.retarget_clips(np.zeros((10, 3, 3), np.float32), np.zeros((10, 3, 4), np.float32), ["a", "b", "c"], offs)
    mr.close()
    eng = _gmr("unitree_g1")._engine
    q = _random_qpos("unitree_g1", offs, seed=3)
    with pytest.raises(EngineError):
        eng.motion_epilogue(q.to(torch.float32), offs)
    with pytest.raises(EngineError):
        eng.motion_epilogue(q[:, :-1], offs)
    with pytest.raises(EngineError):
        eng.motion_epilogue(q.cpu(), offs)
    with pytest.raises(EngineError):
        eng.motion_epilogue(q, offs, out=(torch.empty((10, 3), dtype=torch.float32, device="cuda"),) * 4)
    with pytest.raises(ValueError):
        eng.motion_epilogue(q, [0, 9])
    with pytest.raises(ValueError):
        eng.motion_epilogue(q, [0, 6, 4, 10])
    mr = _mr(["unitree_g1", "booster_t1"])
    with pytest.raises(ValueError):
        mr.motions_from_qpos({"unitree_g1": q, "booster_t1": _random_qpos("booster_t1", offs, 4)}, [1, 10], 30)
    with pytest.raises(EngineError):
        mr.group.motion_epilogue([(q, offs)])
    mr.close()


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_dataset_scripts_robots_flag_writes_the_single_robot_files(golden_dir, tmp_path, capsys):
    import shutil
    from gmr_amd.scripts import bvh_to_robot_dataset, smplx_to_robot_dataset
    robots = ["unitree_g1", "booster_t1"]
    # SMPL-X joint files
    dev = torch.device("cuda", 0)
    g1 = compiled("smplx", "unitree_g1")
    pos, quat, names, offs = synth.synth_clips_torch(g1, np.array([60, 45, 70]), seed=9, device=dev, yaw0=0.5, dtype=torch.float64)
    src = str(tmp_path / "sm_in")
    os.makedirs(src)
    synth.write_smplx_joint_files(src, pos, quat, names, offs, fps=30.0, heights=[1.7, 1.6, 1.8])
    multi, single = str(tmp_path / "sm_multi"), str(tmp_path / "sm_single")
    assert smplx_to_robot_dataset.main(["--src_folder", src, "--tgt_folder", multi, "--robots", ",".join(robots), "--num_cpus", "2", "--hard_motions"]) == 0
    for r in robots:
        assert smplx_to_robot_dataset.main(["--src_folder", src, "--tgt_folder", os.path.join(single, r), "--robot", r, "--num_cpus", "2",
                                            "--hard_motions"]) == 0
    assert _tree(multi) == _tree(single) and len(_tree(multi)) == 6
    for f in _tree(multi):
        assert open(os.path.join(multi, f), "rb").read() == open(os.path.join(single, f), "rb").read(), f
    # a second run converts only what a robot lacks
    os.remove(os.path.join(multi, "booster_t1", "clip_00001.pkl"))
    t0 = os.path.getmtime(os.path.join(multi, "unitree_g1", "clip_00001.pkl"))
    capsys.readouterr()
    assert smplx_to_robot_dataset.main(["--src_folder", src, "--tgt_folder", multi, "--robots", ",".join(robots), "--num_cpus", "2", "--hard_motions"]) == 0
    assert "full args_list: 1" in capsys.readouterr().out
    assert os.path.getmtime(os.path.join(multi, "unitree_g1", "clip_00001.pkl")) == t0
    assert open(os.path.join(multi, "booster_t1", "clip_00001.pkl"), "rb").read() == open(os.path.join(single, "booster_t1", "clip_00001.pkl"), "rb").read()
    # BVH files
    bsrc = str(tmp_path / "bvh_in")
    os.makedirs(bsrc)
    for n in ("a1.bvh", "a2.bvh"):
        shutil.copy(os.path.join(golden_dir, "bvh_lafan_like.bvh"), os.path.join(bsrc, n))
    bm, bs = str(tmp_path / "bvh_multi"), str(tmp_path / "bvh_single")
    assert bvh_to_robot_dataset.main(["--src_folder", bsrc, "--tgt_folder", bm, "--robots", ",".join(robots)]) == 0
    for r in robots:
        assert bvh_to_robot_dataset.main(["--src_folder", bsrc, "--tgt_folder", os.path.join(bs, r), "--robot", r]) == 0
    assert _tree(bm) == _tree(bs) and len(_tree(bm)) == 4
    for f in _tree(bm):
        assert open(os.path.join(bm, f), "rb").read() == open(os.path.join(bs, f), "rb").read(), f

"""The layers on top of Engine.motion_mirror: dataset.augment_mirror, MotionLibrary(mirror=True), the contact labels of a mirrored
clip, MultiRobotRetargeting.retarget_clips(mirror=True) and the dataset script's --mirror."""
import functools
import itertools
import os
import pickle

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gmr_amd import synth  # noqa: E402
from tests import contact_reference as CR  # noqa: E402
from tests import mirror_inputs as mi  # noqa: E402
from tests.test_gpu_dynamics import DEV, _bytes, _dev  # noqa: E402
from tests.test_gpu_mirror import gpu  # noqa: E402
from tests.util import compiled  # noqa: E402

K1 = "booster_k1"
FEET = ["left_foot_link", "right_foot_link"]


@functools.lru_cache(maxsize=None)
def retargeter(robot):
    from gmr_amd import GeneralMotionRetargeting
    return GeneralMotionRetargeting("smplx", robot, device=0, verbose=False)


def signed_permutation(plan, dof):
    """The hinge part of the mirror on a dof array [T, nq - 7]: copies and sign flips, exact in any dtype."""
    src, neg = plan.col_src[7:] - 7, plan.col_sign[7:] < 0.0
    g = dof[:, src]
    return np.where(neg, -g, g)


def test_augment_mirror_keeps_the_originals_first_and_doubles_the_offsets():
    from gmr_amd import dataset
    g = retargeter(K1)
    q = _dev(mi.qpos(K1))
    for about in mi.MODES:
        q2, offs2, fps2 = dataset.augment_mirror(g, q, mi.OFFS, 30.0, about=about)
        assert tuple(q2.shape) == (2 * mi.N, g._engine.nq) and fps2 == 30.0
        assert offs2.dtype == np.int64 and np.array_equal(offs2, np.concatenate([mi.OFFS, mi.OFFS[1:] + mi.N]))
        assert np.array_equal(_bytes(q2[:mi.N].cpu().numpy()), _bytes(mi.qpos(K1)))
        assert np.array_equal(_bytes(q2[mi.N:].cpu().numpy()), _bytes(gpu(K1, about)))           # clip S + i is the mirror of clip i
    assert dataset.augment_mirror.__defaults__[0] == "start"
    rates = np.linspace(20.0, 60.0, mi.S)
    _, _, fps2 = dataset.augment_mirror(g, q, mi.OFFS, rates)
    assert np.array_equal(fps2, np.concatenate([rates, rates]))
    assert np.array_equal(_bytes(dataset.mirror_qpos(g, q, mi.OFFS).cpu().numpy()), _bytes(gpu(K1, "world")))   # about="world" by default
    assert np.array_equal(_bytes(g.mirror_qpos(np.array(mi.qpos(K1)), mi.OFFS, about="start").cpu().numpy()), _bytes(gpu(K1, "start")))
    assert g.symmetry_plan() is g._engine.symmetry_plan() and np.array_equal(g.symmetry_plan(tol_pos=1e-6).col_src, mi.plan(K1).col_src)
    from gmr_amd.symmetry import SymmetryError
    with pytest.raises(SymmetryError, match="left_shoulder_pitch_link"):
        retargeter("unitree_g1").symmetry_plan(tol_pos=1e-6)


def test_motion_library_mirror_doubles_the_clips_and_answers_like_a_library_of_the_mirrored_qpos():
    from gmr_amd import dataset
    g = retargeter(K1)
    q = _dev(mi.qpos(K1))
    lib = dataset.MotionLibrary(g, q, mi.OFFS, fps=30.0, mirror=True)
    plain = dataset.MotionLibrary(g, q, mi.OFFS, fps=30.0)
    mirrored = dataset.MotionLibrary(g, _dev(gpu(K1, "start")), mi.OFFS, fps=30.0)
    assert lib.num_clips == 2 * plain.num_clips == 2 * mi.S and lib.num_frames == 2 * mi.N
    assert np.array_equal(lib.durations.cpu().numpy(), np.concatenate([plain.durations.cpu().numpy()] * 2))
    live = [s for s, T in enumerate(mi.LENS) if T]
    ids = torch.tensor(live, dtype=torch.int64, device=DEV())
    times = plain.durations[ids] * torch.linspace(0.1, 0.9, len(live), dtype=torch.float64, device=DEV())
    a, b = lib.query(ids + mi.S, times), mirrored.query(ids, times)
    c, d = lib.query(ids, times), plain.query(ids, times)
    assert sorted(a) == sorted(b) and len(a) == 10
    for k in a:
        assert np.array_equal(_bytes(a[k].cpu().numpy()), _bytes(b[k].cpu().numpy())), k       # id S + i: the mirrored clip i, bytes equal
        assert np.array_equal(_bytes(c[k].cpu().numpy()), _bytes(d[k].cpu().numpy())), k       # id i: unchanged
    assert not np.array_equal(a["joint_pos"].cpu().numpy(), c["joint_pos"].cpu().numpy())
    world = dataset.MotionLibrary(g, q, mi.OFFS, fps=30.0, mirror=True, mirror_about="world")
    assert np.array_equal(_bytes(world.qpos[mi.N:].cpu().numpy()), _bytes(gpu(K1, "world")))


@functools.lru_cache(maxsize=None)
def stepping_clip():
    """48 frames of booster_k1 standing (root off the plane y = 0 and turned by 0.4 rad), the left foot lifted 13 cm between frames
    12 and 24 and held up, the left arm moved: nothing about it is symmetric."""
    nq = compiled("smplx", K1).robot.nq
    k = np.arange(48)
    s = np.clip((k - 12) / 12.0, 0.0, 1.0)
    s = s * s * (3.0 - 2.0 * s)
    q = np.zeros((48, nq))
    q[:, 0], q[:, 1], q[:, 2] = 0.2, 0.3, 0.9
    q[:, 3], q[:, 6] = np.cos(0.2), np.sin(0.2)
    q[:, 17], q[:, 20], q[:, 21] = -0.8 * s, 1.6 * s, -0.3 * s      # left hip pitch, knee, ankle pitch
    q[:, 9], q[:, 10] = 0.5, -0.4 * s                               # left shoulder pitch and roll
    return q, np.array([0, 48], np.int64)


def test_contact_labels_of_a_mirrored_clip_are_the_originals_with_the_columns_swapped():
    from gmr_amd import dataset
    g = retargeter(K1)
    plan = g.symmetry_plan()
    q, offs = stepping_clip()
    assert plan.mirror_names(FEET) == FEET[::-1]
    orig = dataset.tracking_from_qpos(g, _dev(q), offs, 30.0, 30.0, contact_bodies=FEET)[0]
    # no threshold is within rounding of a label flip on this clip: the numpy contact reference gives the same labels on the
    # exported arrays with every threshold moved either way by far more than the mirror's rounding (1e-4 m, 1e-3 m/s)
    ids = [list(orig["body_names"]).index(n) for n in FEET]
    prm = dataset.ContactParams()
    pos, vel = np.ascontiguousarray(orig["body_pos_w"], np.float32), np.ascontiguousarray(orig["body_lin_vel_w"], np.float32)
    want = np.asarray(orig["contact"])
    for dh_on, dh_off, dv_on, dv_off in itertools.product((-1e-4, 1e-4), (-1e-4, 1e-4), (-1e-3, 1e-3), (-1e-3, 1e-3)):
        ref = CR.contacts(pos, vel, offs, ids, None, CR.GROUND_CLIP_MIN, 0.0, prm.height_on + dh_on, prm.height_off + dh_off,
                          prm.speed_on + dv_on, prm.speed_off + dv_off)
        assert np.array_equal(ref["contact"], want), (dh_on, dh_off, dv_on, dv_off)
    assert want[:, 1].all() and want[:12, 0].all() and not want[24:, 0].any()            # the right foot stands, the left one leaves the ground
    for about in mi.MODES:
        qm = dataset.mirror_qpos(g, _dev(q), offs, about=about)
        same_names = dataset.tracking_from_qpos(g, qm, offs, 30.0, 30.0, contact_bodies=FEET)[0]
        swapped = dataset.tracking_from_qpos(g, qm, offs, 30.0, 30.0, contact_bodies=plan.mirror_names(FEET))[0]
        assert np.array_equal(np.asarray(same_names["contact"]), want[:, ::-1]), about      # the right foot is now the one that lifts
        assert np.array_equal(np.asarray(swapped["contact"]), want), about                # ... and under the mirrored names, the same table
        assert list(swapped["contact_body_names"]) == FEET[::-1]
        for k in ("frames", "touchdowns"):
            assert np.array_equal(swapped["contact_stats"][k], orig["contact_stats"][k]), (about, k)


@functools.lru_cache(maxsize=None)
def two_clips(head=False):
    """Two clips of 24 frames of G1's key-points; ``head``: plus the head booster_k1's tasks ask for, 0.25 m above spine3."""
    cm = compiled("smplx", "unitree_g1")
    pos, quat, names, offs, _ = synth.synth_clips(cm, 2, 24, seed=12, hard=False, dtype=np.float64)
    if head:
        i = names.index("spine3")
        pos = np.concatenate([pos, pos[:, i:i + 1] + np.array([0.0, 0.0, 0.25])], axis=1)
        quat = np.concatenate([quat, quat[:, i:i + 1]], axis=1)
        names = list(names) + ["head"]
    return pos, quat, names, np.asarray(offs, dtype=np.int64)


def test_multi_robot_retarget_clips_mirror_returns_twice_the_clips_per_robot():
    from gmr_amd import MultiRobotRetargeting
    from gmr_amd.symmetry import SymmetryError
    pos, quat, names, offs = two_clips(head=True)
    robots = ["unitree_g1", "booster_k1"]
    mr = MultiRobotRetargeting("smplx", robots, device=0)
    plain = mr.retarget_clips(pos, quat, names, offs)
    both, tracks = mr.retarget_clips(pos, quat, names, offs, mirror=True, track_fps=30.0)
    for r, eng in zip(robots, mr.group.engines):
        plan = eng.symmetry_plan()
        assert len(plain[r]) == 2 and len(both[r]) == 4 and len(tracks[r]) == 4
        for i in range(2):
            for k in ("root_pos", "root_rot", "dof_pos", "local_body_pos"):
                assert np.array_equal(both[r][i][k], plain[r][i][k]), (r, i, k)            # the originals come first, unchanged
            assert np.array_equal(both[r][2 + i]["dof_pos"], signed_permutation(plan, np.asarray(plain[r][i]["dof_pos"]))), (r, i)
            assert both[r][2 + i]["root_pos"].shape == plain[r][i]["root_pos"].shape and both[r][2 + i]["fps"] == plain[r][i]["fps"]
            assert np.array_equal(tracks[r][2 + i]["joint_pos"], signed_permutation(plan, np.asarray(tracks[r][i]["joint_pos"]))), (r, i)
    world = mr.retarget_clips(pos, quat, names, offs, mirror={"about": "world"})
    assert len(world["booster_k1"]) == 4
    # a robot whose plan is refused raises before any solve: the solve of this group would need a GPU call that never happens
    bad = MultiRobotRetargeting("smplx", ["unitree_g1", "stanford_toddy"], device=0)
    calls = []
    bad._solve = lambda *a, **k: calls.append(1)
    with pytest.raises(SymmetryError, match="stanford_toddy"):
        bad.retarget_clips(pos, quat, names, offs, mirror=True)
    assert not calls


def test_the_dataset_script_writes_x_mirror_pkl_beside_every_clip(tmp_path):
    from gmr_amd.scripts import smplx_to_robot_dataset
    pos, quat, names, offs = two_clips()
    src = str(tmp_path / "in")
    os.makedirs(src)
    synth.write_smplx_joint_files(src, torch.from_numpy(pos), torch.from_numpy(quat), names, offs, fps=30.0)
    files = sorted(os.listdir(src))
    assert len(files) == 2
    base = ["--src_folder", src, "--num_cpus", "2", "--hard_motions"]
    plain, out = str(tmp_path / "plain"), str(tmp_path / "out")
    assert smplx_to_robot_dataset.main(base + ["--tgt_folder", plain]) == 0
    assert smplx_to_robot_dataset.main(base + ["--tgt_folder", out, "--mirror"]) == 0
    stems = [f.replace(".npz", "") for f in files]
    assert sorted(os.listdir(plain)) == [s + ".pkl" for s in stems]                        # nothing changes without the flag
    assert sorted(os.listdir(out)) == sorted([s + ".pkl" for s in stems] + [s + "_mirror.pkl" for s in stems])
    plan = retargeter("unitree_g1").symmetry_plan()
    for s in stems:
        assert open(os.path.join(out, s + ".pkl"), "rb").read() == open(os.path.join(plain, s + ".pkl"), "rb").read()
        with open(os.path.join(out, s + ".pkl"), "rb") as f:
            m = pickle.load(f)
        with open(os.path.join(out, s + "_mirror.pkl"), "rb") as f:
            mm = pickle.load(f)
        assert sorted(mm) == sorted(m) and mm["fps"] == m["fps"]
        assert np.array_equal(mm["dof_pos"], signed_permutation(plan, np.asarray(m["dof_pos"])))
        assert not np.array_equal(mm["dof_pos"], m["dof_pos"]) and mm["root_pos"].shape == m["root_pos"].shape

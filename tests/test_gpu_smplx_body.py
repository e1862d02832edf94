"""The SMPL-X body kernel (gmr_smplx_body) and the AMASS file path on the GPU.  Models are random stand-ins (synth.write_smplx_model)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PARENTS = None


def _setup(tmp_path, seed=0):
    from gmr_amd import synth
    from gmr_amd.smplx_body import BodyModelSet
    folder = synth.write_smplx_model_folder(str(tmp_path / "models"), seed=seed)
    return folder, BodyModelSet(folder)


def _restatement(model, betas, root, pose, trans):
    """Section 2 of the feature, the slow way: scipy rotations, an explicit parent loop, float64."""
    from scipy.spatial.transform import Rotation as R
    from gmr_amd.smplx_adapter import SMPLX_PARENTS
    T = root.shape[0]
    J = model.rest_joints(betas)
    fp = np.zeros((T, 55, 3))
    fp[:, 0] = root
    fp[:, 1:22] = pose.astype(np.float64).reshape(T, 21, 3)
    fp[:, 25:55] = model.hand_mean.reshape(30, 3)
    Rg, p = [None] * 55, np.zeros((T, 55, 3))
    for i, par in enumerate(SMPLX_PARENTS):
        Rl = R.from_rotvec(fp[:, i])
        if par < 0:
            Rg[i], p[:, i] = Rl, J[0]
        else:
            Rg[i] = Rg[par] * Rl
            p[:, i] = p[:, par] + Rg[par].apply(J[i] - J[par])
    return root.astype(np.float64), fp, p + trans.astype(np.float64)[:, None]


def _clips(models, lens, dtypes, dev, seed, big=True):
    from gmr_amd import synth
    out, host = [], []
    for k, T in enumerate(lens):
        a = synth.amass_arrays(T, seed + k, dtypes[k % len(dtypes)], big=big)
        m = models.get(("neutral", "male", "female")[k % 3])
        nb = (16, 10, 0)[k % 3]
        c = dict(model=m, betas=a["betas"][:nb])
        for key in ("root_orient", "pose_body", "trans"):
            c[key] = torch.as_tensor(a[key]).to(dev)
        out.append(c)
        host.append((m, a["betas"][:nb], a["root_orient"], a["pose_body"], a["trans"]))
    return out, host


def test_body_kernel_against_scipy_restatement(tmp_path):
    """G1: several clips of several lengths in one launch (T = 1 and an empty clip among them), float32 and float64 inputs, angles
    near 0 and beyond pi, three models, 16 / 10 / 0 betas; all 55 joints and an IK config's 14 columns.  full_pose / global_orient exact,
    joints within 1e-10 m (the bound of this kernel family, test_smplx_keypoints_random_trees).  Measured: see DESIGN 4.8."""
    from gmr_amd import GeneralMotionRetargeting as GMR, smplx_body
    from gmr_amd.smplx_adapter import SMPLX_JOINT_NAMES, SMPLX_PARENTS
    dev = torch.device("cuda", 0)
    _, models = _setup(tmp_path)
    lens = [301, 1, 0, 64, 2, 777, 33]
    clips, host = _clips(models, lens, (np.float64, np.float32), dev, seed=20)
    go, fp, jt, offs, rest = smplx_body.evaluate_clips(clips, return_rest=True)
    assert offs.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist() and go.shape == (sum(lens), 3) and jt.shape == (sum(lens), 55, 3)
    worst, worst_rest = 0.0, 0.0
    for k, h in enumerate(host):
        a, e = offs[k], offs[k + 1]
        w_go, w_fp, w_jt = _restatement(*h)
        assert np.array_equal(go[a:e].cpu().numpy(), w_go) and np.array_equal(fp[a:e].cpu().numpy(), w_fp)
        worst_rest = max(worst_rest, float(np.abs(rest[k].cpu().numpy() - h[0].rest_joints(h[1])).max()))
        if e > a:
            worst = max(worst, float(np.abs(jt[a:e].cpu().numpy() - w_jt).max()))
    print(f"G1: max |joints - restatement| = {worst:.3e} m, max |rest - host rest_joints| = {worst_rest:.3e} m")
    assert worst_rest < 1e-13 and worst < 1e-10
    cols = GMR(src_human="smplx", tgt_robot="unitree_g1").ik_columns
    assert len(cols) == 14
    go2, fp2, jt2, _ = smplx_body.evaluate_clips(clips, columns=cols)
    live = set()
    for c in cols:
        j = SMPLX_JOINT_NAMES.index(c)
        while j >= 0:
            live.add(j)
            j = SMPLX_PARENTS[j]
    live = sorted(live)
    assert len(live) < 32  # several frames share a wavefront
    assert torch.equal(go2, go) and torch.equal(fp2[:, live], fp[:, live]) and torch.equal(jt2[:, live], jt[:, live])
    # nothing at all
    g0 = smplx_body.evaluate_clips([])
    assert g0[0].shape == (0, 3) and g0[3].tolist() == [0]


def _write_batch(tmp_path, folder):
    from gmr_amd import synth
    lens, fps = [481, 90, 7, 250, 1, 120], [120.0, 30.0, 120.0, 60.0, 30.0, 120.0]
    return synth.write_amass_files(str(tmp_path / "amass"), lens, seed=40, fps=fps, dtypes=(np.float64, np.float32), genders=("male", "female", "neutral"),
                                   compressed=(False, True, True, False))


def test_amass_batch_equals_kernel_then_adapter(tmp_path):
    """G2: load_amass_files is, bit for bit, get_smplx_data_offline_fast on the body kernel's own standalone outputs, clip by clip --
    120 -> 30 fps and 1:1 clips, float32 and float64 files, stored and deflated, all 55 columns and ik_columns; heights, fps and
    seq_offsets as load_joint_files gives them for joint files written from the same arrays."""
    from gmr_amd import GeneralMotionRetargeting as GMR, smplx_body
    from gmr_amd import smplx_adapter as sa
    dev = torch.device("cuda", 0)
    folder, models = _setup(tmp_path, seed=5)
    files, arrays = _write_batch(tmp_path, folder)
    g = GMR(src_human="smplx", tgt_robot="unitree_g1")
    for cols in (None, g.ik_columns):
        b = sa.load_amass_files(files, folder, columns=cols)
        assert len(b) == len(files) and b.files == files and b.body_names == (sa.SMPLX_JOINT_NAMES if cols is None else cols) and not b.skipped
        jfiles = []
        for k, a in enumerate(arrays):
            m = models.get(a["gender"])
            clip = dict(model=m, betas=m.clip_betas(a["betas"]), **{key: torch.as_tensor(a[key]).to(dev) for key in ("root_orient", "pose_body", "trans")})
            go, fp, jt, _ = smplx_body.evaluate_clips([clip], columns=cols)
            p, q, names, afps = sa.get_smplx_data_offline_fast(go, fp, jt, src_fps=a["mocap_frame_rate"], columns=cols)
            s, e = b.seq_offsets[k], b.seq_offsets[k + 1]
            assert torch.equal(b.pos[s:e], p) and torch.equal(b.quat[s:e], q) and b.fps[k] == afps
            if cols is None:
                jf = str(tmp_path / f"joint_{k}.npz")
                sa.save_joint_file(jf, jt.cpu().numpy(), go.cpu().numpy(), fp.reshape(fp.shape[0], -1).cpu().numpy(), a["mocap_frame_rate"], a["betas"])
                jfiles.append(jf)
        if cols is None:
            jb = sa.load_joint_files(jfiles)
            assert jb.seq_offsets.tolist() == b.seq_offsets.tolist() == [0, 120, 210, 211, 336, 337, 367]
            assert jb.fps == b.fps and jb.human_heights == b.human_heights
            assert torch.equal(jb.pos, b.pos) and torch.equal(jb.quat, b.quat)
    b10 = sa.load_amass_files(files[:1], folder, num_betas=10)
    m = models.get("male")
    assert float((b10.pos[0, 0] - torch.as_tensor(m.rest_joints(arrays[0]["betas"][:10])[0] + arrays[0]["trans"][0]).to(dev)).abs().max()) < 1e-12


def _qrot(q, v):
    w, u = q[..., :1], q[..., 1:]
    t = 2.0 * torch.cross(u, v, dim=-1)
    return v + w * t + torch.cross(u, t, dim=-1)


def test_positions_follow_the_parents_orientation(tmp_path):
    """G3: on un-resampled clips pos_i - pos_parent = R(quat_parent) (J_i - J_parent) and pos_0 = J_0 + trans, 1e-10, for every joint
    and frame -- the orientation the adapter derives is the rotation the body kernel built the position with."""
    from gmr_amd import synth
    from gmr_amd import smplx_adapter as sa
    dev = torch.device("cuda", 0)
    folder, models = _setup(tmp_path, seed=9)
    files, arrays = synth.write_amass_files(str(tmp_path / "a"), [200, 31, 5], seed=70, fps=30.0, dtypes=(np.float64, np.float32), genders=("female", "neutral"),
                                            compressed=(True, False), big=True)
    b = sa.load_amass_files(files, folder)
    par = torch.as_tensor(sa.SMPLX_PARENTS, device=dev)
    worst = 0.0
    for k, a in enumerate(arrays):
        s, e = b.seq_offsets[k], b.seq_offsets[k + 1]
        J = torch.as_tensor(models.get(a["gender"]).rest_joints(a["betas"])).to(dev)
        pos, quat = b.pos[s:e], b.quat[s:e]
        root = (pos[:, 0] - (J[0] + torch.as_tensor(a["trans"]).to(dev, torch.float64))).abs().max()
        d = pos[:, 1:] - pos[:, par[1:]] - _qrot(quat[:, par[1:]], (J[1:] - J[par[1:]]).expand(e - s, 54, 3))
        worst = max(worst, float(root), float(d.abs().max()))
    print(f"G3: max geometry residual = {worst:.3e} m")
    assert worst < 1e-10


def test_script_end_to_end_from_amass_files(tmp_path, capsys):
    """G4: model folder + AMASS files -> python -m gmr_amd.scripts.smplx_to_robot_dataset --smplx_model_folder -> pickles equal to
    dataset.retarget_clips on the load_amass_files batch; the same with --robots; without the flag joint files give the pickles they
    gave before (the joint-file batch solved in memory)."""
    from gmr_amd import GeneralMotionRetargeting as GMR, MultiRobotRetargeting, dataset, synth
    from gmr_amd import smplx_adapter as sa
    from gmr_amd.scripts import smplx_to_robot_dataset
    folder, _ = _setup(tmp_path, seed=2)
    src = str(tmp_path / "amass")
    files, arrays = synth.write_amass_files(src, [60, 45, 30], seed=80, fps=[120.0, 30.0, 60.0], dtypes=(np.float64, np.float32), genders=("male", "neutral"),
                                            compressed=(False, True))
    open(os.path.join(src, "broken.npz"), "wb").write(b"PK nothing")
    synth.write_amass_file(os.path.join(src, "alien.npz"), arrays[0], gender="robot")
    tgt = str(tmp_path / "out")
    assert smplx_to_robot_dataset.main(["--src_folder", src, "--tgt_folder", tgt, "--robot", "unitree_g1", "--smplx_model_folder", folder, "--hard_motions"]) == 0
    out = capsys.readouterr().out
    assert "broken.npz" in out and "alien.npz" in out and "3 files written, 2 could not be loaded" in out
    g = GMR(src_human="smplx", tgt_robot="unitree_g1")
    b = sa.load_amass_files(files, folder, columns=g.ik_columns)
    ref = dataset.retarget_clips(g, b.pos, b.quat, b.body_names, b.seq_offsets, fps=b.fps, human_heights=b.human_heights)
    keys = ("root_pos", "root_rot", "dof_pos", "local_body_pos")
    for k, f in enumerate(files):
        d = dataset.load_robot_motion(os.path.join(tgt, os.path.basename(f)[:-4] + ".pkl"))[0]
        dataset.validate_motion(d, nq=36)
        assert d["fps"] == ref[k]["fps"] and all(np.array_equal(d[key], ref[k][key]) for key in keys)
    tgt2 = str(tmp_path / "out2")
    robots = ["unitree_g1", "booster_t1"]
    assert smplx_to_robot_dataset.main(["--src_folder", src, "--tgt_folder", tgt2, "--robots", ",".join(robots), "--smplx_model_folder", folder, "--hard_motions"]) == 0
    mr = MultiRobotRetargeting("smplx", robots)
    bm = sa.load_amass_files(files, folder, columns=mr.ik_columns)
    refm = mr.retarget_clips(bm.pos, bm.quat, bm.body_names, bm.seq_offsets, fps=bm.fps, human_heights=bm.human_heights)
    for r in robots:
        for k, f in enumerate(files):
            d = dataset.load_robot_motion(os.path.join(tgt2, r, os.path.basename(f)[:-4] + ".pkl"))[0]
            assert all(np.array_equal(d[key], refm[r][k][key]) for key in keys)
    # joint files, no flag: what the joint-file path gave before
    jsrc, jtgt = str(tmp_path / "joint"), str(tmp_path / "jout")
    os.makedirs(jsrc)
    full = sa.load_amass_files(files[1:2], folder)  # (a 30 fps clip: no resampling, so its key-points round-trip through a joint file)
    jfiles = synth.write_smplx_joint_files(jsrc, full.pos, full.quat, full.body_names, full.seq_offsets, fps=30.0, heights=full.human_heights, dtype=np.float64)
    assert smplx_to_robot_dataset.main(["--src_folder", jsrc, "--tgt_folder", jtgt, "--robot", "unitree_g1", "--hard_motions"]) == 0
    jb = sa.load_joint_files(jfiles, columns=g.ik_columns)
    jref = dataset.retarget_clips(GMR(src_human="smplx", tgt_robot="unitree_g1"), jb.pos, jb.quat, jb.body_names, jb.seq_offsets, fps=jb.fps, human_heights=jb.human_heights)
    d = dataset.load_robot_motion(os.path.join(jtgt, os.path.basename(jfiles[0])[:-4] + ".pkl"))[0]
    assert all(np.array_equal(d[key], jref[0][key]) for key in keys)


def test_native_single_file_loader(tmp_path):
    """G5: utils.smpl.load_smplx_file_native + get_smplx_data_offline_fast: per-frame dicts equal to the batch path's rows run on the same
    float32 body-model outputs (the dtype the `smplx` package emits, which this drop-in keeps)."""
    from gmr_amd import synth
    from gmr_amd import smplx_adapter as sa
    from gmr_amd.utils import smpl
    folder, models = _setup(tmp_path, seed=3)
    files, arrays = synth.write_amass_files(str(tmp_path / "a"), [97, 40], seed=90, fps=[120.0, 30.0], genders=("female",), compressed=(True, False))
    for f, a in zip(files, arrays):
        data, body, out, height = smpl.load_smplx_file_native(f, folder)
        assert body.parents.tolist() == list(sa.SMPLX_PARENTS) and abs(height - (1.66 + 0.1 * a["betas"][0])) < 1e-15
        assert out.joints.dtype == torch.float32 and out.full_pose.shape == (a["root_orient"].shape[0], 165) and out.joints.shape[1:] == (55, 3)
        frames, fps = smpl.get_smplx_data_offline_fast(data, body, out, tgt_fps=30)
        p, q, names, afps = sa.get_smplx_data_offline_fast(out.global_orient, out.full_pose, out.joints, src_fps=a["mocap_frame_rate"])
        assert len(frames) == p.shape[0] and (fps == afps if a["mocap_frame_rate"] > 30 else fps == 30)
        p, q = p.cpu().numpy(), q.cpu().numpy()
        for t in (0, len(frames) // 2, len(frames) - 1):
            assert list(frames[t]) == names and all(np.array_equal(frames[t][n][0], p[t, i]) and np.array_equal(frames[t][n][1], q[t, i]) for i, n in enumerate(names))
        b = sa.load_amass_files([f], folder)  # the float64 batch path: the same clip up to the float32 rounding of the drop-in's arrays
        assert float((b.pos - torch.as_tensor(p).to(b.pos.device)).abs().max()) < 5e-6


def test_iter_amass_batches(tmp_path):
    """G6: batches smaller than the folder, a bad file and an all-bad group: the clips of one load_amass_files call in the same order,
    the bad files in `skipped`, an empty batch for the group without a good file."""
    from gmr_amd import smplx_adapter as sa
    folder, _ = _setup(tmp_path, seed=4)
    files, arrays = _write_batch(tmp_path, folder)
    bad1, bad2, bad3 = (str(tmp_path / n) for n in ("bad1.npz", "bad2.npz", "bad3.npz"))
    open(bad1, "wb").write(b"not a zip")
    np.savez(bad2, root_orient=np.zeros((3, 3)))
    open(bad3, "wb").write(open(files[0], "rb").read()[:5000])
    seq = [files[0], bad1, files[1], files[2], bad2, bad3, files[3], files[4], files[5]]
    with pytest.raises(ValueError):
        list(sa.iter_amass_batches(seq, folder, batch_files=2))
    got = list(sa.iter_amass_batches(seq, folder, batch_files=2, skip_errors=True))
    assert [bb.files for bb in got] == [[files[0]], [files[1], files[2]], [], [files[3], files[4]], [files[5]]]
    assert [[f for f, _ in bb.skipped] for bb in got] == [[bad1], [], [bad2, bad3], [], []]
    assert len(got[2]) == 0 and got[2].pos.shape[0] == 0
    whole = sa.load_amass_files(files, folder)
    assert torch.equal(torch.cat([bb.pos for bb in got if len(bb)]), whole.pos) and torch.equal(torch.cat([bb.quat for bb in got if len(bb)]), whole.quat)
    assert sum((bb.fps for bb in got), []) == whole.fps and sum((bb.human_heights for bb in got), []) == whole.human_heights

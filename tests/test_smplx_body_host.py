"""Host side of the SMPL-X body model (gmr_amd.smplx_body) and of the AMASS file loader: model folding, archive parsing, script flags.
Every "model" here is a random stand-in (gmr_amd.synth.write_smplx_model); nothing licensed is read."""
import os
import pickle

import numpy as np
import pytest
import torch

from gmr_amd import smplx_adapter as sa
from gmr_amd import smplx_body, synth
from gmr_amd.smplx_body import SmplxBodyModel


def _long_way(d, betas, nb):
    return d["J_regressor"] @ (d["v_template"] + d["shapedirs"][:, :, :nb] @ betas[:nb])


@pytest.mark.parametrize("ext", ["npz", "pkl"])
def test_rest_joints_equal_the_regressed_shaped_vertices(tmp_path, ext):
    """H1: rest_joints(betas) against J_regressor @ (v_template + shapedirs betas) in float64 -- the same sums in another order, so the
    bound is a few ulp of the joint magnitude: 8 * eps * max|J|."""
    rng = np.random.default_rng(5)
    for k, V in enumerate((200, 1000, 3000)):
        p = str(tmp_path / f"m{k}.{ext}")
        d = synth.write_smplx_model(p, seed=10 + k, n_verts=V)
        m = SmplxBodyModel.from_file(p)
        assert m.J_template.shape == (55, 3) and m.J_dirs.shape == (55, 3, 16) and m.parents.tolist() == list(sa.SMPLX_PARENTS)
        assert np.array_equal(m.hand_mean, np.concatenate([d["hands_meanl"], d["hands_meanr"]]))
        for _ in range(4):
            betas = rng.normal(0.0, 1.5, 16)
            want = _long_way(d, betas, 16)
            err = np.abs(m.rest_joints(betas) - want).max()
            bound = 8 * np.finfo(np.float64).eps * np.abs(want).max()
            print(f"V={V}: |rest - long way| = {err:.3e}, bound {bound:.3e}")
            assert err <= bound
    import gmr_amd
    assert gmr_amd.SmplxBodyModel is SmplxBodyModel


def test_model_file_rules(tmp_path):
    """H2: num_betas, a wrong tree, missing keys, a J_regressor that is not an ndarray but has .toarray(), from_folder's layout."""
    p = str(tmp_path / "m.npz")
    d = synth.write_smplx_model(p, seed=1)
    betas = np.random.default_rng(2).normal(size=16)
    m10 = SmplxBodyModel.from_file(p, num_betas=10)
    assert m10.num_betas == 10
    assert np.abs(m10.rest_joints(betas) - _long_way(d, betas, 10)).max() < 1e-14
    full = SmplxBodyModel.from_file(p)
    assert np.abs(full.rest_joints(betas[:10]) - _long_way(d, betas, 10)).max() < 1e-14       # a 10-beta file on a 16-column model
    assert full.clip_betas(betas).shape == (16,) and m10.clip_betas(betas).shape == (10,) and full.clip_betas(betas, 10).shape == (10,)
    with pytest.raises(ValueError, match="num_betas"):
        full.clip_betas(betas[:10], 16)
    with pytest.raises(ValueError, match="num_betas"):
        SmplxBodyModel.from_file(p, num_betas=17)
    for key in smplx_body.MODEL_KEYS:
        q = str(tmp_path / f"no_{key}.npz")
        np.savez(q, **{k: v for k, v in d.items() if k != key})
        with pytest.raises(ValueError, match=key):
            SmplxBodyModel.from_file(q)
    kin = d["kintree_table"].copy()
    kin[0, 7] = 3
    q = str(tmp_path / "tree.npz")
    np.savez(q, **dict(d, kintree_table=kin))
    with pytest.raises(ValueError, match="kinematic tree"):
        SmplxBodyModel.from_file(q)
    q = str(tmp_path / "few.npz")
    np.savez(q, **dict(d, J_regressor=d["J_regressor"][:24], kintree_table=d["kintree_table"][:, :24]))
    with pytest.raises(ValueError, match="kinematic tree"):
        SmplxBodyModel.from_file(q)
    q = str(tmp_path / "sparse.pkl")
    ds = synth.write_smplx_model(q, seed=1, sparse_like=True)
    with open(q, "rb") as f:
        assert not isinstance(pickle.load(f, encoding="latin1")["J_regressor"], np.ndarray)
    assert np.array_equal(SmplxBodyModel.from_file(q).J_template, full.J_template) and np.array_equal(ds["J_regressor"], d["J_regressor"])
    folder = synth.write_smplx_model_folder(str(tmp_path / "models"), seed=3, genders=("neutral", "male"))
    assert SmplxBodyModel.from_folder(folder, "male").path.endswith(os.path.join("smplx", "SMPLX_MALE.npz"))
    os.rename(os.path.join(folder, "smplx", "SMPLX_MALE.npz"), os.path.join(folder, "smplx", "keep.npz"))
    synth.write_smplx_model(os.path.join(folder, "smplx", "SMPLX_MALE.pkl"), seed=4)
    assert SmplxBodyModel.from_folder(folder, "MALE").path.endswith("SMPLX_MALE.pkl")
    with pytest.raises(ValueError, match="SMPLX_FEMALE"):
        SmplxBodyModel.from_folder(folder, "female")
    with pytest.raises(ValueError, match="gender"):
        SmplxBodyModel.from_folder(folder, "robot")
    ms = smplx_body.BodyModelSet(folder)
    assert ms.get("neutral") is ms.get("Neutral")
    with pytest.raises(ValueError):
        smplx_body.BodyModelSet({"male": full}).get("female")


def _host_alloc(n):
    return torch.empty(n, dtype=torch.uint8)


def test_amass_member_parser(tmp_path):
    """H3: stored and deflated archives give the same arrays; object-dtype and unknown members are ignored; gender as str, bytes or
    0-d array; a truncated file, a missing pose_body, a frame-count mismatch and a non-positive frame rate are ValueErrors, left out
    under skip_errors."""
    a = synth.amass_arrays(37, seed=3, dtype=np.float64)
    a32 = synth.amass_arrays(12, seed=4, dtype=np.float32)
    f_st, f_df, f_32 = (str(tmp_path / n) for n in ("stored.npz", "deflated.npz", "f32.npz"))
    synth.write_amass_file(f_st, a, gender="female", fps=120.0, compressed=False)
    synth.write_amass_file(f_df, a, gender=np.bytes_(b"female"), fps=120.0, compressed=True)
    synth.write_amass_file(f_32, a32, gender=np.asarray(["male"]), fps=60, compressed=True)
    with pytest.raises(ValueError):  # what the joint-file parser makes of such an archive does not change: object members are refused there
        sa._zip_directory(memoryview(open(f_st, "rb").read()), f_st)
    got = [sa.read_amass_file(f) for f in (f_st, f_df, f_32)]
    for g, want, gender, fps in ((got[0], a, "female", 120.0), (got[1], a, "female", 120.0), (got[2], a32, "male", 60.0)):
        for key in ("root_orient", "pose_body", "trans"):
            assert g[key].dtype == want[key].dtype and np.array_equal(g[key], want[key])
        assert np.array_equal(g["betas"], want["betas"]) and g["gender"] == gender and g["mocap_frame_rate"] == fps
    st = sa.read_amass_members([f_st, f_df, f_32], _host_alloc, threads=3)
    assert st.files == [f_st, f_df, f_32] and [m["T"] for m in st.parsed] == [37, 37, 12] and not st.skipped
    assert all(int(s) % 256 == 0 for s in st.starts) and all(m["arrays"][k]["off"] % 64 == 0 for m in st.parsed for k in m["arrays"])
    assert abs(st.parsed[0]["height"] - (1.66 + 0.1 * a["betas"][0])) < 1e-15
    # the bytes staged are the three arrays', not the archives' (poses, pose_hand ... stay on the disk): per member its numbers, at most a
    # 128-byte .npy header (deflated members) and 64 bytes of alignment; 256 per file
    assert st.total < 3 * 256 + (64 + 128) * 9 + sum(w[k].nbytes for w in (a, a, a32) for k in ("root_orient", "pose_body", "trans")) + 1

    bad = {}
    raw = open(f_st, "rb").read()
    bad["truncated"] = str(tmp_path / "truncated.npz")
    open(bad["truncated"], "wb").write(raw[: len(raw) // 2])
    bad["nopose"] = str(tmp_path / "nopose.npz")
    np.savez(bad["nopose"], **{k: v for k, v in a.items() if k != "pose_body"}, gender="male", mocap_frame_rate=120.0)
    for comp in (False, True):
        bad[f"tmis{comp}"] = str(tmp_path / f"tmis{comp}.npz")
        synth.write_amass_file(bad[f"tmis{comp}"], dict(a, trans=a["trans"][:-1]), compressed=comp)
    bad["fps"] = str(tmp_path / "fps.npz")
    synth.write_amass_file(bad["fps"], a, fps=0.0)
    bad["shape"] = str(tmp_path / "shape.npz")
    synth.write_amass_file(bad["shape"], dict(a, pose_body=a["pose_body"][:, :60]), compressed=True)
    bad["gender"] = str(tmp_path / "gender.npz")
    synth.write_amass_file(bad["gender"], a, gender=np.asarray(["male", "female"]))
    bad["notzip"] = str(tmp_path / "notzip.npz")
    open(bad["notzip"], "wb").write(b"\x93NUMPY" + bytes(200))
    for name, f in bad.items():
        with pytest.raises(ValueError):
            sa.read_amass_members([f], _host_alloc)
    files = [f_st] + list(bad.values()) + [str(tmp_path / "missing.npz"), f_32]
    st = sa.read_amass_members(files, _host_alloc, threads=4, skip_errors=True)
    assert st.files == [f_st, f_32] and [f for f, _ in st.skipped] == files[1:-1]
    m = st.parsed[1]["arrays"]["pose_body"]
    assert np.array_equal(np.frombuffer(st.buf.numpy(), dtype=np.float32, count=12 * 63, offset=int(st.starts[1]) + m["off"]).reshape(12, 63), a32["pose_body"])
    with pytest.raises(FileNotFoundError):
        sa.read_amass_members([str(tmp_path / "missing.npz")], _host_alloc)
    # load_joint_files' own rules are untouched: it still wants stored members
    jf = str(tmp_path / "joint.npz")
    np.savez_compressed(jf, joints=np.zeros((2, 55, 3)), global_orient=np.zeros((2, 3)), full_pose=np.zeros((2, 165)), mocap_frame_rate=30.0, betas=np.zeros(16))
    with pytest.raises(ValueError, match="compressed"):
        sa._joint_meta(memoryview(open(jf, "rb").read()), jf, 55)


def test_script_flags_leave_the_joint_file_run_as_it_is(tmp_path, monkeypatch):
    """H4: without --smplx_model_folder the script plans the same files with the same extension and asks iter_joint_batches for them;
    with it, the same plan goes to iter_amass_batches together with the folder and --num_betas."""
    from gmr_amd.scripts import _walk, smplx_to_robot_dataset
    src, tgt = tmp_path / "in", tmp_path / "out"
    (src / "sub").mkdir(parents=True)
    for n in ("b10.npz", "b2.npz", "x_stagei.npz", "walk_crawl.npz", "notes.txt", os.path.join("sub", "c.npz")):
        (src / n).write_bytes(b"")
    seen = {}

    def fake_convert(args, pairs, src_human, batches, retarget_kw, workers, done):
        seen["pairs"], seen["args"] = pairs, args
        seen["batches"] = batches([s for s, _ in pairs], ["pelvis"])
        return 0
    calls = []
    monkeypatch.setattr(smplx_to_robot_dataset, "convert", fake_convert)
    monkeypatch.setattr(sa, "iter_joint_batches", lambda files, **kw: calls.append(("joint", files, kw)) or "J")
    monkeypatch.setattr(sa, "iter_amass_batches", lambda files, models, **kw: calls.append(("amass", files, models, kw)) or "A")
    base = ["--src_folder", str(src), "--tgt_folder", str(tgt), "--hard_motions"]
    assert smplx_to_robot_dataset.main(base) == 0
    want = [(str(src / "b2.npz"), str(tgt / "b2.pkl")), (str(src / "b10.npz"), str(tgt / "b10.pkl")), (str(src / "sub" / "c.npz"), str(tgt / "sub" / "c.pkl"))]
    assert seen["pairs"] == want and seen["batches"] == "J" and seen["args"].smplx_model_folder is None and seen["args"].num_betas is None
    assert calls[-1][0] == "joint" and calls[-1][1] == [s for s, _ in want]
    assert calls[-1][2] == dict(batch_files=1024, device=None, threads=4, columns=["pelvis"], skip_errors=True)
    assert smplx_to_robot_dataset.main(base + ["--smplx_model_folder", "/models", "--num_betas", "10", "--robots", "unitree_g1,booster_t1"]) == 0
    assert seen["batches"] == "A" and calls[-1][0] == "amass" and calls[-1][1] == [s for s, _ in want] and calls[-1][2] == "/models"
    assert calls[-1][3] == dict(batch_files=1024, device=None, threads=4, columns=["pelvis"], skip_errors=True, num_betas=10)
    assert seen["pairs"][0][1] == (str(tgt / "unitree_g1" / "b2.pkl"), str(tgt / "booster_t1" / "b2.pkl"))

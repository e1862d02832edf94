"""The dataset scripts' self-collision flags end to end (the pattern of tests/test_gpu_clip_report.py's script test): two short clips
give two CSV rows that are the class method's report of the solved qpos, and --max_penetration moves the deeper clip to --hard_out."""
import csv
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gmr_amd import synth  # noqa: E402
from tests.util import compiled  # noqa: E402

RADIUS = 0.06   # fat enough that the synthetic motion penetrates, the two clips by different depths (asserted below)


def test_collision_csv_rows_and_max_penetration_moves_a_clip_to_the_hard_list(tmp_path):
    from gmr_amd import GeneralMotionRetargeting, dataset
    from gmr_amd.scripts import smplx_to_robot_dataset
    from gmr_amd.scripts._walk import hard_motion_names
    cm = compiled("smplx", "unitree_g1")
    pos, quat, names, offs, _ = synth.synth_clips(cm, 2, 24, seed=12, hard=False, dtype=np.float64)
    offs = np.asarray(offs, dtype=np.int64)
    src = str(tmp_path / "in")
    os.makedirs(src)
    synth.write_smplx_joint_files(src, torch.from_numpy(pos), torch.from_numpy(quat), names, offs, fps=30.0)
    files = sorted(os.listdir(src))
    assert len(files) == 2
    base = ["--src_folder", src, "--num_cpus", "2", "--hard_motions", "--collision_radius", repr(RADIUS)]
    plain, csv_path, hard_path = str(tmp_path / "plain"), str(tmp_path / "rep" / "col.csv"), str(tmp_path / "rep" / "hard.txt")
    os.makedirs(os.path.dirname(csv_path))
    assert smplx_to_robot_dataset.main(base + ["--tgt_folder", plain, "--collision_csv", csv_path]) == 0
    assert sorted(os.listdir(plain)) == [f.replace(".npz", ".pkl") for f in files]     # nothing withheld without a bound
    with open(csv_path, newline="") as f:
        rows = list(csv.DictReader(f))
    assert [r["clip"] for r in rows] == [f.split(".")[0] for f in files]
    assert list(rows[0]) == ["clip", *dataset.COLLISION_CSV_FIELDS, "worst_capsule_a", "worst_capsule_b"]
    g = GeneralMotionRetargeting("smplx", "unitree_g1", verbose=False)
    capsule_names = g._engine.default_proxies(RADIUS)[0].names
    for r in rows:   # (the script solves the files as it loads them: the rows are checked for what they must satisfy among themselves)
        assert float(r["penetration_max"]) == max(0.0, -float(r["clearance_min"])) and 0 <= int(r["worst_frame"]) < 24
        assert r["worst_capsule_a"] in capsule_names and r["worst_capsule_b"] in capsule_names and r["worst_capsule_a"] != r["worst_capsule_b"]
        assert int(r["longest_run"]) <= int(r["colliding_frames"]) <= 24 and int(r["hits_sum"]) >= int(r["colliding_frames"]) and r["nonfinite_frames"] == "0"
        assert (int(r["colliding_frames"]) > 0) == (float(r["clearance_min"]) < 0.0)
    # retarget_clips(collision=...) appends the class method's report of the qpos it solved
    motions, col = dataset.retarget_clips(g, pos, quat, names, offs, collision={"radius": RADIUS})
    q = g.retarget_batch(torch.from_numpy(pos).to(g.device), torch.from_numpy(quat).to(g.device), names, seq_offsets=offs)
    rep = g.self_collision_report(q, offs, radius=RADIUS)
    assert len(motions) == 2 and sorted(col) == sorted(rep)
    for k in rep:
        assert np.array_equal(np.asarray(col[k]), np.asarray(rep[k])), k
    pen = [float(r["penetration_max"]) for r in rows]
    assert max(pen) > 0.0 and abs(pen[0] - pen[1]) > 1e-6, pen
    deep = int(np.argmax(pen))
    out = str(tmp_path / "out")
    assert smplx_to_robot_dataset.main(base + ["--tgt_folder", out, "--hard_out", hard_path, "--max_penetration", repr(0.5 * (pen[0] + pen[1]))]) == 0
    assert os.listdir(out) == [files[1 - deep].replace(".npz", ".pkl")]
    assert hard_motion_names([hard_path]) == [files[deep].split(".")[0]]
    for f in os.listdir(out):   # what is written is what the plain run writes
        assert open(os.path.join(out, f), "rb").read() == open(os.path.join(plain, f), "rb").read()

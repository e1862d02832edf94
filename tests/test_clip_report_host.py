"""The per-clip quality report, the parts that need no GPU: the two exports and their ctypes layout, the host segment planner,
the CSV and hard-list writers, and the report flags of the dataset scripts."""
import argparse
import csv
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gmr_clip_report", "gmr_group_clip_report")


def test_clip_report_exports_are_declared_and_bound():
    from gmr_amd import _native, engine
    from gmr_amd.build import build_lib
    build_lib()
    with open(os.path.join(ROOT, "include", "gmr_amd.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bint\s+gmr_clip_report\s*\(gmr_model \*m, const gmr_clip_report_input \*in,\s*const gmr_clip_report_params \*prm, void \*stream\)", src)
    assert re.search(r"\bint\s+gmr_group_clip_report\s*\(gmr_group \*g, const gmr_clip_report_input \*inputs,\s*const gmr_clip_report_params \*prm, void \*stream\)", src)
    assert re.search(r"#define GMR_ABI_VERSION 5\b", src)
    seg = re.search(r"#define GMR_CLIP_REPORT_SEGMENT (\d+)\b", src)
    eps = re.search(r"#define GMR_CLIP_REPORT_LIMIT_EPS (\S+)", src)
    assert seg and int(seg.group(1)) == _native.CLIP_REPORT_SEGMENT == engine.CLIP_REPORT_SEGMENT
    assert eps and float(eps.group(1)) == _native.CLIP_REPORT_LIMIT_EPS == engine.CLIP_REPORT_LIMIT_EPS
    for name in NEW:
        assert name in _native.EXPORTS
    lib = _native.load()
    assert lib.gmr_abi_version() == 5
    # null handles are refused before anything else (no device needed)
    ri, prm = _native.ClipReportInput(), _native.ClipReportParams()
    assert lib.gmr_clip_report(None, ctypes.byref(ri), ctypes.byref(prm), None) == -1
    assert lib.gmr_group_clip_report(None, ctypes.byref(ri), ctypes.byref(prm), None) == -1


def test_clip_report_layouts_match_the_c_structs():
    """ctypes.sizeof / offsets against the structs as a C compiler lays them out (x86-64 SysV, like the library)."""
    from gmr_amd import _native
    R = _native.ClipReportInput
    assert ctypes.sizeof(R) == 192
    want = {"qpos": 0, "n_frames": 8, "human_pos": 16, "human_quat": 24, "in_dtype": 32, "n_cols": 36, "slot_col": 40, "seq_offsets": 48,
            "n_seq": 56, "reserved": 60, "height_scale": 64, "iters": 72, "err_max_out": 80, "err_sum_out": 88, "task_pos_max_out": 96,
            "task_pos_sum_out": 104, "task_rot_max_out": 112, "task_rot_sum_out": 120, "near_lo_out": 128, "near_hi_out": 136,
            "dof_step_max_out": 144, "root_step_max_out": 152, "root_turn_max_out": 160, "solves_max_out": 168, "solves_sum_out": 176,
            "nonfinite_frames_out": 184}
    assert [n for n, _ in R._fields_] == list(want)
    for k, off in want.items():
        assert getattr(R, k).offset == off, k
    P = _native.ClipReportParams
    assert ctypes.sizeof(P) == 16
    assert (P.limit_eps.offset, P.segment_frames.offset, P.offset_to_ground.offset) == (0, 8, 12)
    # the header declares the members in this order
    with open(os.path.join(ROOT, "include", "gmr_amd.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    body = re.search(r"typedef struct gmr_clip_report_input \{(.*?)\} gmr_clip_report_input;", src, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", body)
    assert names == list(want)


def _check_segments(offs, segment):
    from gmr_amd.schedule import report_segments
    offs = np.asarray(offs, dtype=np.int64)
    seg = report_segments(offs, segment)
    assert seg.dtype == np.int64 and seg.ndim == 2 and seg.shape[1] == 3
    cover = np.zeros(int(offs[-1]), dtype=np.int64)
    for clip, a, b in seg:
        assert 0 < b - a <= segment
        assert offs[clip] <= a and b <= offs[clip + 1]  # inside one clip
        assert (a - offs[clip]) % segment == 0
        cover[a:b] += 1
    assert (cover == 1).all()  # every frame in exactly one segment
    for s in range(len(offs) - 1):
        mine = seg[seg[:, 0] == s]
        assert len(mine) == -(-(offs[s + 1] - offs[s]) // segment)  # empty clips give none
        assert (np.diff(mine[:, 1]) > 0).all()  # ascending inside a clip
    assert (np.diff(seg[:, 0]) >= 0).all()  # clip by clip
    return seg


def test_report_segments():
    from gmr_amd.schedule import report_segments
    seg = _check_segments([0, 0, 1, 3, 7, 11, 12, 21], 4)
    assert seg.tolist() == [[1, 0, 1], [2, 1, 3], [3, 3, 7], [4, 7, 11], [5, 11, 12], [6, 12, 16], [6, 16, 20], [6, 20, 21]]
    rng = np.random.default_rng(7)
    for _ in range(50):
        lens = rng.integers(0, 40, size=int(rng.integers(1, 12))) * (rng.random(1) < 0.9)
        _check_segments(np.concatenate([[0], np.cumsum(lens)]), int(rng.integers(1, 70)))
    assert report_segments([0], 4).shape == (0, 3) and report_segments([0, 0, 0], 4).shape == (0, 3)
    with pytest.raises(ValueError):
        report_segments([0, 5, 3], 4)
    with pytest.raises(ValueError):
        report_segments([0, 5], 0)


def _hand_report():
    from gmr_amd.engine import ClipReport
    f = np.array([3, 0, 5])
    return ClipReport(
        f, ["1:pelvis", "1:left_hand", "2:pelvis"], ["hip", "knee"], (True, True),
        err_max=np.array([[0.5, 0.25], [0.0, 0.0], [1.5, 2.125]]), err_sum=np.array([[0.9, 0.6], [0.0, 0.0], [5.0, 2.5]]),
        task_pos_max=np.array([[0.01, 0.02, 0.03], [0, 0, 0], [0.4, 0.05, 0.06]]), task_pos_sum=np.zeros((3, 3)),
        task_rot_max=np.array([[0.1, 0.2, 0.3], [0, 0, 0], [0.7, 0.8, 0.9]]), task_rot_sum=np.zeros((3, 3)),
        near_lo=np.array([[1, 0], [0, 0], [0, 4]], dtype=np.int32), near_hi=np.array([[0, 2], [0, 0], [0, 0]], dtype=np.int32),
        dof_step_max=np.array([[0.1, 0.2], [0, 0], [0.05, 3.0]]), root_step_max=np.array([0.01, 0, 0.02]),
        root_turn_max=np.array([0.1, 0, 0.2]), solves_max=np.array([2, 0, 7], dtype=np.int32),
        solves_sum=np.array([6, 0, 20], dtype=np.int64), nonfinite_frames=np.array([0, 0, 1], dtype=np.int32))


def test_clip_report_means():
    r = _hand_report()
    assert len(r) == 3 and r.last_table == 1
    m = r.err_mean
    assert np.allclose(m[0], [0.3, 0.2]) and np.isnan(m[1]).all() and np.allclose(m[2], [1.0, 0.5])
    assert np.isnan(r.solves_mean[1]) and r.solves_mean[0] == 2.0 and r.solves_mean[2] == 4.0
    assert r.task_pos_mean.shape == (3, 3) and np.isnan(r.task_pos_mean[1]).all()


def test_report_csv(tmp_path):
    from gmr_amd import dataset
    r = _hand_report()
    path = str(tmp_path / "sub" / "report.csv")
    dataset.write_report_csv(path, ["a", "b", "c"], r)
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    head = rows[0]
    assert len(rows) == 4 and head[:2] == ["clip", "frames"]
    for col in ("err1_max", "err2_max", "err1_mean", "root_step_max", "root_turn_max", "solves_max", "solves_sum", "nonfinite_frames",
                "1:pelvis:pos_max", "1:left_hand:pos_max", "2:pelvis:rot_max", "hip:step_max", "knee:near_lo", "knee:near_hi"):
        assert col in head, col
    c = {k: [row[i] for row in rows[1:]] for i, k in enumerate(head)}
    assert c["clip"] == ["a", "b", "c"] and c["frames"] == ["3", "0", "5"]
    assert [float(v) for v in c["err2_max"]] == [0.25, 0.0, 2.125]
    assert float(c["1:pelvis:pos_max"][2]) == 0.4 and float(c["knee:step_max"][2]) == 3.0
    assert c["knee:near_lo"] == ["0", "0", "4"] and c["nonfinite_frames"] == ["0", "0", "1"]
    assert c["err1_mean"][1] == "nan"
    with pytest.raises(ValueError):
        dataset.write_report_csv(path, ["a"], r)


def test_hard_list_round_trips_through_the_scripts_reader(tmp_path):
    from gmr_amd import dataset
    from gmr_amd.scripts._walk import hard_motion_names
    r = _hand_report()
    assert dataset.report_difficulty(r).tolist() == [0.25, 0.0, 2.125]  # err_max of the last used table
    assert dataset.report_hard_mask(r).tolist() == [False, False, False]
    assert dataset.report_hard_mask(r, max_pos_err=0.1).tolist() == [False, False, True]
    assert dataset.report_hard_mask(r, max_dof_step=0.15).tolist() == [True, False, True]
    assert dataset.report_hard_mask(r, max_pos_err=1.0, max_dof_step=5.0).tolist() == [False, False, False]
    path = str(tmp_path / "hard.txt")
    n = dataset.write_hard_list(path, ["walk_01", "empty", "flip_02"], r, [True, False, True])
    assert n == 2
    with open(path) as f:
        assert f.read() == "Motion: walk_01.pkl, Difficulty: 0.25\nMotion: flip_02.pkl, Difficulty: 2.12\n"
    assert hard_motion_names([path]) == ["walk_01", "flip_02"]
    dataset.write_hard_list(path, ["x"], _one(r), [True], append=True)
    assert hard_motion_names([path]) == ["walk_01", "flip_02", "x"]
    # table 2 unused: the difficulty is table 1's error
    r.tables_used = (True, False)
    assert dataset.report_difficulty(r).tolist() == [0.5, 0.0, 1.5]


def _one(r):
    from gmr_amd.engine import ClipReport
    return ClipReport(r.frames[:1], r.task_names, r.hinge_names, r.tables_used, err_max=r.err_max[:1], dof_step_max=r.dof_step_max[:1])


def _parser():
    from gmr_amd.scripts._walk import add_common_flags
    ap = argparse.ArgumentParser()
    ap.add_argument("--robot", default=None)
    add_common_flags(ap)
    return ap


def test_report_flags_parse_and_default_to_off():
    from gmr_amd.scripts._walk import wants_report
    args = _parser().parse_args([])
    assert (args.report_csv, args.hard_out, args.max_pos_err, args.max_dof_step) == (None, None, None, None)
    assert not wants_report(args)
    args = _parser().parse_args(["--report_csv", "r.csv", "--hard_out", "h.txt", "--max_pos_err", "0.3", "--max_dof_step", "1.5", "--robots", "a,b"])
    assert (args.report_csv, args.hard_out, args.max_pos_err, args.max_dof_step) == ("r.csv", "h.txt", 0.3, 1.5)
    assert wants_report(args)
    for flag, val in (("--report_csv", "r.csv"), ("--hard_out", "h"), ("--max_pos_err", "1"), ("--max_dof_step", "1")):
        assert wants_report(_parser().parse_args([flag, val]))


def test_plan_is_unchanged_by_the_report_flags(tmp_path):
    from gmr_amd.scripts._walk import plan, resolve_robots
    src, tgt = tmp_path / "src", tmp_path / "tgt"
    (src / "d").mkdir(parents=True)
    for n in ("a.bvh", "d/b.bvh", "d/c.txt"):
        (src / n).write_text("x")

    def planned(extra):
        ap = _parser()
        ap.add_argument("--src_folder")
        ap.add_argument("--tgt_folder")
        args = ap.parse_args(["--src_folder", str(src), "--tgt_folder", str(tgt)] + extra)
        resolve_robots(ap, args)
        return plan(args, ".bvh", lambda n: n.endswith(".bvh"))

    flags = ["--report_csv", str(tmp_path / "r.csv"), "--hard_out", str(tmp_path / "h.txt"), "--max_pos_err", "0.3", "--max_dof_step", "2"]
    assert planned([]) == planned(flags)
    assert len(planned([])[0]) == 2
    assert planned(["--robots", "unitree_g1,booster_t1"]) == planned(["--robots", "unitree_g1,booster_t1"] + flags)


def test_report_sink_withholds_and_lists(tmp_path):
    """The scripts' per-batch step, on a hand-made report: clips over a bound are not written and are listed."""
    from gmr_amd import dataset
    from gmr_amd.scripts._walk import ReportSink, hard_motion_names
    args = _parser().parse_args(["--report_csv", str(tmp_path / "r.csv"), "--hard_out", str(tmp_path / "h.txt"), "--max_dof_step", "1.0"])
    sink = ReportSink(args)
    r = _hand_report()
    motions, targets = sink.take(dataset, ["/o/a.pkl", "/o/b.pkl", "/o/c.pkl"], ["ma", "mb", "mc"], r)
    assert motions == ["ma", "mb"] and targets == ["/o/a.pkl", "/o/b.pkl"]
    motions, targets = sink.take(dataset, ["/o/d.pkl", "/o/e.pkl", "/o/f.pkl"], ["md", "me", "mf"], r)
    assert targets == ["/o/d.pkl", "/o/e.pkl"]
    with open(args.report_csv, newline="") as f:
        assert [row[0] for row in csv.reader(f)] == ["clip", "a", "b", "c", "d", "e", "f"]  # on disk batch by batch
    sink.close()
    assert hard_motion_names([args.hard_out]) == ["c", "f"]
    with open(args.report_csv, newline="") as f:
        rows = list(csv.reader(f))
    assert [row[0] for row in rows] == ["clip", "a", "b", "c", "d", "e", "f"]
    per_robot = ReportSink(_parser().parse_args(["--report_csv", "x/r.csv", "--hard_out", "h.txt"]), "unitree_g1")
    assert per_robot.csv == "x/r.unitree_g1.csv" and per_robot.hard == "h.unitree_g1.txt"
    per_rank = ReportSink(_parser().parse_args(["--report_csv", "x/r.csv", "--hard_out", "h.txt"]), "unitree_g1", rank=3)
    assert per_rank.csv == "x/r.unitree_g1.rank3.csv" and per_rank.hard == "h.unitree_g1.rank3.txt"


def test_report_csv_appends_without_a_second_header(tmp_path):
    from gmr_amd import dataset
    r = _hand_report()
    path = str(tmp_path / "r.csv")
    dataset.write_report_csv(path, ["a", "b", "c"], r)
    dataset.write_report_csv(path, ["d", "e", "f"], r, append=True)
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    assert [row[0] for row in rows] == ["clip", "a", "b", "c", "d", "e", "f"] and rows[1][1:] == rows[4][1:]


def test_ranks_of_a_sharded_run_write_report_files_of_their_own(tmp_path, monkeypatch):
    """--shard_by_rank: every rank runs the same command line; rank k's hard list and CSV go to <stem>.rank<k><ext>, so a clip
    withheld on one rank stays listed whatever the other ranks write."""
    from gmr_amd import dataset
    from gmr_amd.scripts import _walk
    r = _hand_report()
    seen = {}

    class FakeGMR:
        ik_columns = ["x"]

        def __init__(self, **kw):
            pass

    class Batch:
        skipped, pos, quat, body_names, seq_offsets, human_heights = [], None, None, ["x"], [0, 3, 3, 8], None

        def __init__(self, files):
            self.files = files

        def __len__(self):
            return len(self.files)

    import gmr_amd
    monkeypatch.setattr(gmr_amd, "GeneralMotionRetargeting", FakeGMR)
    monkeypatch.setattr(dataset, "retarget_clips", lambda g, *a, report=False, **k: (["m0", "m1", "m2"], r))
    monkeypatch.setattr(dataset.MotionWriter, "submit", lambda self, motions, paths: seen.setdefault(os.environ["RANK"], []).extend(paths))
    pairs = [(f"/s/c{i}.npz", f"/t/c{i}.pkl") for i in range(6)]
    csv_path, hard_path = str(tmp_path / "r.csv"), str(tmp_path / "h.txt")
    monkeypatch.setenv("WORLD_SIZE", "2")
    for rank in ("0", "1"):
        monkeypatch.setenv("RANK", rank)
        args = _parser().parse_args(["--shard_by_rank", "--device", "0", "--report_csv", csv_path, "--hard_out", hard_path, "--max_dof_step", "1.0"])
        args.robot_list, args.robot, args.tgt_folder = None, "unitree_g1", "/t"
        assert _walk.convert(args, pairs, "smplx", lambda files, cols: [Batch(files)], lambda b: {}, 1, "done") == 0
    assert _walk.hard_motion_names([str(tmp_path / "h.rank0.txt")]) == ["c4"]  # clips 0, 2, 4 -> the third is over the bound
    assert _walk.hard_motion_names([str(tmp_path / "h.rank1.txt")]) == ["c5"]
    assert seen == {"0": ["/t/c0.pkl", "/t/c2.pkl"], "1": ["/t/c1.pkl", "/t/c3.pkl"]}
    for rank, names in (("0", ["c0", "c2", "c4"]), ("1", ["c1", "c3", "c5"])):
        with open(str(tmp_path / f"r.rank{rank}.csv"), newline="") as f:
            assert [row[0] for row in csv.reader(f)] == ["clip"] + names
    assert not os.path.exists(csv_path) and not os.path.exists(hard_path)

"""The contact labels without a GPU: the header, the export and the binding of gmr_motion_contacts, the layout of its struct, the
static stream check of its launch, the tiled bit-mask formulation of the label (tests/contact_reference.py) against the plain
loop, the .npz round trip of the new keys, and the flags of the dataset scripts."""
import ctypes as C
import os
import random
import re
import shutil
import subprocess
import zipfile

import numpy as np
import pytest

from tests import contact_reference as ref
from tests.test_stream_order_host import check_api, reachable, stream_prototypes, units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "gmr_amd.h")) as f:
        return f.read()


# ------------------------------------------------------------------ 1: header, export, binding
def test_symbol_is_declared_exported_and_bound():
    from gmr_amd import _native
    src = _header()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint gmr_motion_contacts\s*\(gmr_model \*m, const gmr_contact_input \*in\);", code)
    assert re.search(r"^#define GMR_CONTACT_GROUND_FIXED 0$", src, flags=re.M) and re.search(r"^#define GMR_CONTACT_GROUND_CLIP_MIN 1$", src, flags=re.M)
    assert (_native.CONTACT_GROUND_FIXED, _native.CONTACT_GROUND_CLIP_MIN) == (ref.GROUND_FIXED, ref.GROUND_CLIP_MIN) == (0, 1)
    assert "gmr_motion_contacts" in _native.EXPORTS
    assert re.search(r"^#define GMR_ABI_VERSION 5$", src, flags=re.M) and _native.ABI_VERSION == 5
    assert "gmr_motion_contacts" not in stream_prototypes() and len(stream_prototypes()) == 27  # the stream travels in the struct
    lib = _native.load()
    assert lib.gmr_abi_version() == 5
    assert lib.gmr_motion_contacts.restype == C.c_int and len(lib.gmr_motion_contacts.argtypes) == 2
    assert lib.gmr_motion_contacts.argtypes[1]._type_ is _native.ContactInput
    ci = _native.ContactInput()
    assert lib.gmr_motion_contacts(None, C.byref(ci)) == -1  # a null handle is refused before anything else (no device needed)
    assert _native.CONTACT_OUTPUTS == ref.FIELDS


def test_struct_layout_equals_the_c_compiler_and_the_listing_in_the_header(tmp_path):
    from gmr_amd import _native
    T = _native.ContactInput
    fields = [k for k, _ in T._fields_]
    src = _header()
    src = src[src[:src.index("typedef struct gmr_contact_input")].rindex("Layout (LP64)"):]   # (the listing nearest above the struct)
    m = re.match(r"Layout \(LP64\): sizeof (\d+); offsets (.*?)\.\s*\*/\s*#define GMR_CONTACT_GROUND_FIXED 0\s*#define GMR_CONTACT_GROUND_CLIP_MIN 1\s*"
                  r"typedef struct gmr_contact_input \{(.*?)\} gmr_contact_input;", src, flags=re.S)
    assert m, "the layout listing in front of gmr_contact_input"
    listing = {k: int(v) for k, v in re.findall(r"([a-z_0-9]+) (\d+)", re.sub(r"\s*\*\s*", " ", m.group(2)))}
    body = re.sub(r"/\*.*?\*/", "", m.group(3), flags=re.S)
    declared = []  # field names in declaration order
    for stmt in body.split(";"):
        declared += re.findall(r"\*?\s*([a-z_0-9]+)\s*(?:,|$)", stmt.strip())
    assert declared == fields
    assert C.sizeof(T) == int(m.group(1)) == 176
    assert listing == {k: getattr(T, k).offset for k in fields}
    assert fields[-8:] == [k + "_out" for k in _native.CONTACT_OUTPUTS] and fields[-9] == "stream"
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.skip("no C compiler")
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gmr_amd.h"\nint main(void) {\n'
                    '  printf("%zu", sizeof(gmr_contact_input));\n'
                    + "".join(f'  printf(" %zu", offsetof(gmr_contact_input, {n}));\n' for n in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", f"-I{ROOT}/include", str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert C.sizeof(T) == got[0]
    assert [getattr(T, n).offset for n in fields] == got[1:]


# ------------------------------------------------------------------ 2: the launch names the call's stream
def test_the_launch_is_on_the_structs_stream_and_nothing_synchronises():
    problems, syncs = check_api(entries=["gmr_motion_contacts"])
    assert not problems, "\n".join(problems)
    assert syncs == {"gmr_motion_contacts": False}
    us = units()
    r = reachable(us, "gmr_motion_contacts")
    assert "contact_run" in r and "scratch_alloc" not in r and "CallScratch" not in r   # no allocation
    launches = [len(re.findall(r"\bhipLaunchKernelGGL\s*\(", us[u])) for u in r]
    assert sum(launches) == 1 and len(re.findall(r"\bhipLaunchKernelGGL\s*\(", us["contact_run"])) == 1   # one kernel
    assert not any(re.search(r"\bhip\w+Async\s*\(", us[u]) for u in r)                                    # no copy
    assert "static_cast<hipStream_t>(in->stream)" in re.sub(r"\s+", "", us["gmr_motion_contacts"])


# ------------------------------------------------------------------ 3: the tiled bit-mask label
def test_tiled_masks_equal_the_loop_on_random_sequences():
    rnd = random.Random(7)
    lengths = set()
    for i in range(2000):
        n = rnd.randint(0, 200) if i >= 201 else i   # every length 0 .. 200 once, then random ones
        lengths.add(n)
        p_e, p_s = rnd.choice([0.02, 0.1, 0.5]), rnd.choice([0.5, 0.9, 0.98])
        enter = [rnd.random() < p_e for _ in range(n)]
        stay = [e or rnd.random() < p_s for e in enter]   # enter implies stay
        assert ref.labels_tiled(enter, stay) == ref.labels_loop(enter, stay), (i, n)
    assert lengths == set(range(201))


def _seq(n, enters=(), leaves=()):
    enter = [k in enters for k in range(n)]
    stay = [k not in leaves for k in range(n)]
    return enter, stay


def test_tiled_masks_on_the_tile_edges():
    # the decisive frame on lane 63: everything behind it, across the edge, follows it
    e, s = _seq(130, enters=[63])
    assert ref.labels_tiled(e, s) == ref.labels_loop(e, s) == [0] * 63 + [1] * 67
    e, s = _seq(130, enters=[0], leaves=[63])
    assert ref.labels_tiled(e, s) == ref.labels_loop(e, s) == [1] * 63 + [0] * 67
    # ... or on lane 0 of the next tile
    e, s = _seq(130, enters=[64])
    assert ref.labels_tiled(e, s) == ref.labels_loop(e, s) == [0] * 64 + [1] * 66
    e, s = _seq(130, enters=[5], leaves=[64])
    assert ref.labels_tiled(e, s) == ref.labels_loop(e, s) == [0] * 5 + [1] * 59 + [0] * 66
    # an undecided run spanning two whole tiles: the carry passes through both untouched
    e, s = _seq(64 * 4, enters=[60], leaves=[64 * 3 + 1])
    want = [0] * 60 + [1] * (64 * 3 + 1 - 60) + [0] * 63
    assert ref.labels_tiled(e, s) == ref.labels_loop(e, s) == want
    e, s = _seq(64 * 4, enters=[10, 64 * 3 + 2], leaves=[63])
    want = [0] * 10 + [1] * 53 + [0] * (64 * 3 + 2 - 63) + [1] * 62
    assert ref.labels_tiled(e, s) == ref.labels_loop(e, s) == want
    # both at once: entering wins (the contract's order), in both formulations
    assert ref.labels_tiled([True], [False]) == ref.labels_loop([True], [False]) == [1]
    assert ref.labels_tiled([], []) == ref.labels_loop([], []) == []


def test_reference_on_a_hand_computed_clip():
    """Two bodies of a three-body model over five frames, fixed ground at 0: the statistics by hand."""
    pos = np.zeros((5, 3, 3), np.float32)
    vel = np.zeros((5, 3, 3), np.float32)
    pos[:, 2, 2] = [0.0, 0.0, 0.0, 0.5, -0.25]      # body 2: down, down, down, up, below the ground
    pos[:, 2, 0] = [0.0, 0.25, 0.25, 0.25, 0.25]    # slides 0.25 in frame 1
    pos[:, 2, 1] = [0.0, 0.0, 0.5, 0.5, 0.5]        # and 0.5 in frame 2
    pos[:, 0, 2] = 1.0                              # body 0: never down
    r = ref.contacts(pos, vel, [0, 5], [2, 0], None, ref.GROUND_FIXED, 0.0, 2.0 ** -5, 2.0 ** -4, 0.25, 0.5)
    assert r["contact"].tolist() == [[1, 0], [1, 0], [1, 0], [0, 0], [1, 0]]
    assert r["frames"].tolist() == [[4, 0]] and r["touchdowns"].tolist() == [[2, 0]] and r["airborne_frames"].tolist() == [1]
    assert r["slide_sum"].tolist() == [[0.75, 0.0]] and r["slide_step_max"].tolist() == [[0.5, 0.0]]
    assert r["depth_max"].tolist() == [[0.25, 0.0]] and r["base"].tolist() == [0.0]
    m = ref.contacts(pos, vel, [0, 5], [2, 0], [0.0, 1.5], ref.GROUND_CLIP_MIN, 0.0, 2.0 ** -5, 2.0 ** -4, 0.25, 0.5)
    assert m["base"].tolist() == [-0.5] and m["contact"][:, 1].tolist() == [1] * 5 and m["contact"][:, 0].tolist() == [0] * 5
    pos[3, 0, 2] = np.nan
    assert np.isnan(ref.contacts(pos, vel, [0, 5], [2, 0], None, ref.GROUND_CLIP_MIN, 0.0, 2.0 ** -5, 2.0 ** -4, 0.25, 0.5)["base"][0])
    assert np.isnan(ref.contacts(pos, vel, [0, 0], [2, 0], None, ref.GROUND_CLIP_MIN, 0.0, 2.0 ** -5, 2.0 ** -4, 0.25, 0.5)["base"][0])


# ------------------------------------------------------------------ 4: the .npz round trip
def _fake_track(M=7, nd=5, nb=3, seed=0):
    from gmr_amd import dataset
    rng = np.random.default_rng(seed)
    shapes = {"joint_pos": (M, nd), "joint_vel": (M, nd), "root_pos": (M, 3), "root_rot": (M, 4), "root_lin_vel": (M, 3),
              "root_ang_vel": (M, 3), "body_pos_w": (M, nb, 3), "body_quat_w": (M, nb, 4), "body_lin_vel_w": (M, nb, 3),
              "body_ang_vel_w": (M, nb, 3)}
    assert tuple(shapes) == dataset.TRACK_ARRAYS
    d = {"fps": 50.0}
    for k, sh in shapes.items():
        d[k] = rng.normal(size=sh).astype(np.float32 if k.startswith("body_") else np.float64)
    d.update(body_names=[f"b{i}" for i in range(nb)], joint_names=[f"joint_{i}" for i in range(nd)], quat_order="xyzw")
    return d


def _save_tracking_as_it_was(path, track):
    """The writer of dataset.save_tracking as it stood before the contact keys existed, statement for statement."""
    from gmr_amd.dataset import TRACK_ARRAYS
    with open(path, "wb") as f:
        np.savez(f, fps=np.float64(track["fps"]), body_names=np.asarray(list(track["body_names"]), dtype=np.str_),
                 joint_names=np.asarray(list(track["joint_names"]), dtype=np.str_), quat_order=np.asarray(track["quat_order"]),
                 **{k: track[k] for k in TRACK_ARRAYS})


def test_save_and_load_tracking_round_trip_the_contact_keys(tmp_path, monkeypatch):
    from gmr_amd import dataset
    assert dataset.CONTACT_STATS == ("frames", "touchdowns", "slide_sum", "slide_step_max", "depth_max", "base")
    plain = _fake_track()
    rng = np.random.default_rng(3)
    d = dict(plain)
    stats = {"frames": np.array([4, 0], np.int32), "touchdowns": np.array([2, 0], np.int32), "slide_sum": rng.random(2),
             "slide_step_max": rng.random(2), "depth_max": rng.random(2), "base": np.float64(-0.125)}
    d.update(contact=rng.integers(0, 2, (7, 2)).astype(np.uint8), contact_body_names=["b2", "b0"], contact_stats=stats, airborne_frames=3)
    p = str(tmp_path / "with.npz")
    assert dataset.save_tracking(p, d) is True
    got = dataset.load_tracking(p)
    assert set(got) == set(d)
    for k in dataset.TRACK_ARRAYS:
        assert np.array_equal(got[k], d[k]) and got[k].dtype == d[k].dtype
    assert got["contact"].dtype == np.uint8 and np.array_equal(got["contact"], d["contact"])
    assert got["contact_body_names"] == ["b2", "b0"] and got["airborne_frames"] == 3 and isinstance(got["airborne_frames"], int)
    assert set(got["contact_stats"]) == set(dataset.CONTACT_STATS)
    for k, v in stats.items():
        assert np.array_equal(got["contact_stats"][k], v) and got["contact_stats"][k].dtype == np.asarray(v).dtype, k
    with np.load(p) as z:  # uncompressed, nothing that needs pickle, the old members first and in their old order
        assert all(info.compress_type == 0 for info in z.zip.infolist())
        assert z.files[:14] == ["fps", "body_names", "joint_names", "quat_order"] + list(dataset.TRACK_ARRAYS)
    # without the keys: the file the writer always wrote, byte for byte (the zip's member times held still for the comparison)
    fixed = zipfile.time.localtime(1_700_000_000)
    monkeypatch.setattr(zipfile.time, "localtime", lambda *a: fixed)
    p_new, p_old = str(tmp_path / "new.npz"), str(tmp_path / "old.npz")
    assert dataset.save_tracking(p_new, plain) is True
    _save_tracking_as_it_was(p_old, plain)
    with open(p_new, "rb") as f, open(p_old, "rb") as g:
        a, b = f.read(), g.read()
    assert a == b and len(a) > 1000
    assert set(dataset.load_tracking(p_new)) == set(plain)
    monkeypatch.undo()
    with open(p, "rb") as f:
        assert f.read() != a


def test_contact_body_ids_names_the_models_bodies():
    from gmr_amd import dataset
    names = ["pelvis", "left_foot", "right_foot"]
    assert dataset.contact_body_ids(names, ["right_foot", "left_foot"]) == [2, 1]
    with pytest.raises(KeyError) as e:
        dataset.contact_body_ids(names, ["left_foot", "left_toe"])
    assert "left_toe" in str(e.value) and all(n in str(e.value) for n in names)
    prm = dataset.ContactParams()
    assert (prm.height_on, prm.height_off, prm.speed_on, prm.speed_off, prm.ground, prm.height_offset) == (0.03, 0.05, 0.3, 0.6, "clip_min", None)


# ------------------------------------------------------------------ 5: the scripts' flags
@pytest.mark.parametrize("script", ["bvh_to_robot_dataset", "smplx_to_robot_dataset"])
def test_dataset_scripts_validate_the_contact_flags(script, tmp_path, capsys):
    import importlib
    mod = importlib.import_module("gmr_amd.scripts." + script)
    src, tgt, trk = str(tmp_path / "in"), str(tmp_path / "out"), str(tmp_path / "trk")
    os.makedirs(src)
    base = ["--src_folder", src, "--tgt_folder", tgt] + (["--hard_motions"] if script.startswith("smplx") else [])
    track = ["--track_fps", "50", "--track_folder", trk]
    feet = "left_ankle_roll_link,right_ankle_roll_link"
    # accepted (an empty folder: nothing to convert, no device touched)
    assert mod.main(base + track + ["--contact_bodies", feet]) == 0
    assert mod.main(base + track + ["--contact_bodies", feet, "--contact_height_on", "0.02", "--contact_height_off", "0.04",
                                    "--contact_speed_on", "0.2", "--contact_speed_off", "0.5"]) == 0
    assert mod.main(base + track + ["--robots", "unitree_g1,booster_t1", "--contact_bodies",
                                    "unitree_g1:" + feet + ";booster_t1:left_foot_link,right_foot_link"]) == 0
    assert mod.main(base + track + ["--robots", "unitree_g1,booster_t1", "--contact_bodies", "booster_t1:left_foot_link"]) == 0
    assert mod.main(base + track) == 0
    bad = [(["--contact_bodies", feet], "--track_fps"),                                        # only with --track_fps
           (track + ["--contact_height_on", "0.02"], "--contact_bodies"),                      # a threshold without bodies
           (track + ["--contact_bodies", " , "], "--contact_bodies"),
           (track + ["--contact_bodies", "unitree_g1:" + feet], "--robots"),                   # the --robots form without --robots
           (track + ["--robots", "unitree_g1,booster_t1", "--contact_bodies", feet], "robot:a,b"),
           (track + ["--robots", "unitree_g1,booster_t1", "--contact_bodies", "fourier_n1:a"], "robot:a,b"),
           (track + ["--robots", "unitree_g1,booster_t1", "--contact_bodies", "unitree_g1:a;unitree_g1:b"], "robot:a,b"),
           (track + ["--contact_bodies", feet, "--contact_height_on", "0.06"], "--contact_height_on"),   # above the default off
           (track + ["--contact_bodies", feet, "--contact_speed_on", "-0.1"], "--contact_speed_on")]
    for flags, word in bad:
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            mod.main(base + flags)
        assert e.value.code == 2 and word in capsys.readouterr().err, flags


def test_contact_flags_become_the_arguments_of_retarget_clips():
    import argparse
    from gmr_amd.scripts import _walk
    ap = argparse.ArgumentParser()
    _walk.add_common_flags(ap)
    none = ap.parse_args([])
    none.robot_list = None
    _walk.resolve_track(ap, none)
    assert none.contact_bodies is None and none.contact_kw == {}   # without the flag nothing is passed on
    args = ap.parse_args(["--track_fps", "50", "--track_folder", "/trk", "--contact_bodies", "a, b", "--contact_speed_off", "0.75"])
    args.robot_list = None
    _walk.resolve_track(ap, args)
    assert args.contact_kw["contact_bodies"] == ["a", "b"]
    prm = args.contact_kw["contact"]
    assert (prm.height_on, prm.height_off, prm.speed_on, prm.speed_off, prm.ground) == (0.03, 0.05, 0.3, 0.75, "clip_min")
    args = ap.parse_args(["--track_fps", "50", "--track_folder", "/trk", "--robots", "r1,r2", "--contact_bodies", "r2:c,d; r1:a"])
    args.robot_list = ["r1", "r2"]
    _walk.resolve_track(ap, args)
    assert args.contact_kw["contact_bodies"] == {"r2": ["c", "d"], "r1": ["a"]}

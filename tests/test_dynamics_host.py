"""Inverse dynamics without a GPU: the header, the export and the binding of gmr_motion_dynamics, the layout of its struct, the
static stream check of its launches, the inertial parser, and the numpy reference of tests/dynamics_reference.py against its
50-digit evaluator, statics and the power balance.

The rounding floor.  |numpy reference - 50-digit evaluator| on the analytic trajectories below (seed 7, six instants; measured
here, x86-64, numpy float64):

    robot        tau (N m)   root_wrench (N, N m)   com (m)    zmp (m)      largest |tau|, |wrench|
    unitree_g1   7.8e-14     1.7e-13                8.9e-16    1.6e-15      46, 474
    booster_k1   1.8e-14     8.5e-14                8.9e-16    5.6e-16      11, 246

That is the floor at twelve well-loaded instants.  The floor the GPU tests are bounded by is measured on their own frames, lightly
loaded ones included (dynamics_reference.FLOAT_WORST, per robot; test_the_recorded_floor_covers_the_gpu_cases_own_frames)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import dynamics_reference as R
from tests.test_stream_order_host import check_api, reachable, stream_prototypes, units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMES = [0.0, 0.13, 0.29, 0.41, 0.57, 0.83]
FREE_ROOT_ROBOTS = ["unitree_g1", "unitree_g1_with_hands", "booster_t1", "stanford_toddy", "fourier_n1", "engineai_pm01", "kuavo_s45",
                    "hightorque_hi", "berkeley_humanoid_lite", "booster_k1"]


def _header():
    with open(os.path.join(ROOT, "include", "gmr_amd.h")) as f:
        return f.read()


def _xml(robot):
    from gmr_amd import params
    return os.path.join(R.ASSETS, params._ROBOT_XML_REL[robot])


# ------------------------------------------------------------------ 1: header, export, binding, layout
def test_symbol_is_declared_exported_and_bound():
    from gmr_amd import _native
    src = _header()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint gmr_motion_dynamics\s*\(gmr_model \*m, const gmr_dynamics_input \*in\);", code)
    assert "gmr_motion_dynamics" in _native.EXPORTS
    assert re.search(r"^#define GMR_ABI_VERSION 5$", src, flags=re.M) and _native.ABI_VERSION == 5   # an addition
    assert "gmr_motion_dynamics" not in stream_prototypes() and len(stream_prototypes()) == 27          # the stream travels in the struct
    lib = _native.load()
    assert lib.gmr_motion_dynamics.restype == C.c_int and len(lib.gmr_motion_dynamics.argtypes) == 2
    assert lib.gmr_motion_dynamics.argtypes[1]._type_ is _native.DynamicsInput
    assert lib.gmr_motion_dynamics(None, C.byref(_native.DynamicsInput())) == -1   # a null handle is refused before anything else
    from gmr_amd import engine
    assert engine.DYNAMICS_DEFAULTS == {"gravity": (0.0, 0.0, -9.81), "ground_z": 0.0, "fz_min": 0.05}
    assert engine.DYNAMICS_FIELDS == _native.DYNAMICS_FRAME_OUTPUTS + _native.DYNAMICS_STATS


def test_struct_layout_equals_the_c_compiler_and_the_listing_in_the_header(tmp_path):
    from gmr_amd import _native
    T = _native.DynamicsInput
    fields = [k for k, _ in T._fields_]
    src = _header()
    src = src[src[:src.index("typedef struct gmr_dynamics_input")].rindex("Layout (LP64)"):]   # (the listing nearest above the struct)
    m = re.match(r"Layout \(LP64\): sizeof (\d+); offsets (.*?)\.\s*\*/\s*typedef struct gmr_dynamics_input \{(.*?)\} gmr_dynamics_input;", src, flags=re.S)
    assert m, "the layout listing in front of gmr_dynamics_input"
    listing = {k: int(v) for k, v in re.findall(r"([a-z_0-9]+) (\d+)", re.sub(r"\s*\*\s*", " ", m.group(2)))}
    body = re.sub(r"/\*.*?\*/", "", m.group(3), flags=re.S)
    declared = []
    for stmt in body.split(";"):
        declared += re.findall(r"\*?\s*([a-z_0-9]+)\s*(?:,|$)", stmt.strip())
    assert declared == fields
    assert C.sizeof(T) == int(m.group(1)) == 272
    assert listing == {k: getattr(T, k).offset for k in fields}
    n_out = len(_native.DYNAMICS_OUTPUTS)
    assert fields[-n_out:] == [k + "_out" for k in _native.DYNAMICS_OUTPUTS] and fields[-n_out - 1] == "stream"
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        return   # (no C compiler here: the listing and ctypes agree, which is what the library is built against)
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gmr_amd.h"\nint main(void) {\n'
                    '  printf("%zu", sizeof(gmr_dynamics_input));\n'
                    + "".join(f'  printf(" %zu", offsetof(gmr_dynamics_input, {n}));\n' for n in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", f"-I{ROOT}/include", str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert C.sizeof(T) == got[0] and [getattr(T, n).offset for n in fields] == got[1:]


def test_the_launches_are_on_the_structs_stream_and_nothing_else_is_enqueued():
    problems, syncs = check_api(entries=["gmr_motion_dynamics"])
    assert not problems, "\n".join(problems)
    assert syncs == {"gmr_motion_dynamics": False}
    us = units()
    r = reachable(us, "gmr_motion_dynamics")
    assert "dynamics_run" in r and "scratch_alloc" not in r and "CallScratch" not in r                      # no allocation
    assert sum(len(re.findall(r"\bhipLaunchKernelGGL\s*\(", us[u])) for u in r) == 2                        # two kernels
    assert len(re.findall(r"\bhipLaunchKernelGGL\s*\(", us["dynamics_run"])) == 2
    assert not any(re.search(r"\bhip\w+Async\s*\(", us[u]) for u in r)                                      # no copy, no memset
    assert "static_cast<hipStream_t>(in->stream)" in re.sub(r"\s+", "", us["gmr_motion_dynamics"])


def test_the_kernel_file_has_no_floating_point_atomics_and_contraction_is_off():
    with open(os.path.join(ROOT, "gmr_amd", "csrc", "dynamics_kernel.hip.h")) as f:
        src = f.read()
    code = re.sub(r"//.*", "", src)
    assert not re.search(r"atomic", code, flags=re.I)
    for kern in ("motion_dynamics_kernel", "motion_dynamics_stats_kernel"):
        body = code[code.index(f"{kern}(const DynamicsArgs a)"):]
        assert body[:body.index("\n", body.index("{")) + 60].count("#pragma clang fp contract(off)") == 1, kern


# ------------------------------------------------------------------ 2: the inertial parser
def _files_of(path, seen=None):
    seen = [] if seen is None else seen
    seen.append(path)
    with open(path) as f:
        text = re.sub(r"<!--.*?-->", "", f.read(), flags=re.S)
    for inc in re.findall(r"<include\s+file=\"([^\"]+)\"", text):
        _files_of(os.path.join(os.path.dirname(path), inc), seen)
    return seen


@pytest.mark.parametrize("robot", FREE_ROOT_ROBOTS)
def test_total_mass_equals_the_sum_of_the_mass_attributes_of_the_files(robot):
    from gmr_amd.inertial import inertial_table
    from gmr_amd.mjcf import load_mjcf
    path = _xml(robot)
    rob = load_mjcf(path, name=robot)
    assert not rob.planar_base and rob.xml_path == os.path.abspath(path)
    tab = inertial_table(rob)
    masses = []
    for fn in _files_of(path):
        with open(fn) as f:
            text = re.sub(r"<!--.*?-->", "", f.read(), flags=re.S)
        masses += [float(x) for x in re.findall(r"<inertial\b[^>]*?\bmass=\"([^\"]+)\"", text)]
    assert len(masses) == rob.nbody - len(tab.missing) and len(masses) > 0
    assert abs(tab.total_mass - sum(masses)) <= 1e-12 * sum(masses)
    assert tab.nbody == rob.nbody and tab.armature.shape == tab.torque_limit.shape == (rob.nq - 7,)
    assert np.all(tab.torque_limit > 0.0) and np.all(tab.armature >= 0.0)
    assert np.allclose(tab.inertia, np.swapaxes(tab.inertia, 1, 2), rtol=0, atol=0)
    assert all(np.all(np.linalg.eigvalsh(I) >= -1e-12) for I in tab.inertia)
    assert [rob.body_names[b] for b in range(rob.nbody) if tab.mass[b] == 0.0 and rob.body_names[b] in tab.missing] == tab.missing


def test_a_pack_robot_has_no_inertial_data_and_says_so():
    from gmr_amd import params
    from gmr_amd.inertial import inertial_table
    from gmr_amd.mjcf import MjcfError, load_mjcf, load_robot
    pack = os.path.join(str(params.PACK_ROOT), "robots", "unitree_g1.json")
    rob = load_robot(pack, name="unitree_g1")
    assert rob.xml_path is None
    with pytest.raises(MjcfError, match="not loaded from an MJCF"):
        inertial_table(rob)
    full = load_mjcf(_xml("unitree_g1"), name="unitree_g1")
    assert full.to_dict() == rob.to_dict()   # the new field takes no part in what a robot pack holds


_TWO = """<mujoco model="two"><compiler angle="radian"/>{defaults}<worldbody><body name="base" pos="0 0 1"><freejoint name="root"/>
<inertial pos="0.01 0.02 0.03" mass="2.5" {base_inertia}/>
<body name="arm" pos="0 0 0.2"{childclass}><joint name="j" axis="0 1 0" range="-1 1"{joint_attrs}/>{arm_inertial}</body></body></worldbody>{actuators}</mujoco>"""


def _two(tmp_path, name, **kw):
    kw.setdefault("defaults", ""); kw.setdefault("childclass", ""); kw.setdefault("joint_attrs", ""); kw.setdefault("actuators", "")
    kw.setdefault("base_inertia", 'diaginertia="0.1 0.2 0.3"')
    kw.setdefault("arm_inertial", '<inertial pos="0 0 0.1" mass="0.5" diaginertia="0.01 0.01 0.001"/>')
    p = tmp_path / f"{name}.xml"
    p.write_text(_TWO.format(**kw))
    return str(p)


def test_fullinertia_and_quat_with_diaginertia_agree(tmp_path):
    from gmr_amd.inertial import load_inertial, quat_to_mat
    q = np.array([0.8, 0.2, -0.4, 0.4])
    Rm = quat_to_mat(q)
    I = Rm @ np.diag([0.1, 0.2, 0.3]) @ Rm.T
    full = " ".join(repr(float(x)) for x in (I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]))
    a = load_inertial(_two(tmp_path, "diag", base_inertia='quat="%s" diaginertia="0.1 0.2 0.3"' % " ".join(map(str, q))))
    b = load_inertial(_two(tmp_path, "full", base_inertia=f'fullinertia="{full}"'))
    assert np.abs(a.inertia[0] - b.inertia[0]).max() <= 4 * np.finfo(float).eps * 0.3
    assert np.abs(a.inertia[0] - I).max() <= 4 * np.finfo(float).eps * 0.3 and np.array_equal(a.inertia[0], a.inertia[0].T)
    assert np.array_equal(a.com[0], [0.01, 0.02, 0.03]) and a.mass.tolist() == [2.5, 0.5] and a.total_mass == 3.0
    assert a.missing == [] and a.parent.tolist() == [-1, 0]


def test_a_torque_limit_is_found_on_the_joint_in_a_default_class_and_on_an_actuator(tmp_path):
    from gmr_amd.inertial import load_inertial
    t = load_inertial(_two(tmp_path, "joint", joint_attrs=' actuatorfrcrange="-30 40" armature="0.02"'))
    assert t.torque_limit.tolist() == [40.0] and t.limit_source == ["actuatorfrcrange"] and t.armature.tolist() == [0.02]
    t = load_inertial(_two(tmp_path, "class", childclass=' childclass="limb"',
                           defaults='<default><default class="limb"><joint actuatorfrcrange="-25 25" armature="0.01"/></default></default>'))
    assert t.torque_limit.tolist() == [25.0] and t.limit_source == ["actuatorfrcrange"] and t.armature.tolist() == [0.01]
    t = load_inertial(_two(tmp_path, "motor", defaults='<default><motor ctrlrange="-2 2"/></default>',
                           actuators='<actuator><motor name="m" joint="j" gear="7.5"/></actuator>'))
    assert t.torque_limit.tolist() == [15.0] and t.limit_source == ["motor"] and t.armature.tolist() == [0.0]
    t = load_inertial(_two(tmp_path, "position", actuators='<actuator><position joint="j" ctrlrange="-1 1" forcerange="-12 12"/></actuator>'))
    assert t.torque_limit.tolist() == [12.0] and t.limit_source == ["position"]
    t = load_inertial(_two(tmp_path, "both", joint_attrs=' actuatorfrcrange="-30 40"',
                           actuators='<actuator><motor joint="j" ctrlrange="-1 1" gear="5"/></actuator>'))
    assert t.torque_limit.tolist() == [40.0]                     # the joint's own range wins
    t = load_inertial(_two(tmp_path, "none"))
    assert np.isinf(t.torque_limit[0]) and t.limit_source == ["none"]


def test_bodies_without_inertial_are_listed_and_a_model_without_any_is_an_error(tmp_path):
    from gmr_amd.inertial import load_inertial
    from gmr_amd.mjcf import MjcfError
    t = load_inertial(_two(tmp_path, "half", arm_inertial=""))
    assert t.missing == ["arm"] and t.mass.tolist() == [2.5, 0.0] and not t.inertia[1].any()
    p = tmp_path / "bare.xml"
    p.write_text('<mujoco><worldbody><body name="b"><freejoint/><body name="c"><joint axis="0 0 1"/></body></body></worldbody></mujoco>')
    with pytest.raises(MjcfError, match="no body carries"):
        load_inertial(str(p))
    g1 = R.model("unitree_g1")[1]
    assert len(g1.missing) == 7 and all(g1.mass[g1.body_names.index(n)] == 0.0 for n in g1.missing)


# ------------------------------------------------------------------ 3: the reference against 50 digits, statics, power
@pytest.fixture(scope="module", params=["unitree_g1", "booster_k1"])
def analytic(request):
    rob, tab = R.model(request.param)
    tr = R.Trajectory(rob, 7)
    q, v, a = tr.state(TIMES)
    return request.param, rob, tab, tr, q, v, a, R.dynamics(rob, tab, q, v, a)


def test_numpy_reference_against_50_digits(analytic):
    robot, rob, tab, tr, q, v, a, ref = analytic
    assert rob.nbody == (38 if robot == "unitree_g1" else 23)
    worst, mag = {k: 0.0 for k in ref}, {k: 0.0 for k in ref}
    for i, t in enumerate(TIMES):
        want = R.mp_dynamics(tr, tab, t)
        for k in ref:
            worst[k] = max(worst[k], float(np.abs(ref[k][i] - want[k]).max()))
            mag[k] = max(mag[k], float(np.abs(want[k]).max()))
    print(f"{robot}: worst |numpy - 50 digits|: " + ", ".join(f"{k} {v:.2e} (largest {mag[k]:.3g})" for k, v in worst.items()))
    for k in ref:
        assert worst[k] <= R.FLOAT_WORST[robot][k], f"{k}: the recorded floor {R.FLOAT_WORST[robot][k]:.1e} is below the measured {worst[k]:.2e}"
        assert worst[k] <= 64 * np.finfo(float).eps * max(1.0, mag[k])    # and the floor is rounding, not a modelling difference


@pytest.mark.parametrize("robot", ["unitree_g1", "booster_k1", "unitree_g1_with_hands"])
def test_the_recorded_floor_covers_the_gpu_cases_own_frames(robot):
    """The floor under the GPU bound, re-measured where it is worst: the rows of the GPU tests' explicit case with the largest torque
    and wrench, the lightest load and the largest ZMP, and every clip's first row (the recorded figures are of all 332 rows)."""
    from tests import dynamics_inputs as di
    rows = di.floor_rows(robot)
    worst = di.measure_floor(robot, rows)
    print(f"{robot}: {len(rows)} rows: worst |numpy - 50 digits|: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= R.FLOAT_WORST[robot][k], f"{k}: the recorded floor {R.FLOAT_WORST[robot][k]:.1e} is below the measured {v:.2e}"


def test_statics_the_root_force_is_the_weight(analytic):
    robot, rob, tab, tr, q, v, a, _ = analytic
    z = np.zeros_like(v)
    st = R.dynamics(rob, tab, q, z, z)
    weight = tab.total_mass * 9.81
    assert np.abs(st["root_wrench"][:, :3] - [0.0, 0.0, weight]).max() <= 16 * np.finfo(float).eps * weight
    # the ZMP of a static pose is the ground projection of the centre of mass
    assert np.abs(st["zmp"] - st["com"][:, :2]).max() <= 1e-13


def test_power_balance_on_the_analytic_trajectory(analytic):
    """F . v + M . w + tau . theta' is the rate of kinetic plus potential energy, taken in 50 digits from poses alone."""
    robot, rob, tab, tr, q, v, a, ref = analytic
    for i in (0, 2, 5):
        terms = np.concatenate([ref["root_wrench"][i, :3] * v[i, :3], ref["root_wrench"][i, 3:] * v[i, 3:6], ref["tau"][i] * v[i, 6:]])
        P, E = float(terms.sum()), R.mp_energy_rate(tr, tab, TIMES[i])
        print(f"{robot} t = {TIMES[i]}: power {P:.12g}, d/dt energy {E:.12g}, difference {abs(P - E):.2e}")
        assert abs(P - E) <= 1e-11 * np.abs(terms).sum() and abs(P) > 1.0


# ------------------------------------------------------------------ 4: differences and statistics of the reference
def test_differences_follow_the_contract_at_the_ends_of_a_clip():
    rng = np.random.default_rng(3)
    nq, fps = 10, 32.0
    offs = [0, 0, 1, 3, 6, 11]
    q = np.round(rng.uniform(-1, 1, (11, nq)) * 1024) / 1024
    q[:, 3:7] = [1.0, 0.0, 0.0, 0.0]
    v, a = R.differences(q, offs, fps)
    assert not v[0].any() and not a[0].any()                           # one frame
    assert not a[1:3].any() and np.array_equal(v[1], v[2]) and np.array_equal(v[1, 0], (q[2, 0] - q[1, 0]) * fps)   # two frames
    assert np.array_equal(a[3], a[4]) and np.array_equal(a[4], a[5])   # three frames: one interior value
    assert np.array_equal(a[6], a[7]) and np.array_equal(a[10], a[9]) and not np.array_equal(a[7], a[8])
    assert np.array_equal(a[8, 6], ((q[9, 7] - 2.0 * q[8, 7]) + q[7, 7]) * fps * fps)
    assert np.array_equal(v[8, 6], (q[9, 7] - q[7, 7]) / (2.0 / fps)) and not v[:, 3:6].any() and not a[:, 3:6].any()


def test_differences_of_a_steady_turn_give_its_rate():
    fps, rate = 64.0, 1.5
    t = np.arange(8) / fps
    q = np.zeros((8, 8))
    q[:, 3], q[:, 6] = np.cos(0.5 * rate * t), np.sin(0.5 * rate * t)
    v, a = R.differences(q, [0, 8], fps)
    assert np.abs(v[:, 5] - rate).max() <= 1e-13 and np.abs(a[:, 5]).max() <= 1e-10 and not v[:, 3:5].any()


def test_statistics_count_one_frame_over_the_limit_and_skip_a_non_finite_one():
    tab = R.model("booster_k1")[1]
    nh = tab.armature.shape[0]
    tau = np.full((7, nh), 1.0)
    wr = np.zeros((7, 6))
    wr[:, 2] = tab.total_mass * 9.81
    lim = np.where(np.isfinite(tab.torque_limit), tab.torque_limit, 1e3)
    tab = R.InertialTable(**{**tab.__dict__, "torque_limit": lim})
    tau[4, 2] = -2.0 * lim[2]
    tau[5, 0] = np.nan
    wr[6, 2] = 0.0
    st = R.statistics(tab, tau, wr, [0, 3, 7])
    assert st["frames_over_limit"].sum() == 1 and st["frames_over_limit"][1, 2] == 1 and st["frames_any_over_limit"].tolist() == [0, 1]
    assert st["tau_ratio_max"][1, 2] == 2.0 and st["tau_abs_max"][1, 2] == 2.0 * lim[2] and st["tau_rms"][0, 0] == 1.0
    assert st["nonfinite_frames"].tolist() == [0, 1] and st["unloaded_frames"].tolist() == [0, 1]
    assert st["fz_ratio_max"].tolist() == [1.0, 1.0] and st["fz_ratio_min"].tolist() == [1.0, 0.0]


# ------------------------------------------------------------------ 5: the report's CSV and the exclusion threshold
def test_dynamics_csv_names_the_worst_joint_and_the_threshold_marks_the_clip(tmp_path):
    from gmr_amd import dataset
    rep = {"tau_ratio_max": np.array([[0.2, 0.9, 0.1], [1.5, 0.3, 0.0]]), "tau_abs_max": np.array([[2.0, 9.0, 1.0], [15.0, 3.0, 4.0]]),
           "frames_any_over_limit": np.array([0, 4], np.int32), "fz_ratio_max": np.array([1.2, 2.0]), "fz_ratio_min": np.array([0.8, 0.0]),
           "unloaded_frames": np.array([0, 3], np.int32), "nonfinite_frames": np.array([0, 0], np.int32), "joint_names": ["a", "b", "c"]}
    p = tmp_path / "dyn.csv"
    dataset.write_dynamics_csv(str(p), ["walk", "jump"], rep)
    rows = [r.split(",") for r in p.read_text().strip().splitlines()]
    assert rows[0] == ["clip", *dataset.DYNAMICS_CSV_FIELDS, "worst_joint", "worst_ratio", "worst_tau_abs_max"]
    assert rows[1] == ["walk", "0", "1.2", "0.8", "0", "0", "b", "0.9", "9.0"] and rows[2][:2] == ["jump", "4"] and rows[2][-3:] == ["a", "1.5", "15.0"]
    assert dataset.dynamics_hard_mask(rep, 1.0).tolist() == [False, True] and dataset.dynamics_hard_mask(rep, 2.0).tolist() == [False, False]


def test_the_dataset_scripts_flags_ask_for_the_report_and_the_sink_writes_both_files(tmp_path):
    import argparse
    from gmr_amd import dataset
    from gmr_amd.scripts import _walk
    ap = argparse.ArgumentParser()
    _walk.add_common_flags(ap)
    off = ap.parse_args([])
    assert off.dynamics_csv is None and off.max_torque_ratio is None and not _walk.wants_dynamics(off) and not _walk.wants_report(off)
    args = ap.parse_args(["--dynamics_csv", str(tmp_path / "dyn.csv"), "--max_torque_ratio", "1.0", "--hard_out", str(tmp_path / "hard.txt")])
    assert _walk.wants_dynamics(args) and _walk.wants_report(args)
    assert _walk.report_path(args.dynamics_csv, "unitree_g1", 2).endswith("dyn.unitree_g1.rank2.csv")

    class Report:   # what dataset.report_hard_mask and report_difficulty read of a ClipReport
        task_pos_max = np.array([[0.01], [0.02]])
        dof_step_max = np.array([[0.1], [0.2]])
        err_max = np.array([[0.1, 0.1], [0.2, 0.2]])
        last_table = 1

        def __len__(self):
            return 2

    dyn = {"tau_ratio_max": np.array([[0.2, 0.9], [1.5, 0.3]]), "tau_abs_max": np.array([[2.0, 9.0], [15.0, 3.0]]),
           "frames_any_over_limit": np.array([0, 4], np.int32), "fz_ratio_max": np.array([1.2, 2.0]), "fz_ratio_min": np.array([0.8, 0.0]),
           "unloaded_frames": np.array([0, 3], np.int32), "nonfinite_frames": np.array([0, 0], np.int32), "joint_names": ["a", "b"]}
    sink = _walk.ReportSink(args)
    kept, targets = sink.take(dataset, ["out/walk.pkl", "out/jump.pkl"], ["m0", "m1"], Report(), dyn)
    assert kept == ["m0"] and targets == ["out/walk.pkl"] and sink.withheld == 1
    assert (tmp_path / "dyn.csv").read_text().splitlines()[2].startswith("jump,4,")
    assert "jump.pkl" in (tmp_path / "hard.txt").read_text() and "walk.pkl" not in (tmp_path / "hard.txt").read_text()
    # --dynamics_csv alone: the clip report is not computed, nothing is withheld, the CSV is written
    alone = ap.parse_args(["--dynamics_csv", str(tmp_path / "only.csv")])
    assert _walk.wants_dynamics(alone) and _walk.wants_sink(alone) and not _walk.wants_report(alone)
    sink = _walk.ReportSink(alone)
    kept, targets = sink.take(dataset, ["out/walk.pkl", "out/jump.pkl"], ["m0", "m1"], None, dyn)
    assert kept == ["m0", "m1"] and sink.withheld == 0 and len((tmp_path / "only.csv").read_text().splitlines()) == 3

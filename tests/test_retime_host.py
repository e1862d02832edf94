"""The host side of the retiming: the numpy restatement's own properties on the cases of tests/retime_inputs.py (the figures the
issue quotes are re-derived here), the headers, exports, bindings and struct layouts of gmr_motion_retime_plan and
gmr_motion_retime_apply, the static stream check, and the argument checks of the Python layer.  No GPU is needed."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from tests import retime_inputs as ri
from tests import retime_reference as RR
from tests.test_stream_order_host import check_api, reachable, stream_prototypes, units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gmr_motion_retime_plan", "gmr_motion_retime_apply")
G1, K1 = "unitree_g1", "booster_k1"


def clips(offs):
    return [(int(a), int(b)) for a, b in zip(offs[:-1], offs[1:])]


def all_cases():
    return [(r, n) for r in ri.ROBOTS for n in ri.CASES if n != "striding" or r == G1]


# ------------------------------------------------------------------ 1: the restatement's own properties
@pytest.mark.parametrize("robot,name", all_cases())
def test_the_mean_stretch_covers_the_raw_stretch_and_time_runs_forward(robot, name):
    c = ri.case(robot, name)
    p, out, st, oo, _ = ri.reference(robot, name)
    for s, (a, b) in enumerate(clips(c.offs)):
        if b == a:
            assert p["out_len"][s] == 0
            continue
        need, ticks, cum = p["need"][a:b], p["ticks"][a:b], p["cum"][a:b]
        assert need[-1] == 0.0 and ticks[-1] == 0 and cum[0] == 0
        raw = RR.stretches(need[:-1], c.max_stretch)
        assert np.all(ticks[:-1] >= np.ceil(raw * 1024.0))                                   # m_i >= s_i, in ticks
        assert np.all(ticks[:-1] >= 1024) and np.all(ticks[:-1] <= np.ceil(c.max_stretch * 1024.0))
        assert np.all(np.diff(cum) == ticks[:-1])                                           # cum: the earlier intervals, monotone
        total = int(cum[-1])
        assert p["clip_stats"][s, 3] == total and p["out_len"][s] == (total + 1023) // 1024 + 1
        W = c.window
        if W and b - a - 1 > 2 * W + 2:                                                     # away from the clip's ends the stretch changes slowly
            assert np.abs(np.diff(ticks[W:b - a - 1 - W])).max() <= np.ceil((c.max_stretch - 1.0) / (2 * W + 1) * 1024.0) + 1
        # the output: the exact first and last rows, a source time that runs forward and ends at the last row
        o0, o1 = int(oo[s]), int(oo[s + 1])
        assert o1 - o0 == p["out_len"][s]
        assert out[o0].tobytes() == c.q[a].tobytes() and out[o1 - 1].tobytes() == c.q[b - 1].tobytes()
        assert st[o0] == 0.0 and st[o1 - 1] == b - a - 1 and np.all(np.diff(st[o0:o1]) >= 0.0) and np.all(np.diff(st[o0:o1]) <= 1.0)


@pytest.mark.parametrize("robot", ri.ROBOTS)
def test_a_limits_nothing_reaches_give_the_input_back(robot):
    c = ri.case(robot, "identity")
    p, out, st, oo, sl = ri.reference(robot, "identity")
    assert p["out_len"].tolist() == ri.LENS and np.array_equal(oo, ri.OFFS)
    for a, b in clips(c.offs):
        assert b == a or np.all(p["ticks"][a:b - 1] == 1024)
    assert out.tobytes() == c.q.tobytes() and not sl.any()
    assert np.array_equal(st, np.concatenate([np.arange(n, dtype=np.float64) for n in ri.LENS]))
    assert not p["clip_stats"][:, :3].any() and p["need_max"].max() == 0.5


def test_b_a_uniform_limit_stretches_some_intervals_and_leaves_the_rest_alone():
    p = ri.reference(G1, "uniform")[0]
    assert p["clip_stats"][list(ri.LONG), 0].tolist() == [51, 63, 59, 108]
    touched = untouched = 0
    for s in ri.LONG:
        a, b = int(ri.OFFS[s]), int(ri.OFFS[s + 1])
        tk = p["ticks"][a:b - 1]
        assert np.array_equal(tk > 1024, p["need"][a:b - 1] > 1.0)                          # W = 0: an interval alone
        touched, untouched = touched + int((tk > 1024).sum()), untouched + int((tk == 1024).sum())
    assert touched == 281 and untouched == 37                                               # both kinds occur
    k = ri.reference(K1, "uniform")[0]
    a, b = int(ri.OFFS[ri.C130]), int(ri.OFFS[ri.C130 + 1])
    assert np.all(k["ticks"][a:b - 1] == 1024) and k["out_len"][ri.C130] == 130 and k["clip_stats"][ri.C130, 0] == 0


def test_c_per_column_limits_at_half_of_each_columns_top_speed():
    p = ri.reference(G1, "columns")[0]
    assert p["out_len"].tolist() == [0, 1, 3, 5, 7, 125, 127, 129, 251]
    assert np.abs(p["need_max"][list(ri.LONG)] - 2.0).max() <= 4 * RR.EPS and p["need_max"].max() <= 2.0 + 4 * RR.EPS   # 2 up to rounding
    assert p["need_max"][:2].tolist() == [0.0, 0.0]                                        # no interval: no need
    assert not p["clip_stats"][:, 1:3].any()


def test_d_the_widest_window_is_wider_than_the_short_clips():
    for robot in ri.ROBOTS:
        b, d = ri.reference(robot, "uniform")[0], ri.reference(robot, "wide")[0]
        assert np.array_equal(b["need"], d["need"]) and np.array_equal(b["clip_stats"][:, :3], d["clip_stats"][:, :3])
        assert np.all(d["ticks"] >= b["ticks"]) and np.all(d["out_len"] >= b["out_len"])
    d = ri.reference(G1, "wide")[0]
    for s in (2, 3, 4):                                                                     # a window over the whole clip: one stretch
        a, b = int(ri.OFFS[s]), int(ri.OFFS[s + 1])
        assert len(set(d["ticks"][a:b - 1].tolist())) == 1


def test_e_a_cap_that_binds_is_counted():
    for robot in ri.ROBOTS:
        c = ri.case(robot, "cap")
        p = ri.reference(robot, "cap")[0]
        assert np.all(p["clip_stats"][list(ri.LONG), 1] > 0) and p["ticks"].max() == 1536
        assert np.all(p["clip_stats"][:, 1] <= p["clip_stats"][:, 0]) and p["need_max"].max() > c.max_stretch


@pytest.mark.parametrize("robot", ri.ROBOTS)
def test_f_one_fast_interval_on_the_tile_edge_becomes_a_tent_of_ticks(robot):
    p, out, st, oo, _ = ri.reference(robot, "burst")
    assert p["out_len"].tolist() == [171] and p["clip_stats"][0, :3].tolist() == [1, 0, 0]
    assert abs(p["need_max"][0] - 0.5 * 64.0 / (3.0 * np.pi)) <= 4 * RR.EPS * 4
    tk = p["ticks"][:129]
    assert int(np.argmax(tk)) == 63 and np.all(tk[:47] == 1024) and np.all(tk[80:] == 1024)
    assert np.all(np.diff(tk[46:64]) > 0) and np.all(np.diff(tk[63:81]) < 0)                # up to row 63 and down again: across the edge
    assert np.array_equal(tk[47:63], tk[64:80][::-1])
    assert np.all(out[:, -1] >= 0.0) and np.all(out[:, -1] <= 0.5) and np.all(np.diff(out[:, -1]) >= 0.0)


def test_g_the_striding_library():
    c = ri.case(G1, "striding")
    p = ri.reference(G1, "striding")[0]
    lens = np.diff(c.offs)
    assert lens.size == ri.STRIDING_CLIPS + 1 and lens[ri.STRIDING_CLIPS // 2] == 1000 and set(lens.tolist()) == {5, 1000}
    assert p["clip_stats"][ri.STRIDING_CLIPS // 2, 0] > 100 and (p["out_len"] > lens).sum() > 10 and (p["out_len"] == lens).sum() > 10
    assert c.q.shape[0] <= 4000                                                             # a few thousand rows


@pytest.mark.parametrize("robot,name", all_cases())
def test_no_hinge_of_the_output_exceeds_its_limit_beyond_one_lerps_rounding(robot, name):
    """Where no interval of a clip is capped or non-finite: |dq| fps / vmax <= 1 + b, b derived in retime_reference.bound."""
    c = ri.case(robot, name)
    p, out, _, oo, _ = ri.reference(robot, name)
    b = RR.bound(c.fps, float(np.abs(c.q[:, 7:]).max()), float(c.vmax.min()), c.window, c.max_stretch)
    assert b < 1e-11
    worst = 0.0
    for s, r in enumerate(RR.ratios(out, oo, c.fps, c.vmax)):
        if r.size and not p["clip_stats"][s, 1:3].any():
            worst = max(worst, float(r.max()))
    print(f"{robot} {name}: worst |dq| fps / vmax = 1 + {worst - 1.0:.2e}, b = {b:.2e}")
    assert worst <= 1.0 + b
    if name in ("uniform", "columns", "wide", "burst", "striding"):
        assert worst > 0.99                                                                 # and the limit is used


def test_a_non_finite_hinge_entry_makes_its_two_intervals_non_finite_and_nothing_else():
    c = ri.case(K1, "identity")
    q = np.array(c.q)
    row = int(ri.OFFS[ri.C64]) + 30
    q[row, 9] = np.inf
    p = RR.plan(q, c.offs, c.fps, c.vmax, c.window, c.max_stretch)
    base = ri.reference(K1, "identity")[0]
    assert np.flatnonzero(np.isnan(p["need"])).tolist() == [row - 1, row] and p["clip_stats"][ri.C64, 2] == 2
    assert np.array_equal(p["ticks"], base["ticks"]) and np.array_equal(p["out_len"], base["out_len"])
    q = np.array(c.q)
    q[row, 2] = np.nan                                                                     # a root entry: no need, no ticks
    p = RR.plan(q, c.offs, c.fps, c.vmax, c.window, c.max_stretch)
    assert all(p[k].tobytes() == base[k].tobytes() for k in p)


# ------------------------------------------------------------------ 2: header, exports, binding, layout
def _header():
    with open(os.path.join(ROOT, "include", "gmr_amd.h")) as f:
        return f.read()


def test_symbols_are_declared_exported_and_bound():
    from gmr_amd import _native
    src = _header()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint gmr_motion_retime_plan\s*\(gmr_model \*m, const gmr_retime_plan_input \*in\);", code)
    assert re.search(r"\bint gmr_motion_retime_apply\s*\(gmr_model \*m, const gmr_retime_apply_input \*in\);", code)
    assert re.search(r"^#define GMR_ABI_VERSION 5$", src, flags=re.M) and _native.ABI_VERSION == 5   # an addition
    protos = stream_prototypes()
    assert len(protos) == 27                                                                # the stream travels in the struct
    lib = _native.load()
    for entry, struct in zip(ENTRIES, (_native.RetimePlanInput, _native.RetimeApplyInput)):
        assert entry in _native.EXPORTS and entry not in protos
        f = getattr(lib, entry)
        assert f.restype == C.c_int and len(f.argtypes) == 2 and f.argtypes[1]._type_ is struct
        assert f(None, C.byref(struct())) == -1                                             # a null handle is refused before anything else
    assert re.search(r"^ \*   gmr_motion_retime_plan, gmr_motion_retime_apply\s+\(no counterpart in the reference\)", src, flags=re.M)
    assert (_native.RETIME_MAX_NQ, _native.RETIME_MAX_WINDOW, _native.RETIME_MAX_STRETCH, _native.RETIME_Q) == (64, 32, 64.0, 1024)
    assert lib.gmr_abi_version() == 5
    with open(os.path.join(ROOT, "gmr_amd", "csrc", "retime_kernel.hip.h")) as f:
        k = f.read()
    for name, value in (("kRetimeMaxWindow", 32), ("kRetimeTile", 64), ("kRetimeTargetWaves", 16384)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, k).group(1)) == value
    assert re.search(r"constexpr int64_t kRetimeQ = 1024;", k) and RR.Q == 1024


@pytest.mark.parametrize("which", [0, 1])
def test_struct_layouts_equal_the_c_compiler_and_the_listings_in_the_header(tmp_path, which):
    from gmr_amd import _native
    T, name, size = [(_native.RetimePlanInput, "gmr_retime_plan_input", 120), (_native.RetimeApplyInput, "gmr_retime_apply_input", 88)][which]
    fields = [k for k, _ in T._fields_]
    src = _header()
    src = src[src[:src.index("typedef struct " + name)].rindex("Layout (LP64)"):]
    m = re.match(r"Layout \(LP64\): sizeof (\d+); offsets (.*?)\.\s*\*/\s*typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S)
    assert m, "the layout listing in front of " + name
    listing = {k: int(v) for k, v in re.findall(r"([a-z_0-9]+) (\d+)", re.sub(r"\s*\*\s*", " ", m.group(2)))}
    body = re.sub(r"/\*.*?\*/", "", m.group(3), flags=re.S)
    declared = []
    for stmt in body.split(";"):
        declared += re.findall(r"\*?\s*([a-z_0-9]+)\s*(?:,|$)", stmt.strip())
    assert declared == fields
    assert C.sizeof(T) == int(m.group(1)) == size
    assert listing == {k: getattr(T, k).offset for k in fields}
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        return   # (no C compiler here: the listing and ctypes agree, which is what the library is built against)
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gmr_amd.h"\nint main(void) {\n'
                    f'  printf("%zu", sizeof({name}));\n'
                    + "".join(f'  printf(" %zu", offsetof({name}, {n}));\n' for n in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", f"-I{ROOT}/include", str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert C.sizeof(T) == got[0] and [getattr(T, n).offset for n in fields] == got[1:]


def test_the_launches_are_on_the_structs_stream_and_nothing_else_is_enqueued():
    problems, syncs = check_api(entries=list(ENTRIES))
    assert not problems, "\n".join(problems)
    assert syncs == {e: False for e in ENTRIES}
    us = units()
    for entry, run, launches in ((ENTRIES[0], "retime_plan_run", 3), (ENTRIES[1], "retime_apply_run", 1)):
        r = reachable(us, entry)
        assert run in r and "scratch_alloc" not in r and "CallScratch" not in r             # no allocation
        assert sum(len(re.findall(r"\bhipLaunchKernelGGL\s*\(", us[u])) for u in r) == launches
        assert not any(re.search(r"\bhip\w+Async\s*\(", us[u]) for u in r)                   # no copy, no memset
        body = us[entry]
        assert "static_cast<hipStream_t>(in->stream)" in re.sub(r"\s+", "", body)
        assert "hipLaunchKernelGGL" not in body and "hipSetDevice" not in body              # the entry only checks ...
        assert body.index("in->n_seq == 0") < body.index(run + "(")                         # ... and returns before a launch without work
    run = us["retime_plan_run"]
    assert run.index("motion_retime_need_kernel") < run.index("motion_retime_ticks_kernel") < run.index("motion_retime_scan_kernel")
    text = open(os.path.join(ROOT, "gmr_amd", "csrc", "api.hip")).read()
    assert text.count('"GMR_AMD_RETIME_WAVES"') == 1 and "strtol" not in text                # the override goes through clip_launch.h


def test_the_kernel_file_has_no_atomics_and_contraction_is_off_where_floats_are_computed():
    with open(os.path.join(ROOT, "gmr_amd", "csrc", "retime_kernel.hip.h")) as f:
        src = f.read()
    code = re.sub(r"//.*", "", src)
    assert not re.search(r"atomic", code, flags=re.I)
    for kernel in ("motion_retime_need_kernel(RetimePlanArgs A)", "motion_retime_ticks_kernel(RetimePlanArgs A)",
                   "motion_retime_apply_kernel(RetimeApplyArgs A)"):
        body = code[code.index(kernel):]
        assert body[:body.index("\n", body.index("{")) + 60].count("#pragma clang fp contract(off)") == 1
    assert not re.search(r"\b(sin|cos|atan2|sincos|acos)\s*\(", code)                        # the only trigonometry is track_slerp's
    assert code.count("track_slerp(") == 1 and code.count("track_lerp(") == 1 and code.count("wave_max(") == 2


# ------------------------------------------------------------------ 3: the Python layer's checks
def _stand_in(planar=False, nq=10):
    import torch
    return types.SimpleNamespace(device=torch.device("cpu"), nq=nq, cm=types.SimpleNamespace(robot=types.SimpleNamespace(planar_base=planar)))


def test_bad_arguments_raise_before_the_library_is_called():
    torch = pytest.importorskip("torch")
    from gmr_amd.engine import Engine, EngineError
    q = torch.zeros((6, 10), dtype=torch.float64)
    offs, v = [0, 6], np.ones(3)
    plan = lambda *a, **k: Engine.motion_retime_plan(_stand_in(), *a, **k)   # noqa: E731
    for args, text in [((q, offs, 0.0, v, 4, 8.0), "fps"), ((q, offs, np.inf, v, 4, 8.0), "fps"), ((q, offs, np.nan, v, 4, 8.0), "fps"),
                       ((q, offs, 30.0, v, -1, 8.0), "window"), ((q, offs, 30.0, v, 33, 8.0), "window"),
                       ((q, offs, 30.0, v, 4, 0.5), "max_stretch"), ((q, offs, 30.0, v, 4, 65.0), "max_stretch"), ((q, offs, 30.0, v, 4, np.nan), "max_stretch"),
                       ((q, offs, 30.0, np.ones(4), 4, 8.0), "vmax"), ((q, offs, 30.0, [1.0, 0.0, 1.0], 4, 8.0), "vmax"),
                       ((q, offs, 30.0, [1.0, -2.0, 1.0], 4, 8.0), "vmax"), ((q, offs, 30.0, [1.0, np.nan, 1.0], 4, 8.0), "vmax")]:
        with pytest.raises(ValueError, match=text):
            plan(*args)
    with pytest.raises(EngineError, match="qpos"):
        plan(q[:, :9], offs, 30.0, v, 4, 8.0)
    with pytest.raises(EngineError, match="vmax"):
        plan(q, offs, 30.0, torch.ones(3, dtype=torch.float32), 4, 8.0)
    with pytest.raises(NotImplementedError, match="planar"):
        Engine.motion_retime_plan(_stand_in(planar=True), q, offs, 30.0, v, 4, 8.0)
    i64 = lambda n: torch.zeros(n, dtype=torch.int64)   # noqa: E731
    apply = lambda *a, **k: Engine.motion_retime_apply(_stand_in(), *a, **k)   # noqa: E731
    with pytest.raises(NotImplementedError, match="planar"):
        Engine.motion_retime_apply(_stand_in(planar=True), q, offs, {"ticks": i64(6), "cum": i64(6)}, [0, 6])
    with pytest.raises(EngineError, match="ticks"):
        apply(q, offs, {"ticks": i64(5), "cum": i64(6)}, [0, 6])
    with pytest.raises(EngineError, match="cum"):
        apply(q, offs, {"ticks": i64(6), "cum": torch.zeros(6, dtype=torch.int32)}, [0, 6])
    with pytest.raises(EngineError, match="out_offsets must hold 2 entries"):
        apply(q, offs, {"ticks": i64(6), "cum": i64(6)}, [0, 3, 6])
    with pytest.raises(EngineError, match="needs out"):
        apply(q, offs, {"ticks": i64(6), "cum": i64(6)}, torch.tensor([0, 6]))
    with pytest.raises(EngineError, match="5 rows"):                                        # (out's qpos says how many rows there are)
        apply(q, offs, {"ticks": i64(6), "cum": i64(6)}, [0, 6], out={"qpos": torch.zeros((5, 10), dtype=torch.float64), "src_time": torch.zeros(6, dtype=torch.float64)})
    with pytest.raises(EngineError, match="must not be qpos"):
        apply(q, offs, {"ticks": i64(6), "cum": i64(6)}, [0, 6], out={"qpos": q, "src_time": torch.zeros(6, dtype=torch.float64)})


def test_the_limits_table_takes_the_forms_the_retargeter_takes():
    pytest.importorskip("torch")
    from gmr_amd import dataset
    from gmr_amd.model import DEFAULT_VELOCITY_LIMIT
    from tests import dynamics_reference as DR
    rob = DR.model(G1)[0]
    hinges = sorted((int(b) for b in rob.hinge_bodies()), key=lambda b: int(rob.qpos_adr[b]))
    nh = rob.nq - 7
    assert dataset.retime_vmax(rob, 5.0).tolist() == [5.0] * nh
    name = rob.jnt_names[hinges[3]]
    v = dataset.retime_vmax(rob, {name: 2.5})
    assert v[3] == 2.5 and np.all(np.isinf(np.delete(v, 3)))                                # unnamed hinges: no limit
    d = dataset.retime_vmax(rob)                                                            # None: every limited hinge at the default
    assert np.array_equal(d, np.where([rob.jnt_limited[b] for b in hinges], DEFAULT_VELOCITY_LIMIT, np.inf))
    assert dataset.retime_vmax(rob, None, {name: 1.5})[3] == 1.5                            # None: the retargeter's own table first
    assert dataset.retime_vmax(rob, 4.0, {name: 1.5})[3] == 4.0
    for bad in (0.0, -1.0, {name: 0.0}):
        with pytest.raises(ValueError):
            dataset.retime_vmax(rob, bad)
    with pytest.raises(KeyError):
        dataset.retime_vmax(rob, {"no_such_joint": 1.0})
    assert (dataset.RETIME_WINDOW, dataset.RETIME_MAX_STRETCH) == (ri.WINDOW, ri.MAX_STRETCH) == (4, 8.0)
    with pytest.raises(NotImplementedError, match="planar"):
        dataset.retime_to_limits(types.SimpleNamespace(model=types.SimpleNamespace(planar_base=True)), None, [0], 30.0)


def test_the_walker_has_the_switch_and_it_is_off_by_default():
    import argparse
    import inspect
    from gmr_amd import dataset
    from gmr_amd.scripts import _walk
    ap = argparse.ArgumentParser()
    _walk.add_common_flags(ap)
    assert ap.parse_args([]).retime_to_limits is None                                        # off: nothing existing changes
    assert ap.parse_args(["--retime_to_limits"]).retime_to_limits is True                    # the retargeter's limits, else the default
    assert ap.parse_args(["--retime_to_limits", "6.5"]).retime_to_limits == 6.5
    for argv in (["--retime_to_limits", "0"], ["--retime_to_limits", "-1"], ["--retime_to_limits", "--robots", "unitree_g1,booster_k1"]):
        with pytest.raises(SystemExit):
            _walk.resolve_track(ap, ap.parse_args(argv))
    assert inspect.signature(dataset.retarget_clips).parameters["retime"].default is None
    src = inspect.getsource(_walk.convert)
    assert '"retime": args.retime_to_limits' in src and "**ret_kw" in src

"""The host side of the clip composition: the numpy restatement against a 50-digit evaluation of the mathematical definition, the
plan's validation, the header, the export and the binding of gmr_motion_compose, the layout of its struct and the static stream check.
No GPU is needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from gmr_amd.compose import ComposeError, ComposePlan, Segment, random_sequences
from tests import compose_inputs as ci
from tests import compose_reference as CR
from tests.test_stream_order_host import check_api, reachable, stream_prototypes, units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "gmr_motion_compose"


# ------------------------------------------------------------------ 1: the restatement against 50 digits
def _largest(q, T):
    return float(max(np.abs(q[:, :3]).max(), np.abs(q[:, 7:]).max(), np.abs(T[:, 2:4]).max(), 1.0))


@pytest.mark.parametrize("name,clip", [("blend1", 0), ("blend1", 1), ("blend8", 1), ("overlap", 0), ("overlap", 1), ("edges", 0),
                                       ("edges", 1), ("negated", 0), ("pieces", 0)])
def test_the_restatement_equals_the_definition_within_its_bound(name, clip):
    """32 K eps (1 + L) on positions, hinges and the quaternion's components outside blends; 1e-12 rad on the quaternion in blends."""
    robot = "booster_k1"
    q, plan = ci.case(robot, name)
    out, T = ci.reference(robot, name)
    K = int(plan.clip_segs[clip + 1] - plan.clip_segs[clip])
    bound = CR.mp_bound(K, _largest(q, T))
    worst = CR.measure_floor(plan, q, clip, got=out)
    print(f"{name}[{clip}]: K = {K}, worst |numpy - 50 digits| {worst}, bound {bound:.2e}, slerp bound {CR.SLERP_RAD:.0e} rad")
    assert worst["pos"] <= bound and worst["quat"] <= bound
    assert worst["slerp"] <= CR.SLERP_RAD


def test_the_long_chain_stays_within_the_bound_of_its_130_compositions():
    robot = "booster_k1"
    q, plan = ci.case(robot, "long")
    out, T = ci.reference(robot, "long")
    worst = CR.measure_floor(plan, q, 0, got=out)
    bound = CR.mp_bound(130, _largest(q, T))
    print(f"long: worst {worst}, bound {bound:.2e}")
    assert worst["pos"] <= bound and worst["quat"] <= bound and worst["slerp"] <= CR.SLERP_RAD
    assert out.shape[0] == plan.n_out_frames == 130 * 12 - 129 * 3 + 1
    assert np.array_equal(out[-1], q[int(ci.OFFS[1])])                      # the one-frame clip behind the empty one: a copy


def test_the_transforms_angle_and_shift_equal_the_definitions():
    robot = "booster_k1"
    for name in ("edges", "blend8"):
        q, plan = ci.case(robot, name)
        _, T = ci.reference(robot, name)
        _, maps = CR.mp_compose(plan, q, 0)
        K = len(maps)
        bound = CR.mp_bound(K, _largest(q, T))
        for k, (theta, t) in enumerate(maps):
            c, s, tx, ty, hw, hz = (CR.mpf(float(v)) for v in T[k])
            assert abs(float(c - CR.mp.cos(theta))) <= bound and abs(float(s - CR.mp.sin(theta))) <= bound, (name, k)
            assert abs(float(tx - t[0])) <= bound and abs(float(ty - t[1])) <= bound, (name, k)
            sign = -1 if hw * CR.mp.cos(theta / 2) + hz * CR.mp.sin(theta / 2) < 0 else 1
            assert abs(float(sign * hw - CR.mp.cos(theta / 2))) <= bound and abs(float(sign * hz - CR.mp.sin(theta / 2))) <= bound, (name, k)
    # the turn of exactly pi takes the c < 0 branch and is exact
    q, plan = ci.case(robot, "edges")
    T = ci.reference(robot, "edges")[1]
    assert T[1, 0] == -1.0 and T[1, 1] == 0.0 and abs(T[1, 4]) == 0.0 and abs(T[1, 5]) == 1.0
    assert T[int(plan.clip_segs[1]) + 1, 0] == -1.0
    for c, s in [(-1.0, 0.0), (-1.0, -0.0), (-0.5, -0.8660254037844386), (0.0, 1.0), (1.0, 0.0), (-1e-300, 1.0)]:
        hw, hz = CR.half_angle(c, s)
        assert hw >= 0.0 and abs((hw * hw - hz * hz) - c) <= 4 * CR.EPS and abs(2.0 * hw * hz - s) <= 4 * CR.EPS


def test_the_first_segment_is_copied_and_whole_clips_come_back_as_their_bytes():
    for robot in ci.ROBOTS:
        q, plan = ci.case(robot, "whole")
        out, T = ci.reference(robot, "whole")
        assert out.tobytes() == q.tobytes() and np.array_equal(T, np.tile(CR.IDENTITY, (plan.n_seg, 1)))
        assert np.array_equal(plan.out_offsets, np.concatenate([[0], np.cumsum([n for n in ci.LENS if n])]))


@pytest.mark.parametrize("robot", ci.ROBOTS)
def test_the_recorded_deviation_of_the_reproduction_case_covers_the_restatements(robot):
    q, plan = ci.case(robot, "pieces")
    out, _ = ci.reference(robot, "pieces")
    clip = q[int(ci.OFFS[ci.C130]):int(ci.OFFS[ci.C130 + 1])]
    assert out.shape == clip.shape
    d = float(np.abs(out - clip).max())
    print(f"{robot}: the restatement's deviation from the clip {d:.3e}, recorded {ci.PIECES_D[robot]:.1e}")
    assert d <= ci.PIECES_D[robot] <= 4.0 * max(d, 1e-16)
    assert np.array_equal(out[:42], clip[:42])                              # the first piece outside its overlap: copied


def test_sign_continuity_of_the_restatement_with_a_negated_source_clip():
    """The composition of the library whose 64-frame clip has its quaternions negated is, byte for byte, the composition of the
    library as it is: the segment's half angle takes the other sign, and (-h) (x) (-r) = h (x) r."""
    robot = "booster_k1"
    q, plan = ci.case(robot, "negated")
    out, T = ci.reference(robot, "negated")
    plain, T0 = CR.compose(plan, ci.qpos(robot))
    assert np.array_equal(T[:, :4], T0[:, :4]) and np.array_equal(T[1, 4:], -T0[1, 4:]) and np.array_equal(T[[0, 2], 4:], T0[[0, 2], 4:])
    assert out.tobytes() == plain.tobytes()
    assert np.all(np.sum(out[1:, 3:7] * out[:-1, 3:7], axis=1) > 0.0)
    flipped = CR.compose(plan, q, T=T0)[0]                                  # without the fix the sign jumps behind the overlap
    assert not np.all(np.sum(flipped[1:, 3:7] * flipped[:-1, 3:7], axis=1) > 0.0)


# ------------------------------------------------------------------ 2: the plan
def test_out_offsets_for_blends_of_one_frame_and_of_a_whole_segment():
    offs = ci.OFFS
    p = ComposePlan(offs, [[Segment(ci.C63, 0, 63), Segment(ci.C64, 0, 64)], [], [Segment(ci.C65, 3, 10)]], 1)
    assert p.out_offsets.tolist() == [0, 126, 126, 136] and p.n_out_frames == 136 and p.n_seg == 3 and p.n_out == 3
    assert p.seg_src.tolist() == [int(offs[ci.C63]), int(offs[ci.C64]), int(offs[ci.C65]) + 3] and p.seg_len.tolist() == [63, 64, 10]
    assert p.seg_blend.tolist() == [0, 1, 0] and p.seg_out.tolist() == [0, 62, 126] and p.clip_segs.tolist() == [0, 2, 2, 3]
    assert p.seg_src.dtype == p.seg_out.dtype == p.clip_segs.dtype == p.out_offsets.dtype == np.int64
    assert p.seg_len.dtype == p.seg_blend.dtype == np.int32
    assert p.blended_rows().sum() == 1 and p.blended_rows()[62]
    whole = ComposePlan(offs, [[Segment(ci.C130, 0, 70), Segment(ci.C64, 0, 64)], [Segment(3, 0, 3), Segment(ci.C63, 0, 63)]], [64, 3])
    assert whole.out_offsets.tolist() == [0, 70, 133] and whole.seg_out.tolist() == [0, 6, 70, 70] and whole.blended_rows().sum() == 67
    # seg_out[k] = seg_out[k-1] + seg_len[k-1] - seg_blend[k], on every case of the tests
    for name in ci.CASES:
        plan = ci.case("booster_k1", name)[1]
        for o in range(plan.n_out):
            k0, k1 = int(plan.clip_segs[o]), int(plan.clip_segs[o + 1])
            assert (plan.seg_blend[k0:k1] == 0).tolist() == [True] + [False] * (k1 - k0 - 1) if k1 > k0 else True
            for k in range(k0 + 1, k1):
                assert plan.seg_out[k] == plan.seg_out[k - 1] + plan.seg_len[k - 1] - plan.seg_blend[k]
            if k1 > k0:
                assert plan.seg_out[k0] == plan.out_offsets[o] and plan.seg_out[k1 - 1] + plan.seg_len[k1 - 1] == plan.out_offsets[o + 1]
    assert ComposePlan(offs, [], 8).n_out_frames == 0 and ComposePlan(offs, [[]], 8).out_offsets.tolist() == [0, 0]


def test_every_invariant_raises_a_compose_error_that_names_the_segment():
    offs = ci.OFFS
    A, B = Segment(ci.C63, 0, 20), Segment(ci.C64, 0, 10)
    bad = [([[Segment(ci.S, 0, 1)]], 8, "there are 9 clips"), ([[Segment(-1, 0, 1)]], 8, "there are 9 clips"),
           ([[Segment(ci.C63, 0, 0)]], 8, "at least one frame"), ([[Segment(ci.C63, 60, 4)]], 8, "the clip has 63 frames"),
           ([[Segment(ci.C63, -1, 4)]], 8, "the clip has 63 frames"), ([[Segment(0, 0, 1)]], 8, "the clip has 0 frames"),
           ([[A, B]], 0, "overlaps at least one frame"), ([[A, B]], -2, "overlaps at least one frame"),
           ([[B, A]], 11, "longer than the segment before it"), ([[A, B]], 11, "are more than its length"),
           ([[A, B, A]], [6, 5], r"segment 1 \(clip 6, begin 0, length 10\): the blends before and after it, 6 \+ 5"),
           ([[A, B]], [1, 2], "2 blends for 1 transitions"), ([[A, B]], [[1], [2]], "2 lists for 1 output clips"),
           ([[A, B]], 1.5, "must be an int")]
    for sequences, blend, text in bad:
        with pytest.raises(ComposeError, match=text):
            ComposePlan(offs, sequences, blend)
    with pytest.raises(ComposeError, match="seq_offsets"):
        ComposePlan([1, 5], [[Segment(0, 0, 2)]], 1)
    assert issubclass(ComposeError, ValueError)
    ComposePlan(offs, [[A, B, A]], [6, 4])                                  # 6 + 4 == 10: allowed
    ComposePlan(offs, [[B, A]], 10)                                         # 10 == 10: allowed


def test_random_sequences_draw_valid_chains_and_are_reproducible():
    seqs = random_sequences(ci.OFFS, 5, 4, 20, 8, rng=3)
    assert seqs == random_sequences(ci.OFFS, 5, 4, 20, 8, rng=np.random.default_rng(3))
    assert len(seqs) == 5 and all(len(c) == 4 for c in seqs)
    assert all(isinstance(s, Segment) and s.length >= 20 and s.clip in (ci.C63, ci.C64, ci.C65, ci.C130) for c in seqs for s in c)
    plan = ComposePlan(ci.OFFS, seqs, 8)
    assert plan.n_seg == 20 and plan.n_out_frames == int(plan.seg_len.sum()) - 15 * 8
    assert all(s.length >= 16 for c in random_sequences(ci.OFFS, 3, 2, 0, 8, rng=0) for s in c)   # room for both blends
    with pytest.raises(ComposeError, match="no clip has"):
        random_sequences(ci.OFFS, 1, 2, 131, 8)
    with pytest.raises(ComposeError):
        random_sequences(ci.OFFS, 1, 2, 10, 0)


def test_the_plan_module_needs_no_torch():
    import gmr_amd.compose as mod
    assert mod.ComposePlan([0, 4], [[(0, 0, 4), (0, 0, 4)]], 2).n_out_frames == 6   # plain tuples will do
    with open(mod.__file__) as f:
        src = f.read()
    assert not re.search(r"^\s*(import|from)\s+torch", src, flags=re.M) and not re.search(r"^\s*from\s+\.(engine|dataset)", src, flags=re.M)


# ------------------------------------------------------------------ 3: header, export, binding, layout
def _header():
    with open(os.path.join(ROOT, "include", "gmr_amd.h")) as f:
        return f.read()


def test_symbol_is_declared_exported_and_bound():
    from gmr_amd import _native
    src = _header()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint gmr_motion_compose\s*\(gmr_model \*m, const gmr_compose_input \*in\);", code)
    assert ENTRY in _native.EXPORTS
    assert re.search(r"^#define GMR_ABI_VERSION 5$", src, flags=re.M) and _native.ABI_VERSION == 5   # an addition
    assert ENTRY not in stream_prototypes() and len(stream_prototypes()) == 27                        # the stream travels in the struct
    assert re.search(r"^ \*   gmr_motion_compose\s+\(no counterpart in the reference\)", src, flags=re.M)
    assert _native.COMPOSE_MAX_NQ == 64
    lib = _native.load()
    assert lib.gmr_motion_compose.restype == C.c_int and len(lib.gmr_motion_compose.argtypes) == 2
    assert lib.gmr_motion_compose.argtypes[1]._type_ is _native.ComposeInput
    assert lib.gmr_motion_compose(None, C.byref(_native.ComposeInput())) == -1   # a null handle is refused before anything else
    assert lib.gmr_abi_version() == 5


def test_struct_layout_equals_the_c_compiler_and_the_listing_in_the_header(tmp_path):
    from gmr_amd import _native
    T = _native.ComposeInput
    fields = [k for k, _ in T._fields_]
    src = _header()
    src = src[src[:src.index("typedef struct gmr_compose_input")].rindex("Layout (LP64)"):]
    m = re.match(r"Layout \(LP64\): sizeof (\d+); offsets (.*?)\.\s*\*/\s*typedef struct gmr_compose_input \{(.*?)\} gmr_compose_input;", src, flags=re.S)
    assert m, "the layout listing in front of gmr_compose_input"
    listing = {k: int(v) for k, v in re.findall(r"([a-z_0-9]+) (\d+)", re.sub(r"\s*\*\s*", " ", m.group(2)))}
    body = re.sub(r"/\*.*?\*/", "", m.group(3), flags=re.S)
    declared = []
    for stmt in body.split(";"):
        declared += re.findall(r"\*?\s*([a-z_0-9]+)\s*(?:,|$)", stmt.strip())
    assert declared == fields
    assert C.sizeof(T) == int(m.group(1)) == 104
    assert listing == {k: getattr(T, k).offset for k in fields}
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        return   # (no C compiler here: the listing and ctypes agree, which is what the library is built against)
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gmr_amd.h"\nint main(void) {\n'
                    '  printf("%zu", sizeof(gmr_compose_input));\n'
                    + "".join(f'  printf(" %zu", offsetof(gmr_compose_input, {n}));\n' for n in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", f"-I{ROOT}/include", str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert C.sizeof(T) == got[0] and [getattr(T, n).offset for n in fields] == got[1:]


def test_the_two_launches_are_on_the_structs_stream_and_nothing_else_is_enqueued():
    problems, syncs = check_api(entries=[ENTRY])
    assert not problems, "\n".join(problems)
    assert syncs == {ENTRY: False}
    us = units()
    r = reachable(us, ENTRY)
    assert "compose_run" in r and "scratch_alloc" not in r and "CallScratch" not in r                     # no allocation
    assert sum(len(re.findall(r"\bhipLaunchKernelGGL\s*\(", us[u])) for u in r) == 2                      # two launches
    assert not any(re.search(r"\bhip\w+Async\s*\(", us[u]) for u in r)                                    # no copy, no memset
    assert "static_cast<hipStream_t>(in->stream)" in re.sub(r"\s+", "", us[ENTRY])
    body = us[ENTRY]
    assert "hipLaunchKernelGGL" not in body and "hipSetDevice" not in body                                # the entry only checks ...
    assert body.index("in->n_seg == 0") < body.index("in->qpos_out == in->qpos") < body.index("compose_run(")   # ... and refuses first
    run = us["compose_run"]
    assert run.index("motion_compose_plan_kernel") < run.index("gmr::motion_compose_kernel")              # the plan first


def test_the_kernel_file_has_no_atomics_no_lds_no_barrier_and_contraction_is_off():
    with open(os.path.join(ROOT, "gmr_amd", "csrc", "compose_kernel.hip.h")) as f:
        src = f.read()
    code = re.sub(r"//.*", "", src)
    assert not re.search(r"atomic", code, flags=re.I) and "__syncthreads" not in code and "__shared__" not in code
    for kernel in ("motion_compose_plan_kernel(ComposeArgs A)", "motion_compose_kernel(ComposeArgs A)"):
        body = code[code.index(kernel):]
        assert body[:body.index("\n", body.index("{")) + 60].count("#pragma clang fp contract(off)") == 1
    assert not re.search(r"\b(sin|cos|atan2|sincos|acos)\s*\(", code)      # the only trigonometry is track_slerp's
    assert code.count("track_slerp(") == 1

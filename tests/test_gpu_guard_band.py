"""Every stream-taking entry stays inside the arrays it was given (tests/guard_band.py has the harness; include/gmr_amd.h,
"Extent and alignment", the contract).

The cases are the ones of the stream-order tests (tests/test_gpu_stream_order.py: CASES, and the three of the contact, foot-lock
and low-pass modules): one call with every device input, host table, device output and host output it touches.  Here each of
those arrays sits alone in a guarded arena filled with 0x00, 0xFF and 0x41 in turn; a call must leave every guard and every
input as it found them, give the same bytes under the three fills -- a result that depends on bytes outside a declared input
does not, nor does an output element nothing wrote -- and those bytes must be the answer it gives in ordinary torch allocations.

  test_stays_inside_its_arrays                 all 30 cases, every array 256-byte aligned
  test_edge_lengths                            the entries whose only size is a frame count, at 1, 63, 64 and 65 frames
  test_paths_the_stream_cases_do_not_take      optional outputs left out, the other FK kernels, the generic IK instance
  test_element_aligned_pointers                all 30 again with the inputs, the outputs or both only element-aligned
  test_the_harness_sees_the_real_library       an output / input declared one row short: the kernel's last row is the guard

Measured on one MI355X (ROCm 7): DESIGN.md 3f."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gmr_amd import _native  # noqa: E402
from tests import guard_band as gb  # noqa: E402
from tests import stream_order as so  # noqa: E402
from tests.test_gpu_contact import ContactCase  # noqa: E402
from tests.test_gpu_footlock import FootlockCase  # noqa: E402
from tests.test_gpu_lowpass import FilteredTrack  # noqa: E402
from tests.test_gpu_stream_order import (CASES, DEV, ENTRIES, F64, IKCase, MotionCase, case_bvh_fk, case_evaluate, case_fk,  # noqa: E402
                                         case_kin, case_smplx)
from tests.util import compiled  # noqa: E402

EXTRA = {"gmr_motion_contacts": ContactCase, "gmr_motion_footlock": FootlockCase, "gmr_motion_track/lowpass": lambda: FilteredTrack(0)}
ALL = ENTRIES + sorted(EXTRA)
LENGTHS = [1, 63, 64, 65]   # one frame; a tile short by one; an exact tile; a tile plus one (an odd element count for pair and quad stores)


def _plain(case):
    """The case's answer in ordinary torch allocations."""
    ser = so.serial_answers(case, DEV())
    assert ser["deterministic"], f"{case.entry}: two runs on the same inputs differ in {so.differing(ser['true'], ser['true2'])}"
    return ser["true"]


@functools.lru_cache(maxsize=None)
def _case(entry):
    case = CASES[entry](0) if entry in CASES else EXTRA[entry]()
    return case, _plain(case)


@functools.lru_cache(maxsize=None)
def _aligned_answer(entry):
    case, plain = _case(entry)
    return gb.check(case, DEV(), plain, 0, 0)


# ------------------------------------------------------------------ 1: all 30, aligned
def test_the_thirty_cases():
    assert len(ALL) == 30 and len(ENTRIES) == 27


@pytest.mark.parametrize("entry", ALL)
def test_stays_inside_its_arrays(entry):
    """The cases' own sizes hold the edges of the clip-table entries: 200 frames = 3 x 64 + 8, clips of 70, 1 and 129 frames, 65 IK
    frames in nine items, 130 -> 65 resampled SMPL-X frames, an empty SMPL-X clip."""
    _aligned_answer(entry)


# ------------------------------------------------------------------ 2: the entries whose only size is a frame count
BY_LENGTH = {
    "gmr_fk": lambda n: case_fk(0, n=n),
    "gmr_fk_shape": lambda n: case_fk(0, shape=True, n=n),
    "gmr_dof_to_rot": lambda n: case_kin(0, "gmr_dof_to_rot", n),
    "gmr_rot_to_dof": lambda n: case_kin(0, "gmr_rot_to_dof", n),
    "gmr_local_rot_to_global": lambda n: case_kin(0, "gmr_local_rot_to_global", n),
    "gmr_evaluate": lambda n: case_evaluate(0, n),
    "gmr_bvh_fk": lambda n: case_bvh_fk(0, False, n),
    "gmr_bvh_fk_rows": lambda n: case_bvh_fk(0, True, n),
}
for _name in ("gmr_smplx_keypoints", "gmr_smplx_keypoints_cols", "gmr_smplx_keypoints_in"):
    BY_LENGTH[_name] = lambda n, _name=_name: case_smplx(0, _name, n, n)
    BY_LENGTH[_name + "/T=2n"] = lambda n, _name=_name: case_smplx(0, _name, 2 * n, n)


def _check_fresh(case, shift_in=0, shift_out=0):
    return gb.check(case, DEV(), _plain(case), shift_in, shift_out)


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("entry", sorted(BY_LENGTH))
def test_edge_lengths(entry, n):
    case = BY_LENGTH[entry](n)
    assert case.entry == entry.split("/")[0]
    _check_fresh(case)


# ------------------------------------------------------------------ 3: the paths the stream cases do not take
@functools.lru_cache(maxsize=None)
def _fk_engine(robot, parts):
    """A handle of its own: GMR_AMD_FK_PARTS is read when the handle is created."""
    import os
    from gmr_amd.engine import Engine
    old = os.environ.get("GMR_AMD_FK_PARTS")
    try:
        if parts is None:
            os.environ.pop("GMR_AMD_FK_PARTS", None)
        else:
            os.environ["GMR_AMD_FK_PARTS"] = str(parts)
        return Engine(compiled("smplx", robot), 0)
    finally:
        os.environ.pop("GMR_AMD_FK_PARTS", None)
        if old is not None:
            os.environ["GMR_AMD_FK_PARTS"] = old


def _epilogue_without_height_adjust(n, min_z=False):
    offs = (np.array([0, n // 2, n // 2, n], np.int64), np.array([0, n, n, n], np.int64))   # clips of n / 2, 0 and the rest
    c = MotionCase(0, "epilogue", False, offs)
    c.epilogue_flags = _native.MOTION_ROOT_ORIGIN
    if not min_z:                       # min_z_out = NULL (the struct's field stays zero): no per-clip minimum is computed at all
        del c.out_spec["min_z_out0"]
        c.out_names.remove("min_z_out")
    return c


# gmr_fk with body_rot = NULL launches fk_pos_kernel<parts> (api.hip, gmr_fk): parts = 1 unless the whole-tile image,
# (7 max(1, nslots) + 3 nbody) x 256 bytes, is beyond 160 KiB, which no model within GMR_MAX_BODIES = 64 reaches (7 x 64 + 3 x 64 =
# 640 words per frame is exactly the limit, and a tree has fewer branch slots than bodies): unitree_g1 and unitree_g1_with_hands
# both take fk_pos_kernel<1>, and so would any synthetic tree.  fk_pos_kernel<2> and the grouped flush of fk_kernel<0> without
# rotations are reached the way the experiments of DESIGN.md reach them, with GMR_AMD_FK_PARTS = 2 and 0 at handle creation.
OTHER_PATHS = {
    "gmr_fk/no_rot/unitree_g1/fk_pos_kernel<1>": lambda n: case_fk(0, n=n, want_rot=False),
    "gmr_fk/no_rot/unitree_g1_with_hands/fk_pos_kernel<1>": lambda n: case_fk(0, n=n, eng=_fk_engine("unitree_g1_with_hands", None), want_rot=False),
    "gmr_fk/no_rot/unitree_g1_with_hands/fk_pos_kernel<2>": lambda n: case_fk(0, n=n, eng=_fk_engine("unitree_g1_with_hands", 2), want_rot=False),
    "gmr_fk/no_rot/unitree_g1/fk_kernel<0>": lambda n: case_fk(0, n=n, eng=_fk_engine("unitree_g1", 0), want_rot=False),
    "gmr_fk/rot/unitree_g1_with_hands": lambda n: case_fk(0, n=n, eng=_fk_engine("unitree_g1_with_hands", None)),
    "gmr_evaluate/no_err": lambda n: case_evaluate(0, n, omit=("err",)),
    "gmr_evaluate/no_task_err": lambda n: case_evaluate(0, n, omit=("task_err",)),
    "gmr_evaluate/no_xpos": lambda n: case_evaluate(0, n, omit=("xpos",)),
    "gmr_evaluate/no_xquat": lambda n: case_evaluate(0, n, omit=("xquat",)),
    "gmr_motion_epilogue/no_height_adjust/no_min_z": _epilogue_without_height_adjust,
    "gmr_motion_epilogue/no_height_adjust/min_z": lambda n: _epilogue_without_height_adjust(n, True),   # still written: the header
}


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("path", sorted(OTHER_PATHS))
def test_paths_the_stream_cases_do_not_take(path, n):
    _check_fresh(OTHER_PATHS[path](n))


def test_paths_the_stream_cases_do_not_take_ik_f64():
    """gmr_ik_solve with float64 key-points runs the generic kernel instance (the stream case's float32 ones the shaped one); its
    size is the case's 65 frames in nine items."""
    case = IKCase(0, "solve", False, dtype=F64)
    ans = _check_fresh(case)
    assert set(ans) == {"qpos0", "iters0"}


# ------------------------------------------------------------------ 4: element-aligned pointers (after the aligned tests)
@pytest.mark.parametrize("which", ["in", "out", "both"])
@pytest.mark.parametrize("entry", ALL)
def test_element_aligned_pointers(entry, which):
    """test_engine_epilogue_unaligned_out's property for the whole ABI: with every input, every output or both one element off a
    256-byte boundary (4 bytes for float32 / int32, 8 for float64 / int64, 1 for text), the bytes are those of the aligned call
    and nothing outside the arrays is touched.  No entry refuses such a pointer."""
    case, _ = _case(entry)
    aligned = _aligned_answer(entry)
    got = gb.check(case, DEV(), aligned, 1 if which in ("in", "both") else 0, 1 if which in ("out", "both") else 0)
    assert so.same(got, aligned)


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("path", ["gmr_fk/no_rot/unitree_g1/fk_pos_kernel<1>", "gmr_fk/no_rot/unitree_g1_with_hands/fk_pos_kernel<2>",
                                  "gmr_fk/no_rot/unitree_g1/fk_kernel<0>"])
def test_element_aligned_pointers_of_the_other_fk_kernels(path, n):
    """(the 16-byte tile stores of fk_pos_kernel<1> are reached by no case of the sweep above)"""
    case = OTHER_PATHS[path](n)
    aligned = _check_fresh(case)
    assert so.same(gb.check(case, DEV(), aligned, 1, 1), aligned)


# ------------------------------------------------------------------ 5: the harness sees the real library
def _short_by_a_row(case, kind, name):
    """The case with one array declared one leading row shorter than the call says; returns the bytes of that row."""
    if kind == "out":
        shape, dt = case.out_spec[name]
        case.out_spec[name] = ((shape[0] - 1,) + tuple(shape[1:]), dt)
        return int(np.prod(shape[1:])) * torch.empty((), dtype=dt).element_size()
    t, d = case.dev_in[name]
    case.dev_in[name] = (t[:-1].contiguous(), d[:-1].contiguous())
    return t[0].numel() * t.element_size()


CONTROLS = {"gmr_fk": (lambda: case_fk(0, n=65), "body_pos", "dof"),
            "gmr_motion_epilogue": (lambda: MotionCase(0, "epilogue", False), "local_body_pos_out0", "qpos0")}


@pytest.mark.parametrize("entry", sorted(CONTROLS))
def test_the_harness_sees_the_real_library(entry):
    """Two controls that need no broken kernel and never leave the arena.  (i) An output declared one row shorter than n_frames
    says: the kernel's last row lands in the guard and is reported as a write behind that buffer, and nowhere else.  (ii) An
    input declared one row shorter: the kernel's last row is the guard, and the three fills' answers differ."""
    make, out_name, in_name = CONTROLS[entry]
    case = make()
    row = _short_by_a_row(case, "out", out_name)
    for fill in gb.FILLS:
        _, viol = gb.run(case, DEV(), fill)
        assert len(viol) == 1, (fill, viol)
        name, side, first, count = viol[0]
        assert (name, side) == ("out:" + out_name, "after"), viol
        # the row's bytes but for those that happen to equal the fill: few of a pose's float32 do, except under the zero fill,
        # where the root's own local position (0, 0, 0) and every exact zero behind it go unseen
        assert 0 <= first and first + count <= row and count > row // 2, (fill, viol, row)
    case = make()
    _short_by_a_row(case, "in", in_name)
    runs = {fill: gb.run(case, DEV(), fill) for fill in gb.FILLS}
    assert all(not viol for _, viol in runs.values()), {f: v for f, (_, v) in runs.items()}
    a0, a1, a2 = (runs[f][0] for f in gb.FILLS)
    assert not so.same(a0, a1) and not so.same(a0, a2) and not so.same(a1, a2)
    with pytest.raises(AssertionError, match="fills .* differ"):
        gb.check(case, DEV(), a0)

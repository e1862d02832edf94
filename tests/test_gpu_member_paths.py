"""The three member-wise host paths of gmr_amd/csrc/api.hip (motion_run, track_run, report_run) through their single and group
entries: a member without work in the MIDDLE of a group, and every refusal with its return code and full message.

Skipped member: a group of three free-joint robots; member 1 has n_frames = 0 with n_seq > 0, members 0 and 2 have clips of 0, 1
and 65 frames (an empty clip, a single frame, one frame past the 64-frame tile) and different clip counts.  Every output of
members 0 and 2 equals that member's single call bit for bit (the single calls are tied to the oracle and the references by the
tests of each path; nothing here restates a tolerance).

Refusals: one row per message of the three paths, through the single form and, with the bad member at index 1 of three, through
the group form ("member 1: " in front, except for the messages about the call as a whole), plus inputs that break two rules at
once, which report the rule that is checked first.  Rows that are left out:
  - "hipSetDevice failed", "hipMemsetD32Async failed", the scratch allocation's message, "hipMemcpyAsync failed" and "kernel launch
    failed" (all three paths): device failures;
  - "the epilogue tile needs N bytes of LDS", "the tracking tile needs N bytes of LDS": no model the library accepts is that large;
  - "the low-pass filter takes at most 64 qpos columns": no robot of the registry has more than 57 hinges;
  - "model has no IK config": every robot of the registry is compiled with its tasks;
  - "clip s: no low-pass coefficients": unreachable, the cutoff is refused during validation."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gmr_amd import _native  # noqa: E402
from gmr_amd.engine import _REPORT_FIELDS, TRACK_FIELDS, _motion_input, _report_input, _track_input  # noqa: E402
from tests.test_gpu_motion_epilogue import _random_qpos  # noqa: E402

ROBOTS = ["unitree_g1", "booster_t1", "stanford_toddy"]
CLIPS = {0: np.array([0, 0, 1, 66], dtype=np.int64),            # lengths 0, 1, 65
         2: np.array([0, 65, 65, 66, 131], dtype=np.int64)}    # lengths 65, 0, 1, 65
FPS_IN, FPS_OUT = 30.0, 50.0
EINVAL, EUNSUPPORTED = -1, -3
INF = float("inf")


@pytest.fixture(scope="module")
def group():
    from gmr_amd import MultiRobotRetargeting
    mr = MultiRobotRetargeting("smplx", ROBOTS, device=0)
    yield mr
    torch.cuda.synchronize()
    mr.close()


@pytest.fixture(scope="module")
def planar_group():
    from gmr_amd import MultiRobotRetargeting
    mr = MultiRobotRetargeting("smplx", ["unitree_g1", "galaxea_r1pro"], device=0)
    yield mr
    mr.close()


def _bits_equal(a, b):
    iv = {8: torch.int64, 4: torch.int32, 1: torch.uint8}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(iv), b.view(iv))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _keypoints(cm, N, seed):
    """Random key-points for the model's slots behind one column nothing consumes -- (pos, quat, slot_col)."""
    names = ["_unused"] + list(cm.slot_names)
    rng = np.random.default_rng(seed)
    pos = rng.normal(size=(N, len(names), 3)) * 0.5 + [0.0, 0.0, 0.9]
    w = rng.normal(size=(N, len(names), 4))
    return torch.from_numpy(pos).cuda(), torch.from_numpy(w / np.linalg.norm(w, axis=-1, keepdims=True)).cuda(), \
        np.ascontiguousarray(cm.slot_columns(names), dtype=np.int32)


# ------------------------------------------------------------------ a member without work in the middle
def test_epilogue_skipped_member_in_the_middle(group):
    lib, engs = group.group._lib, group.engines
    qs = {i: _random_qpos(ROBOTS[i], CLIPS[i], 300 + i) for i in (0, 2)}
    flags = (True, True, 0.03)  # height adjust, root origin, ground offset
    inputs = (_native.MotionInput * 3)()
    outs, mins, keep = {}, {}, []
    for i in (0, 2):
        mins[i] = torch.full((len(CLIPS[i]) - 1,), float("nan"), dtype=torch.float32, device="cuda")
        inputs[i], outs[i], k = _motion_input(engs[i], qs[i], CLIPS[i], *flags, None, mins[i])
        keep.append(k)
    idle = np.zeros(4, dtype=np.int64)
    mins[1] = torch.full((3,), float("nan"), dtype=torch.float32, device="cuda")
    inputs[1].n_frames, inputs[1].n_seq, inputs[1].seq_offsets, inputs[1].min_z_out = 0, 3, idle.ctypes.data, mins[1].data_ptr()
    inputs[1].flags = _native.MOTION_HEIGHT_ADJUST | _native.MOTION_ROOT_ORIGIN
    assert lib.gmr_group_motion_epilogue(group.group._g, inputs, _stream()) == 0
    assert torch.isinf(mins[1]).all() and (mins[1] > 0).all()
    for i in (0, 2):
        mz = torch.full_like(mins[i], float("nan"))
        mi, alone, k = _motion_input(engs[i], qs[i], CLIPS[i], *flags, None, mz)
        assert lib.gmr_motion_epilogue(engs[i]._h, C.byref(mi), _stream()) == 0
        for a, b in zip(outs[i], alone):
            assert a.shape[0] == int(CLIPS[i][-1]) and _bits_equal(a, b), i
        assert _bits_equal(mins[i], mz) and torch.isfinite(mz[torch.from_numpy(np.diff(CLIPS[i]) > 0).cuda()]).all(), i


def test_track_skipped_member_in_the_middle(group):
    lib, engs = group.group._lib, group.engines
    qs = {i: _random_qpos(ROBOTS[i], CLIPS[i], 310 + i) for i in (0, 2)}
    cut = {0: 6.0, 2: 0.0}  # member 0 is filtered, member 2 is not
    inputs = (_native.TrackInput * 3)()
    outs, keep = {}, []
    for i in (0, 2):
        inputs[i], outs[i], k = _track_input(engs[i], qs[i], CLIPS[i], FPS_IN, FPS_OUT, None, True, lowpass_hz=cut[i])
        keep.append(k)
    inputs[1].n_frames, inputs[1].n_seq, inputs[1].fps_out = 0, 2, FPS_OUT
    assert lib.gmr_group_motion_track(group.group._g, inputs, _stream()) == 0
    for i in (0, 2):
        ti, alone, k = _track_input(engs[i], qs[i], CLIPS[i], FPS_IN, FPS_OUT, None, True, lowpass_hz=cut[i])
        assert lib.gmr_motion_track(engs[i]._h, C.byref(ti), _stream()) == 0
        assert set(alone) == set(TRACK_FIELDS) and np.array_equal(alone.out_offsets, outs[i].out_offsets) and alone.out_offsets[-1] > 65
        for f in TRACK_FIELDS:
            assert _bits_equal(outs[i][f], alone[f]), (i, f)


def test_report_skipped_member_in_the_middle(group):
    lib, engs = group.group._lib, group.engines
    offs = {0: CLIPS[0], 1: np.zeros(3, dtype=np.int64), 2: CLIPS[2]}  # member 1: two clips, no frames
    qs = {i: _random_qpos(ROBOTS[i], offs[i], 320 + i) for i in (0, 2)}
    qs[1] = torch.zeros((0, engs[1].nq), dtype=torch.float64, device="cuda")
    kp = {0: _keypoints(group._cms[0], int(offs[0][-1]), 77), 1: (None, None, None), 2: (None, None, None)}  # key-points on member 0 only
    prm = _native.ClipReportParams(1e-3, 0, 0)

    def make(i):
        ri, rep, k = _report_input(engs[i], qs[i], kp[i][0], kp[i][1], kp[i][2], offs[i], None, None)
        for f in _REPORT_FIELDS:
            if getattr(rep, f) is not None:
                getattr(rep, f).fill_(7)
        return ri, rep, k

    inputs = (_native.ClipReportInput * 3)()
    reps, keep = {}, []
    for i in range(3):
        inputs[i], reps[i], k = make(i)
        keep.append(k)
    assert lib.gmr_group_clip_report(group.group._g, inputs, C.byref(prm), _stream()) == 0
    for i in range(3):
        ri, alone, k = make(i)
        assert lib.gmr_clip_report(engs[i]._h, C.byref(ri), C.byref(prm), _stream()) == 0
        assert (alone.err_max is not None) == (i == 0)
        for f in _REPORT_FIELDS:
            a, b = getattr(reps[i], f), getattr(alone, f)
            assert (a is None) == (b is None) and (a is None or _bits_equal(a, b)), (i, f)
    assert (reps[1].nonfinite_frames == 0).all() and (reps[1].root_step_max == 0).all()
    assert (reps[0].err_max[2] > 0).all() and (reps[2].dof_step_max[3] > 0).any()  # the 65-frame clips were really measured


# ------------------------------------------------------------------ the refusal table
OFFS = np.array([0, 3, 5], dtype=np.int64)


def _a(*v):
    return np.array(v, dtype=np.int64)


class _Path:
    """One path: its entries, a valid input per member, and how a row is run through the single and the group form."""

    def __init__(self, mr, single, grouped, struct, make, params=None):
        self.mr, self.lib, self.struct, self.make, self.params = mr, mr.group._lib, struct, make, params
        self.single, self.grouped = getattr(self.lib, single), getattr(self.lib, grouped)
        self.n = len(mr.engines)

    def _call(self, fn, handle, arg, prm):
        extra = () if self.params is None else (C.byref(prm if prm is not None else self.params),)
        return fn(handle, arg, *extra, _stream())

    def refused(self, change, rc, msg, prefixed=True, prm=None, forms=("single", "group"), also_member0=None):
        if "single" in forms:
            eng = self.mr.engines[1]
            inp, keep = self.make(eng)
            keep = [keep, change(inp)]
            assert self._call(self.single, eng._h, C.byref(inp), prm) == rc, msg
            assert self.lib.gmr_last_error(eng._h).decode() == msg
        if "group" in forms:
            inputs, keep = (self.struct * self.n)(), []
            for i, eng in enumerate(self.mr.engines):
                inputs[i], k = self.make(eng)
                keep.append(k)
            keep.append(change(inputs[1]))
            if also_member0:
                keep.append(also_member0(inputs[0]))
            assert self._call(self.grouped, self.mr.group._g, inputs, prm) == rc, msg
            assert self.lib.gmr_group_last_error(self.mr.group._g).decode() == ("member 1: " if prefixed else "") + msg
        del keep

    def null_inputs(self):
        eng = self.mr.engines[1]
        assert self._call(self.single, eng._h, None, None) == EINVAL and self.lib.gmr_last_error(eng._h).decode() == "null input"
        assert self._call(self.grouped, self.mr.group._g, None, None) == EINVAL
        assert self.lib.gmr_group_last_error(self.mr.group._g).decode() == "null inputs"
        assert self._call(self.single, None, None, None) == EINVAL and self._call(self.grouped, None, None, None) == EINVAL


def _set(**fields):
    """A row's change: set these fields of the input (arrays by their address; they are kept alive by the caller)."""
    def change(inp):
        for k, v in fields.items():
            setattr(inp, k, v.ctypes.data if isinstance(v, np.ndarray) else v)
        return list(fields.values())
    return change


def _valid_motion(eng):
    q = torch.zeros((5, eng.nq), dtype=torch.float64, device="cuda")
    q[:, 3] = 1.0
    mi, res, k = _motion_input(eng, q, OFFS, True, True, 0.0, None, None)
    return mi, (res, k)


def _valid_track(eng):
    q = torch.zeros((5, eng.nq), dtype=torch.float64, device="cuda")
    q[:, 3] = 1.0
    ti, res, k = _track_input(eng, q, OFFS, FPS_IN, FPS_OUT, None, True)
    return ti, (res, k)


def _valid_report(eng):
    q = torch.zeros((5, eng.nq), dtype=torch.float64, device="cuda")
    q[:, 3] = 1.0
    ri, rep, k = _report_input(eng, q, None, None, None, OFFS, None, None)
    return ri, (rep, k)


def test_epilogue_refusals(group, planar_group):
    p = _Path(group, "gmr_motion_epilogue", "gmr_group_motion_epilogue", _native.MotionInput, _valid_motion)
    p.null_inputs()
    p.refused(_set(n_frames=-1), EINVAL, "negative n_frames")
    for f in ("qpos", "seq_offsets", "root_pos_out", "root_rot_out", "local_body_pos_out", "dof_pos_out"):
        p.refused(_set(**{f: None}), EINVAL, "null argument")
    p.refused(_set(flags=4), EINVAL, "unknown flags")
    p.refused(_set(seq_offsets=_a(0, 3, 4)), EINVAL, "seq_offsets must run from 0 to n_frames")
    p.refused(_set(seq_offsets=_a(1, 3, 5)), EINVAL, "seq_offsets must run from 0 to n_frames")
    p.refused(_set(n_seq=0), EINVAL, "seq_offsets must run from 0 to n_frames")
    p.refused(_set(seq_offsets=_a(0, 4, 2, 5), n_seq=3), EINVAL, "seq_offsets must not decrease")
    # 2^38 frames are 2^32 tiles of 64 (refused before anything reads the frames)
    p.refused(_set(n_frames=2 ** 38, seq_offsets=_a(0, 2 ** 38), n_seq=1), EINVAL, "too many frames for one launch", prefixed=False)
    # two rules at once: the one checked first is reported
    p.refused(_set(n_frames=-1, flags=8), EINVAL, "negative n_frames")
    p.refused(_set(qpos=None, flags=8), EINVAL, "null argument")
    p.refused(_set(seq_offsets=_a(0, 4, 2, 6), n_seq=3), EINVAL, "seq_offsets must run from 0 to n_frames")
    planar = _Path(planar_group, "gmr_motion_epilogue", "gmr_group_motion_epilogue", _native.MotionInput, _valid_motion)
    planar.refused(lambda inp: None, EUNSUPPORTED, "the motion schema needs a free-joint root; a planar base is not supported")
    planar.refused(_set(qpos=None), EUNSUPPORTED, "the motion schema needs a free-joint root; a planar base is not supported")


def test_track_refusals(group, planar_group):
    p = _Path(group, "gmr_motion_track", "gmr_group_motion_track", _native.TrackInput, _valid_track)
    p.null_inputs()
    ratio = FPS_IN / FPS_OUT
    p.refused(_set(n_frames=-1), EINVAL, "negative n_frames")
    for bad in (-1.0, float("nan"), INF):
        p.refused(_set(lowpass_hz=bad), EINVAL, "lowpass_hz must be finite and >= 0")
    for f in ("qpos", "seq_offsets", "out_offsets", "ratio"):
        p.refused(_set(**{f: None}), EINVAL, "null argument")
    for bad in (0.0, -50.0, float("nan"), INF):
        p.refused(_set(fps_out=bad), EINVAL, "fps_out must be positive")
    p.refused(_set(seq_offsets=_a(0, 3, 4)), EINVAL, "seq_offsets must run from 0 to n_frames")
    p.refused(_set(n_seq=0), EINVAL, "seq_offsets must run from 0 to n_frames")
    p.refused(_set(out_offsets=_a(1, 5, 8)), EINVAL, "out_offsets must start at 0")
    p.refused(_set(seq_offsets=_a(0, 4, 2, 5), out_offsets=_a(0, 6, 6, 11), ratio=np.full(3, ratio), n_seq=3), EINVAL, "seq_offsets must not decrease")
    p.refused(_set(out_offsets=_a(0, 5, 4)), EINVAL, "out_offsets must not decrease")
    p.refused(_set(seq_offsets=_a(0, 5, 5), out_offsets=_a(0, 8, 9)), EINVAL, "clip 1 has output frames but no source frames")
    for bad in (0.0, -0.6, float("nan"), INF):
        p.refused(_set(ratio=np.array([ratio, bad])), EINVAL, "ratio (fps_in / fps_out) must be positive")
    fs = np.array([ratio])[0] * FPS_OUT
    p.refused(_set(lowpass_hz=20.0), EINVAL, f"clip 0: lowpass_hz {20.0:.6f} is not below half its frame rate {fs:.6f}")
    p.refused(_set(seq_offsets=_a(0, 0, 5), out_offsets=_a(0, 0, 8), lowpass_hz=15.0), EINVAL,
              f"clip 1: lowpass_hz {15.0:.6f} is not below half its frame rate {fs:.6f}")  # the clip without frames has no rate to break
    # 2^38 output frames are more than 2^31 tiles of 62 (refused before anything reads the frames)
    p.refused(_set(seq_offsets=_a(0, 5), out_offsets=_a(0, 2 ** 38), n_seq=1), EINVAL, "too many frames for one launch", prefixed=False)
    # two rules at once: the one checked first is reported
    p.refused(_set(seq_offsets=_a(0, 4, 2, 5), out_offsets=_a(1, 6, 6, 11), ratio=np.full(3, ratio), n_seq=3), EINVAL, "out_offsets must start at 0")
    p.refused(_set(seq_offsets=_a(0, 4, 2, 5), out_offsets=_a(0, -1, 6, 11), ratio=np.full(3, ratio), n_seq=3), EINVAL, "out_offsets must not decrease")
    p.refused(_set(n_frames=-1, lowpass_hz=-1.0), EINVAL, "negative n_frames")
    planar = _Path(planar_group, "gmr_motion_track", "gmr_group_motion_track", _native.TrackInput, _valid_track)
    planar.refused(lambda inp: None, EUNSUPPORTED, "the tracking export needs a free-joint root; a planar base is not supported")


def test_report_refusals(group):
    prm = _native.ClipReportParams(1e-3, 0, 0)
    p = _Path(group, "gmr_clip_report", "gmr_group_clip_report", _native.ClipReportInput, _valid_report, params=prm)
    p.null_inputs()
    cm = group._cms[1]
    hp, hq, cols = _keypoints(cm, 5, 5)
    n_cols = int(hp.shape[1])
    err_out = torch.zeros((2, 2), dtype=torch.float64, device="cuda")
    kp = dict(human_pos=hp.data_ptr(), human_quat=hq.data_ptr(), slot_col=cols, n_cols=n_cols, in_dtype=_native.GMR_DTYPE_F64)
    p.refused(lambda inp: None, EINVAL, "negative segment_frames", prefixed=False, prm=_native.ClipReportParams(1e-3, -1, 0))
    for bad in (-1.0, float("nan")):
        p.refused(lambda inp: None, EINVAL, "limit_eps must be >= 0", prefixed=False, prm=_native.ClipReportParams(bad, 0, 0))
    p.refused(_set(n_frames=-1), EINVAL, "negative size")
    p.refused(_set(n_seq=-1), EINVAL, "negative size")
    p.refused(_set(n_seq=0), EINVAL, "seq_offsets must run from 0 to n_frames")
    p.refused(_set(seq_offsets=None), EINVAL, "seq_offsets must run from 0 to n_frames")
    p.refused(_set(seq_offsets=_a(0, 3, 4)), EINVAL, "seq_offsets must run from 0 to n_frames")
    p.refused(_set(seq_offsets=_a(1, 3, 5)), EINVAL, "seq_offsets must run from 0 to n_frames")
    p.refused(_set(seq_offsets=_a(0, 4, 2, 5), n_seq=3), EINVAL, "seq_offsets must not decrease")
    p.refused(_set(qpos=None), EINVAL, "null qpos")
    p.refused(_set(err_max_out=err_out.data_ptr()), EINVAL, "the error fields need the human key-points")
    for drop in ("human_quat", "human_pos", "slot_col"):
        p.refused(_set(**dict(kp, **{drop: None})), EINVAL, "the key-points need both arrays, their dtype and slot_col")
    p.refused(_set(**dict(kp, n_cols=0)), EINVAL, "the key-points need both arrays, their dtype and slot_col")
    p.refused(_set(**dict(kp, in_dtype=7)), EINVAL, "the key-points need both arrays, their dtype and slot_col")
    high = cols.copy()
    high[2] = n_cols
    p.refused(_set(**dict(kp, slot_col=high)), EINVAL, f"slot_col[2]={n_cols} outside [0,{n_cols})")
    low = cols.copy()
    low[0] = -1
    p.refused(_set(**dict(kp, slot_col=low)), EINVAL, f"slot_col[0]=-1 outside [0,{n_cols})")
    # one-frame segments: 2^32 frames are more than 2^31 segments; two members of 2^31 - 1 segments are too many together
    one = _native.ClipReportParams(1e-3, 1, 0)
    p.refused(_set(n_frames=2 ** 32, seq_offsets=_a(0, 2 ** 32), n_seq=1), EINVAL, "too many segments for one launch", prm=one)
    most = _set(n_frames=2 ** 31 - 1, seq_offsets=_a(0, 2 ** 31 - 1), n_seq=1)
    p.refused(most, EINVAL, "too many clips for one launch", prefixed=False, prm=one, forms=("group",), also_member0=most)
    # two rules at once: the one checked first is reported
    p.refused(_set(n_frames=-1), EINVAL, "negative segment_frames", prefixed=False, prm=_native.ClipReportParams(1e-3, -1, 0))
    p.refused(_set(seq_offsets=_a(0, 4, 2, 5), n_seq=3, qpos=None), EINVAL, "seq_offsets must not decrease")
    p.refused(_set(**dict(kp, human_quat=None, slot_col=high)), EINVAL, "the key-points need both arrays, their dtype and slot_col")

"""Foot locking (gmr_motion_footlock, Engine.motion_footlock, dataset.lock_feet, dataset.tracking_from_qpos with lock_feet) on the
GPU, against the contract in include/gmr_amd.h restated in numpy (tests/footlock_reference.py) on the inputs of
tests/footlock_inputs.py: clips of 0, 1, 2, 63, 64, 65, 129 and 200 frames, random runs plus the hand-made shapes (a run across the
63 / 64 edge, runs on a clip's first and last frame, two runs meeting at a clip boundary, a gap shorter than 2 W, a run shorter
than min_run), W = 0, C = 1 and C = 2.

Parity of pos, shift and qpos: TOL = 16 x the rounding floor recorded in tests/test_footlock_host.py (float64 against
numpy.longdouble on these inputs: 3.0e-15), far inside the project's by-definition pin of 1e-9.  The kernels evaluate the
contract's operations in its order without contraction; what differs from numpy is the last bit of sin and cos.
Measured on an MI355X: see DESIGN.md 4.13."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import footlock_inputs as fi  # noqa: E402
from tests import footlock_reference as ref  # noqa: E402
from tests import stream_order as so  # noqa: E402
from tests.test_footlock_host import ROUNDING_FLOOR  # noqa: E402
from tests.test_stream_order_host import check_api  # noqa: E402
from tests.util import compiled  # noqa: E402

TOL = min(16 * ROUNDING_FLOOR, 1e-9)
FILL = 0xA5
F64, I32, U8 = torch.float64, torch.int32, torch.uint8
OFFS, N, S = fi.OFFS, fi.N, len(fi.LENS)


def DEV():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _engine(robot=fi.ROBOT):
    from gmr_amd.engine import Engine
    return Engine(compiled("smplx", robot), device=0)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))   # (a copy: the shared inputs are read-only)
    return (t if dtype is None else t.to(dtype)).to(DEV())


def _shapes(rows=N, clips=S, cols=2):
    nq = fi.robot().nq
    return {"qpos": ((rows, nq), F64), "pos": ((rows, cols, 3), F64), "shift": ((rows, cols, 3), F64), "runs": ((clips, cols), I32),
            "locked_frames": ((clips, cols), I32), "shift_max": ((clips, cols), F64), "residual_max": ((clips, cols), F64),
            "limit_frames": ((clips, cols), I32)}


def _sentinel_out(**kw):
    out = {}
    for k, (sh, dt) in _shapes(**kw).items():
        out[k] = torch.empty(sh, dtype=dt, device=DEV())
        if out[k].numel():
            out[k].view(U8).fill_(FILL)
    return out


def _run(qpos, lab, ids, offs=OFFS, out=None, **kw):
    kw.setdefault("blend_frames", fi.W)
    kw.setdefault("min_run", fi.MIN_RUN)
    res = _engine().motion_footlock(_dev(qpos), offs, _dev(lab), ids, out=out, **kw)
    return {k: v.cpu().numpy() for k, v in res.items()}


@functools.lru_cache(maxsize=None)
def _gpu(case):
    """The GPU's answer to a named case of tests/footlock_inputs.py into pre-filled caller-owned outputs: computed once, shared."""
    if case == "main":
        return _run(fi.qpos(), fi.labels(), fi.feet_ids(), out=_sentinel_out())
    if case == "one":
        return _run(fi.qpos(), fi.labels(cols=1), fi.feet_ids(fi.FEET[:1]), out=_sentinel_out(cols=1))
    if case == "w0":
        return _run(fi.qpos(), fi.labels(), fi.feet_ids(), out=_sentinel_out(), blend_frames=0)
    if case == "nan":
        return _run(fi.nan_qpos(), fi.labels(), fi.feet_ids(), out=_sentinel_out())
    q, lab, _ = fi.limit_case()
    return _run(q, lab, fi.feet_ids(fi.FEET[:1]), offs=[0, fi.LIMIT_FRAMES], out=_sentinel_out(rows=fi.LIMIT_FRAMES, clips=1, cols=1))


def _worst(got, want):
    d = np.abs(got - want)
    d[np.isnan(got) & np.isnan(want)] = 0.0
    return float(np.nanmax(d)) if d.size and not np.isnan(d).any() else (0.0 if not d.size else float("inf"))


def _check(got, want, what):
    worst = {}
    for k in ("pos", "shift", "qpos"):
        worst[k] = _worst(got[k], want[k])
    for k in ("shift_max", "residual_max"):
        worst[k] = _worst(got[k], want[k])
    print(f"{what}: worst |GPU - reference|: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()) + f"  (TOL {TOL:.3e})")
    for k in ("runs", "locked_frames", "limit_frames"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k].tolist(), want[k].tolist())
    for k in ("pos", "shift", "qpos", "shift_max", "residual_max"):
        assert worst[k] <= TOL, (what, k, worst[k])


def _bytes(d):
    return {k: np.ascontiguousarray(v).view(np.uint8).reshape(-1) for k, v in d.items()}


def _chain_columns(ids):
    rob = fi.robot()
    paths, chains = ref.paths_and_chains(rob, ids)
    return sorted(int(rob.qpos_adr[p[i]]) for p, c in zip(paths, chains) for i in c)


# ------------------------------------------------------------------ 1: parity, counts, byte equality, outcome
@pytest.mark.parametrize("case", ["main", "one", "w0"])
def test_outputs_equal_the_reference(case):
    got, want = _gpu(case), fi.reference(case)
    _check(got, want, case)
    assert want["runs"].sum() >= 20 and want["locked_frames"].sum() > 200   # the case says something
    assert float(got["residual_max"].max()) <= 1e-6
    assert not got["limit_frames"].any()
    for k in ("runs", "locked_frames", "shift_max", "residual_max", "limit_frames"):   # the clip without frames
        assert not np.any(got[k][0]), k


def test_the_hand_made_runs_are_what_they_were_made_to_be():
    want, got = fi.reference("main"), _gpu("main")
    rl = want["run_list"]
    assert (60, 70) in rl[7][0] and rl[7][1][0] == (0, 5) and rl[7][1][-1] == (190, 199)
    assert rl[5][0][-1] == (60, 64) and rl[6][0][0] == (0, 4)                    # two runs meet at the boundary of clips 5 and 6
    assert (20, 30) in rl[6][1] and (35, 45) in rl[6][1]                         # the gap of four frames
    assert not any(a <= 100 <= b for a, b in rl[6][0])                           # the lone frame is no run
    assert rl[1][0] == [] and rl[2][0] == [(0, 1)] and got["runs"][1, 0] == 0 and got["runs"][2].tolist() == [1, 1]
    a6, a7 = int(OFFS[6]), int(OFFS[7])
    sh = got["shift"]
    assert np.abs(sh[a7 + 55:a7 + 60, 0, :2]).max(axis=1).min() > 0 and not sh[a7 + 54, 0].any()    # five ramp frames, then none
    assert np.abs(sh[a7 + 71:a7 + 76, 0, :2]).max(axis=1).min() > 0 and not sh[a7 + 76, 0].any()
    assert np.abs(sh[a6 + 31:a6 + 35, 1, :2]).max(axis=1).min() > 0                                # the gap is bridged
    assert not sh[a6 + 100, 0].any()                                                               # the lone frame: no run, no ramp near it
    assert not got["shift"][..., 2].any() and not np.signbit(got["shift"][..., 2]).any()           # z: +0.0 everywhere
    w0 = _gpu("w0")["shift"]
    assert not w0[a7 + 59, 0].any() and not w0[a7 + 71, 0].any() and w0[a7 + 60, 0].any()          # W = 0: no ramp


@pytest.mark.parametrize("case", ["main", "one", "w0"])
def test_everything_outside_the_solved_chain_entries_is_copied_bit_for_bit(case):
    got = _gpu(case)
    q = fi.qpos()
    ids = fi.feet_ids(fi.FEET[:1] if case == "one" else fi.FEET)
    cols = _chain_columns(ids)
    other = [c for c in range(q.shape[1]) if c not in cols]
    assert len(cols) == 6 * len(ids) and set(range(7)) <= set(other)
    assert np.array_equal(np.ascontiguousarray(got["qpos"][:, other]).view(np.uint8), np.ascontiguousarray(q[:, other]).view(np.uint8))
    solved = np.abs(got["shift"]).max(axis=(1, 2)) > 0        # (a solved frame with a shift of exactly zero moves nothing either)
    assert 0 < solved.sum() < N
    assert np.array_equal(np.ascontiguousarray(got["qpos"][~solved]).view(np.uint8), np.ascontiguousarray(q[~solved]).view(np.uint8))
    assert np.abs(got["qpos"][solved] - q[solved]).max() > 1e-5


def test_two_calls_give_identical_bytes():
    again = _run(fi.qpos(), fi.labels(), fi.feet_ids(), out=_sentinel_out())
    for (k, a), b in zip(_bytes(_gpu("main")).items(), _bytes(again).values()):
        assert np.array_equal(a, b), k


def test_without_out_the_call_allocates_the_same_answer():
    res = _run(fi.qpos(), fi.labels(), fi.feet_ids())
    for (k, a), b in zip(_bytes(_gpu("main")).items(), _bytes(res).values()):
        assert np.array_equal(a, b), k


def test_locked_feet_stay_on_their_anchors():
    """With the original labels, every run's foot origins, re-evaluated by Engine.evaluate, lie within 1e-6 m of the anchor in xy."""
    got, want = _gpu("main"), fi.reference("main")
    eng = _engine()
    xpos = eng.evaluate(_dev(got["qpos"]), want_errors=False, want_poses=True)[1].cpu().numpy()
    ids = fi.feet_ids()
    n_runs, worst = 0, 0.0
    for s in range(S):
        a = int(OFFS[s])
        for c in range(2):
            for f, e in want["run_list"][s][c]:
                p0 = want["pos"][a + f:a + e + 1, c, :2]
                anchor = p0.mean(axis=0)
                p1 = xpos[a + f:a + e + 1, ids[c], :2]
                worst = max(worst, float(np.abs(p1 - anchor).max()))
                n_runs += 1
    print(f"{n_runs} runs, worst |foot - anchor| in xy after locking: {worst:.3e} m")
    assert n_runs >= 20 and worst <= 1e-6
    before = eng.evaluate(_dev(fi.qpos()), want_errors=False, want_poses=True)[1].cpu().numpy()
    assert _worst(before[:, ids], want["pos"]) <= 1e-9     # pos_out is what gmr_evaluate reports as xpos


# ------------------------------------------------------------------ 2: limits
def test_a_hinge_on_its_limit_pushed_outward_stays_on_it():
    got, want = _gpu("limit"), fi.reference("limit")
    _check(got, want, "limit")
    q, _, adr = fi.limit_case()
    assert got["limit_frames"][0, 0] > 0 and got["limit_frames"][0, 0] == want["limit_frames"][0, 0]
    assert float(got["qpos"][:, adr].min()) == float(q[0, adr])                   # the hinge does not leave its bound
    assert int((got["qpos"][:, adr] == q[0, adr]).sum()) >= got["limit_frames"][0, 0]
    assert (got["qpos"][:, adr] > q[0, adr]).any()                                # ... and moves inward where it is pulled inward


# ------------------------------------------------------------------ 3: non-finite rows
def test_a_nan_row_is_copied_through_splits_its_run_and_stays_in_its_clip():
    got, want, clean = _gpu("nan"), fi.reference("nan"), _gpu("main")
    _check(got, want, "nan")
    g = int(OFFS[fi.NAN_CLIP]) + fi.NAN_FRAME
    q = fi.nan_qpos()
    assert np.array_equal(got["qpos"][g].view(np.uint8), np.ascontiguousarray(q[g]).view(np.uint8))      # copied through
    assert np.isnan(got["pos"][g]).all() and not got["shift"][g].any()
    rl = want["run_list"][fi.NAN_CLIP]
    assert (60, 64) in rl[0] and (66, 70) in rl[0]                                                       # the run splits
    assert got["runs"][fi.NAN_CLIP, 0] == _gpu("main")["runs"][fi.NAN_CLIP, 0] + 1
    a, b = int(OFFS[fi.NAN_CLIP]), int(OFFS[fi.NAN_CLIP + 1])
    cb, gb = _bytes(clean), _bytes(got)
    for k, (sh, dt) in _shapes().items():   # every output of every other clip: byte for byte the clean run's
        row = int(np.prod(sh[1:])) * torch.empty((), dtype=dt).element_size()
        lo, hi = (a * row, b * row) if k in ("qpos", "pos", "shift") else (fi.NAN_CLIP * row, (fi.NAN_CLIP + 1) * row)
        assert np.array_equal(np.delete(gb[k], np.s_[lo:hi]), np.delete(cb[k], np.s_[lo:hi])), k


def test_rows_outside_every_clip_are_not_written():
    offs = np.array([3, 40, 40, 90], dtype=np.int64)    # rows 0 .. 2 and 90 .. N-1 belong to no clip
    out = _sentinel_out(clips=3)
    got = _run(fi.qpos(), fi.labels(), fi.feet_ids(), offs=offs, out=out)
    want = ref.footlock(fi.robot(), fi.qpos(), offs, fi.labels(), fi.feet_ids(), fi.W, fi.MIN_RUN)
    for k in ("qpos", "pos", "shift"):
        assert bool((out[k][:3].view(U8) == FILL).all()) and bool((out[k][90:].view(U8) == FILL).all()), k
        assert _worst(got[k][3:90], want[k][3:90]) <= TOL, k
    for k in ("runs", "locked_frames"):
        assert np.array_equal(got[k], want[k]), k


# ------------------------------------------------------------------ 4: bad arguments
def test_bad_arguments_are_refused_with_their_code_and_launch_nothing():
    from gmr_amd import engine
    eng = _engine()
    out = _sentinel_out()
    fl, _, keep = engine._footlock_input(eng, _dev(fi.qpos()), OFFS, _dev(fi.labels()), fi.feet_ids(), fi.W, fi.MIN_RUN, 8, 1e-6, 0.2, out)
    fl.stream = torch.cuda.current_stream().cuda_stream
    rob = fi.robot()
    names = list(rob.body_names)

    def ids(*bodies):
        a = np.array([b if isinstance(b, int) else names.index(b) for b in bodies], dtype=np.int32)
        keep.append(a)
        return a.ctypes.data

    bad = [({"n_contact": 0}, -1), ({"n_contact": 9}, -1), ({"n_contact": -1}, -1), ({"blend_frames": -1}, -1), ({"min_run": 0}, -1),
           ({"iterations": 0}, -1), ({"iterations": 33}, -1), ({"damping": 0.0}, -1), ({"damping": np.nan}, -1), ({"step_cap": 0.0}, -1),
           ({"step_cap": np.inf}, -1), ({"body_ids": None}, -1), ({"n_frames": -1}, -1), ({"n_seq": -1}, -1),
           ({"qpos": None}, -1), ({"seq_offsets": None}, -1), ({"contact": None}, -1), ({"qpos_out": None}, -1), ({"pos_out": None}, -1),
           ({"shift_out": None}, -1), ({"qpos_out": fl.qpos}, -1),
           ({"body_ids": ids(fi.feet_ids()[0], rob.nbody)}, -1), ({"body_ids": ids(-1, fi.feet_ids()[1])}, -1),     # out of range
           ({"body_ids": ids(fi.FEET[0], fi.FEET[0])}, -1),                                                     # named twice
           ({"body_ids": ids("left_hip_roll_link", fi.FEET[1])}, -1),                                           # a chain of two hinges
           ({"body_ids": ids(fi.FEET[0], "left_knee_link")}, -1),                                               # the knee's path lies inside the foot's
           ({"body_ids": ids(0, fi.FEET[1])}, -1)]                                                              # the root: no hinge at all
    for change, rc in bad:
        keep_vals = {k: getattr(fl, k) for k in change}
        for k, v in change.items():
            setattr(fl, k, v)
        got = eng._lib.gmr_motion_footlock(eng._h, C.byref(fl))
        msg = eng._lib.gmr_last_error(eng._h)
        for k, v in keep_vals.items():
            setattr(fl, k, v)
        assert got == rc and msg and len(msg) > 5, (change, got, msg)
    for change in ({"n_frames": 0}, {"n_seq": 0}):   # nothing to do: GMR_OK, and no launch either
        keep_vals = {k: getattr(fl, k) for k in change}
        for k, v in change.items():
            setattr(fl, k, v)
        assert eng._lib.gmr_motion_footlock(eng._h, C.byref(fl)) == 0
        for k, v in keep_vals.items():
            setattr(fl, k, v)
    torch.cuda.synchronize()
    for k, t in out.items():
        assert bool((t.view(U8) == FILL).all()), k
    assert eng._lib.gmr_motion_footlock(eng._h, C.byref(fl)) == 0   # the struct itself was good
    torch.cuda.synchronize()
    assert np.array_equal(out["qpos"].cpu().numpy().view(np.uint8), _gpu("main")["qpos"].view(np.uint8))
    with pytest.raises(ValueError):
        eng.motion_footlock(_dev(fi.qpos()), OFFS, _dev(fi.labels()), [fi.feet_ids()[0], eng.nbody])
    with pytest.raises(ValueError):
        eng.motion_footlock(_dev(fi.qpos()), OFFS, _dev(fi.labels()), fi.feet_ids(), iterations=33)
    with pytest.raises(engine.EngineError, match="contact"):
        eng.motion_footlock(_dev(fi.qpos()), OFFS, _dev(fi.labels(cols=1)), fi.feet_ids())
    with pytest.raises(engine.EngineError, match="gmr_motion_footlock"):
        eng.motion_footlock(_dev(fi.qpos()), OFFS, _dev(fi.labels()), [names.index("left_hip_roll_link"), fi.feet_ids()[1]])
    q = _dev(fi.qpos())
    with pytest.raises(engine.EngineError, match="alias"):
        eng.motion_footlock(q, OFFS, _dev(fi.labels()), fi.feet_ids(), out={**_sentinel_out(), "qpos": q})
    empty = eng.motion_footlock(q[:0], [0, 0, 0], _dev(fi.labels()[:0]), fi.feet_ids())   # no rows: no launch, every clip empty
    assert empty["qpos"].shape == (0, rob.nq) and not empty["runs"].any() and empty["runs"].shape == (2, 2)


def _small_call(eng, body_id, frames=20, qpos=None, run=(5, 14)):
    """A complete, valid one-clip, one-column call on `eng` with every output pre-filled: (struct, outputs by name, keep-alive)."""
    from gmr_amd import _native
    fl = _native.FootlockInput()
    q = torch.zeros((frames, eng.nq), dtype=F64, device=DEV()) if qpos is None else _dev(qpos)
    if qpos is None:
        q[:, 3] = 1.0
    lab = torch.zeros((frames, 1), dtype=U8, device=DEV())
    lab[run[0]:run[1] + 1] = 1
    offs = torch.tensor([0, frames], dtype=torch.int64, device=DEV())
    ids = np.array([body_id], np.int32)
    shapes = {"qpos": ((frames, eng.nq), F64), "pos": ((frames, 1, 3), F64), "shift": ((frames, 1, 3), F64), "runs": ((1, 1), I32),
              "locked_frames": ((1, 1), I32), "shift_max": ((1, 1), F64), "residual_max": ((1, 1), F64), "limit_frames": ((1, 1), I32)}
    out = {}
    for k, (sh, dt) in shapes.items():
        out[k] = torch.empty(sh, dtype=dt, device=DEV())
        out[k].view(U8).fill_(FILL)
        setattr(fl, k + "_out", out[k].data_ptr())
    fl.qpos, fl.seq_offsets, fl.contact, fl.body_ids = q.data_ptr(), offs.data_ptr(), lab.data_ptr(), ids.ctypes.data
    fl.n_frames, fl.n_seq, fl.n_contact, fl.blend_frames, fl.min_run, fl.iterations = frames, 1, 1, fi.W, fi.MIN_RUN, 8
    fl.damping, fl.step_cap = 1e-6, 0.2
    fl.stream = torch.cuda.current_stream().cuda_stream
    return fl, out, [q, lab, offs, ids]


def _refused_without_a_launch(eng, body_id, rc, word):
    fl, out, keep = _small_call(eng, body_id)
    assert eng._lib.gmr_motion_footlock(eng._h, C.byref(fl)) == rc
    msg = eng._lib.gmr_last_error(eng._h)
    assert word in msg, msg
    torch.cuda.synchronize()
    for k, t in out.items():
        assert bool((t.view(U8) == FILL).all()), k


def test_a_planar_base_model_is_unsupported():
    from gmr_amd.engine import Engine
    cm = compiled("smplx", "galaxea_r1pro")
    assert cm.robot.planar_base
    eng = Engine(cm, device=0)
    _refused_without_a_launch(eng, eng.nbody - 1, -3, b"planar")


def test_a_chain_of_more_than_16_hinges_and_a_path_of_more_than_32_bodies_are_unsupported(tmp_path):
    """Synthetic trees (tests/footlock_inputs.py::synthetic_limb): GMR_EUNSUPPORTED, nothing written; a body half way down the long
    limb is accepted by the same handle."""
    from gmr_amd.engine import Engine
    eng = Engine(fi.synthetic_limb(tmp_path, 17, 0, "over_chain"), device=0)
    _refused_without_a_launch(eng, eng.nbody - 1, -3, b"at most 16")
    _refused_without_a_launch(eng, 2, -1, b"at least 3")
    fl, out, keep = _small_call(eng, 10)
    assert eng._lib.gmr_motion_footlock(eng._h, C.byref(fl)) == 0
    torch.cuda.synchronize()
    assert out["runs"].item() == 1 and out["locked_frames"].item() == 10
    eng = Engine(fi.synthetic_limb(tmp_path, 3, 30, "over_path"), device=0)
    _refused_without_a_launch(eng, eng.nbody - 1, -3, b"at most 32")


@pytest.mark.parametrize("hinges,fixed", [(16, 0), (3, 29)], ids=["chain16", "path32"])
def test_the_longest_chain_and_the_longest_path_equal_the_reference(hinges, fixed, tmp_path):
    """At the limits themselves (16 chain hinges: the largest LDS layout of the solve; 32 path bodies: the whole path table) the
    call runs and agrees with the reference within the project's by-definition pin of 1e-9 -- the bound of 16 rounding floors
    was recorded for the G1 inputs and is not claimed for these trees."""
    from gmr_amd.engine import Engine
    cm = fi.synthetic_limb(tmp_path, hinges, fixed, "at_limit")
    rob, frames = cm.robot, 20
    rng = np.random.default_rng(hinges)
    q = np.tile(np.asarray(rob.qpos0, dtype=np.float64), (frames, 1))
    q[:, 7:] = rng.uniform(-0.5, 0.5, rob.nq - 7) + 2e-3 * np.sin(np.arange(frames)[:, None] / 3.0 + rng.uniform(0, 6, rob.nq - 7))
    lab = np.zeros((frames, 1), np.uint8)
    lab[5:15] = 1
    want = ref.footlock(rob, q, [0, frames], lab, [rob.nbody - 1], fi.W, fi.MIN_RUN)
    eng = Engine(cm, device=0)
    fl, out, keep = _small_call(eng, rob.nbody - 1, frames, qpos=q)
    assert eng._lib.gmr_motion_footlock(eng._h, C.byref(fl)) == 0
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    worst = {k: _worst(got[k], want[k]) for k in ("pos", "shift", "qpos", "shift_max", "residual_max")}
    print(f"{hinges} hinges + {fixed} fixed: worst |GPU - reference|: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for k in ("runs", "locked_frames", "limit_frames"):
        assert np.array_equal(got[k], want[k]), k
    assert max(worst.values()) <= 1e-9 and want["runs"][0, 0] == 1 and float(want["shift_max"][0, 0]) > 1e-5
    assert np.array_equal(got["qpos"][:, :7].view(np.uint8), np.ascontiguousarray(q[:, :7]).view(np.uint8))


# ------------------------------------------------------------------ 5: stream order (the entry is outside the 27 of the shared suite)
def test_the_static_stream_check_passes():
    problems, syncs = check_api(entries=["gmr_motion_footlock"])
    assert not problems and syncs == {"gmr_motion_footlock": False}


class FootlockCase(so.Case):
    """The launch of the tests above with everything it reads in two versions: other motion and other labels behind the same
    offsets, the host body ids in the other order, and in the struct another ramp, run length and iteration.  Both are valid."""
    entry, launches, h2d = "gmr_motion_footlock", 3, 0
    struct_values = True

    def __init__(self):
        super().__init__()
        ids = np.array(fi.feet_ids(), np.int32)
        self.dev_in = {"qpos": (_dev(fi.qpos()), _dev(fi.qpos(seed=2))), "seq_offsets": (_dev(OFFS), _dev(OFFS)),
                       "contact": (_dev(fi.labels()), _dev(fi.labels(seed=2, hand_made=False)))}
        self.host_in = {"body_ids": (ids, ids[::-1].copy())}
        self.out_spec = {k + "_out": v for k, v in _shapes().items()}

    def new_struct(self):
        from gmr_amd import _native
        return _native.FootlockInput()

    def fill(self, st, b, decoy):
        for k, t in list(b.dev.items()) + list(b.out.items()):
            setattr(st, k, t.data_ptr())
        st.body_ids = b.host["body_ids"].ctypes.data
        st.n_frames, st.n_seq, st.n_contact = N, S, 2
        st.blend_frames, st.min_run, st.iterations = (3, 3, 6) if decoy else (fi.W, fi.MIN_RUN, 8)
        st.damping, st.step_cap = (1e-4, 0.1) if decoy else (1e-6, 0.2)

    def invoke(self, b, st, stream):
        st.stream = stream.value
        eng = _engine()
        return eng._lib.gmr_motion_footlock(eng._h, C.byref(st))


@functools.lru_cache(maxsize=None)
def _stream_case():
    """(case, serial answers, spin in cycles, spin in ms): the spin is ten times the call's serial time, at least 5 ms."""
    case = FootlockCase()
    ser = so.serial_answers(case, DEV())
    spin_ms = so.spin_ms_for(ser["ms"])
    assert ser["deterministic"], f"two runs on the same inputs differ in {so.differing(ser['true'], ser['true2'])}"
    for k in ("dev_decoy", "host_decoy"):
        assert not so.same(ser[k], ser["true"]), f"the {k} answer equals the true one: the case could not tell an ordering error"
    return case, ser, int(spin_ms / so.calibrate_spin()["ms_per_cycle"]), spin_ms


def test_stream_order_behind_a_late_producer():
    """Issued behind a producer that is still running, with no host synchronisation and its struct and body ids overwritten on
    return, the call computes the serial answer byte for byte, and it returns while the producer is still running."""
    case, ser, cycles, spin_ms = _stream_case()
    want = _gpu("main")
    assert all(np.array_equal(ser["true"][k + "_out"], v) for k, v in _bytes(want).items())   # the serial answer is the tests' answer
    r = so.run_late(case, DEV(), cycles)
    print(f"gmr_motion_footlock: serial {ser['ms']:.3f} ms, spin {spin_ms:.1f} ms, issue took {r['issue_ms']:.3f} ms, "
          f"returned before producer: {r['returned_before_producer']}")
    assert not r["vacuous"], "the producer had finished before the call was issued: the run proves nothing"
    assert so.same(r["answer"], ser["true"]), f"differs from the serial answer in {so.differing(r['answer'], ser['true'])}"
    assert not so.same(r["answer"], ser["dev_decoy"]) and not so.same(r["answer"], ser["host_decoy"])
    assert r["returned_before_producer"]


# ------------------------------------------------------------------ 6: end to end
E2E_FRAMES, E2E_FPS = 120, 50.0


def _jittering_stance():
    """One clip at 50 Hz: the G1 stands with bent knees while its root, and with it both feet, jumps by 1.2 mm in x between
    consecutive frames (0.06 m/s: slow and low, so the contact kernel labels both feet planted throughout)."""
    rob = fi.robot()
    q0 = np.array(rob.qpos0, dtype=np.float64)
    q0[3:7] = [1.0, 0.0, 0.0, 0.0]
    for b in rob.hinge_bodies():
        n = rob.jnt_names[b]
        if "hip_pitch" in n:
            q0[rob.qpos_adr[b]] = -0.4
        elif "knee" in n:
            q0[rob.qpos_adr[b]] = 0.8
        elif "ankle_pitch" in n:
            q0[rob.qpos_adr[b]] = -0.4
    q = np.tile(q0, (E2E_FRAMES, 1))
    q[:, 0] += 6e-4 * (-1.0) ** np.arange(E2E_FRAMES)
    q[:, 1] += 2e-3 * np.sin(np.arange(E2E_FRAMES) / 40.0)
    return torch.from_numpy(q).to(DEV())


def test_tracking_from_qpos_with_lock_feet_removes_the_slide():
    from gmr_amd import GeneralMotionRetargeting, dataset
    g = GeneralMotionRetargeting("smplx", fi.ROBOT, device=0)
    qpos, offs = _jittering_stance(), [0, E2E_FRAMES]
    before = dataset.tracking_from_qpos(g, qpos, offs, E2E_FPS, E2E_FPS, contact_bodies=fi.FEET)[0]
    after = dataset.tracking_from_qpos(g, qpos, offs, E2E_FPS, E2E_FPS, contact_bodies=fi.FEET, lock_feet=True)[0]
    print("slide_step_max before", before["contact_stats"]["slide_step_max"], "after", after["contact_stats"]["slide_step_max"],
          "footlock_stats", {k: v.tolist() for k, v in after["footlock_stats"].items()})
    assert before["contact"].all() and after["contact"].all() and "footlock_stats" not in before
    assert (before["contact_stats"]["slide_step_max"] >= 1e-3).all()
    assert (after["contact_stats"]["slide_step_max"] <= 2e-6).all()
    st = after["footlock_stats"]
    assert set(st) == set(dataset.FOOTLOCK_STATS) and st["runs"].tolist() == [1, 1] and st["locked_frames"].tolist() == [E2E_FRAMES] * 2
    assert (st["residual_max"] <= 1e-6).all() and (st["shift_max"] >= 5e-4).all() and not st["limit_frames"].any()
    assert set(after) - set(before) == {"footlock_stats"}
    assert np.array_equal(after["root_pos"], before["root_pos"]) and np.array_equal(after["root_rot"], before["root_rot"])  # the root is not moved
    locked, stats = dataset.lock_feet(g, qpos, offs, E2E_FPS, fi.FEET)
    assert stats["runs"].cpu().tolist() == [[1, 1]] and np.array_equal(locked[:, :7].cpu().numpy(), qpos[:, :7].cpu().numpy())
    with pytest.raises(ValueError, match="contact_bodies"):
        dataset.tracking_from_qpos(g, qpos, offs, E2E_FPS, E2E_FPS, lock_feet=True)


def test_multi_robot_tracking_from_qpos_locks_each_named_robots_feet():
    from gmr_amd import GeneralMotionRetargeting, MultiRobotRetargeting, dataset
    robots = [fi.ROBOT, "booster_t1"]
    mr = MultiRobotRetargeting("smplx", robots, device=0)
    q1 = torch.from_numpy(np.tile(np.asarray(compiled("smplx", "booster_t1").robot.qpos0, dtype=np.float64), (E2E_FRAMES, 1))).to(DEV())
    qpos, offs = {fi.ROBOT: _jittering_stance(), "booster_t1": q1}, [0, E2E_FRAMES]
    got = mr.tracking_from_qpos(qpos, offs, E2E_FPS, E2E_FPS, contact_bodies={fi.ROBOT: fi.FEET}, lock_feet=True)
    one = dataset.tracking_from_qpos(GeneralMotionRetargeting("smplx", fi.ROBOT, device=0), qpos[fi.ROBOT], offs, E2E_FPS, E2E_FPS,
                                     contact_bodies=fi.FEET, lock_feet=True)[0]
    d = got[fi.ROBOT][0]
    assert "footlock_stats" not in got["booster_t1"][0] and "contact" not in got["booster_t1"][0]
    for k in dataset.TRACK_ARRAYS:
        assert np.array_equal(d[k].view(np.uint8), one[k].view(np.uint8)), k
    for k in dataset.FOOTLOCK_STATS:
        assert np.asarray(d["footlock_stats"][k]).tobytes() == np.asarray(one["footlock_stats"][k]).tobytes(), k
    assert (d["contact_stats"]["slide_step_max"] <= 2e-6).all()
    mr.close()

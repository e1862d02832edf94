"""gmr_motion_transitions on the GPU against the numpy restatement (tests/transitions_reference.py; inputs:
tests/transitions_inputs.py).

`points` go through sin / cos of two libms: they are held to the bound the self-collision tests hold the same poses' clearances to
(self_collision_reference.bound: ten times the numpy FK's own measured distance to 50 digits).  Everything behind the points is bit
for bit: fed the kernel's own points, the restatement must give the bytes of `moments`, `cost_out`, `best_cost` and `best_frame`.
Nothing in a bound was measured on a kernel."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gmr_amd import transitions as tr  # noqa: E402
from gmr_amd.compose import ComposePlan, Segment  # noqa: E402
from tests import compose_reference as CR  # noqa: E402
from tests import self_collision_reference as SR  # noqa: E402
from tests import transitions_inputs as ti  # noqa: E402
from tests import transitions_reference as TR  # noqa: E402
from tests.test_gpu_dynamics import DEV, _bytes, _dev, engine  # noqa: E402

F64, I32, U8 = torch.float64, torch.int32, torch.uint8
G1, K1 = "unitree_g1", "booster_k1"
EINVAL, EUNSUPPORTED = -1, -3
NAMES = ("points", "moments", "best_cost", "best_frame", "cost_out")


def sentinel_out(n_rows, P, E, D, NT):
    shapes = {"points": ((n_rows, P, 3), F64), "moments": ((n_rows, 6), F64), "best_cost": ((E, D), F64), "best_frame": ((E, D), I32),
              "cost_out": ((E, NT), F64)}
    out = {k: torch.empty(sh, dtype=dt, device=DEV()) for k, (sh, dt) in shapes.items()}
    for t in out.values():
        if t.numel():
            t.view(U8).fill_(ti.FILL)
    return out


def run(robot, q, offs, ids, w, L, src=None, dst=None, stride=1, min_gap=0):
    """One dense call into pre-filled caller-owned outputs: (host arrays by name, the MotionTransitions)."""
    src_c, so, dst_c, do = ti.tables(offs, L, src, dst, stride)
    out = sentinel_out(q.shape[0], len(ids), int(so[-1]), len(dst_c), int(do[-1]))
    mt = engine(robot).motion_transitions(_dev(q), offs, ids, w, L, src, dst, stride, min_gap, dense=True, out=out)
    assert all(mt[k] is out[k] for k in NAMES)
    assert np.array_equal(mt.src_offsets, so) and np.array_equal(mt.dst_offsets, do)
    return {k: t.cpu().numpy() for k, t in mt.items()}, mt


def check(robot, q, offs, ids, w, L, src=None, dst=None, stride=1, min_gap=0):
    """The comparison every case gets; returns (host arrays, MotionTransitions)."""
    got, mt = run(robot, q, offs, ids, w, L, src, dst, stride, min_gap)
    what = f"{robot} L {L} P {len(ids)} stride {stride} min_gap {min_gap}"
    # 1: the points against the restated FK
    ref = TR.points(ti.model(robot), q, offs, ids)
    err = float(np.abs(got["points"] - ref).max()) if ref.size else 0.0
    print(f"{what}: |points - numpy FK| {err:.2e} of {SR.bound(robot):.0e}, {got['best_cost'].shape[0]} sources x {got['cost_out'].shape[1]} targets")
    assert err <= SR.bound(robot), what
    # 2: fed the kernel's own points, the restatement gives the kernel's bytes
    mom = TR.moments(got["points"], mt.weights, offs, L)
    wr = ti.written_moments(offs, q.shape[0], L)
    assert np.array_equal(_bytes(got["moments"][wr]), _bytes(mom[wr])), what
    assert np.all(_bytes(got["moments"][~wr]) == ti.FILL), what                              # and nothing else is written
    dense, best, frame = TR.search(got["points"], mt.weights, offs, L, mt.src_clips, mt.src_offsets, stride, mt.dst_clips, mt.dst_offsets, min_gap)
    bad = np.argwhere(got["cost_out"].view(np.int64) != dense.view(np.int64))
    assert bad.size == 0, f"{what}: {len(bad)} costs differ from the restatement, first (source, target) {bad[:6].tolist()}"
    assert np.array_equal(_bytes(got["best_cost"]), _bytes(best)) and np.array_equal(got["best_frame"], frame), what
    # 3: the reduction is the row-wise first minimum of the dense matrix
    b2, f2 = TR.best_of_dense(got["cost_out"], offs, L, mt.src_clips, mt.src_offsets, stride, mt.dst_clips, mt.dst_offsets, min_gap, q.shape[0])
    assert np.array_equal(_bytes(got["best_cost"]), _bytes(b2)) and np.array_equal(got["best_frame"], f2), what
    assert got["best_frame"].dtype == np.int32 and not np.isnan(got["cost_out"]).any() and (got["cost_out"] >= 0.0).all()
    return got, mt


@functools.lru_cache(maxsize=None)
def main_case(robot, L):
    """The main comparison's answer, computed and checked once, shared and read-only."""
    q, offs = ti.library(robot, L)
    ids, w = ti.all_bodies(robot)
    got, mt = check(robot, q, offs, ids, w, L, min_gap=L)
    for a in got.values():
        a.setflags(write=False)
    return got, mt


# ------------------------------------------------------------------ the main comparison
@pytest.mark.parametrize("L", ti.WINDOWS)
@pytest.mark.parametrize("robot", ti.ROBOTS)
def test_points_costs_and_the_reduction_equal_the_restatement(robot, L):
    got, mt = main_case(robot, L)
    lens = ti.lens(L)
    assert np.diff(mt.src_offsets).tolist() == [max(n - L + 1, 0) for n in lens] == np.diff(mt.dst_offsets).tolist()
    assert len(ti.all_bodies(robot)[0]) == {G1: 38, K1: 23}[robot] and abs(mt.weights.sum() - 1.0) <= 4 * TR.EPS
    bf, bc = got["best_frame"], got["best_cost"]
    for b, n in enumerate(lens):                                                            # a clip shorter than the window has no target frame
        assert (n >= L) or (np.all(bf[:, b] == -1) and np.all(bc[:, b] == np.inf))
    # the same clip on both sides: the excluded band is +inf in the dense matrix and never the best frame
    a = 8
    u0, c0 = int(mt.src_offsets[a]), int(mt.dst_offsets[a])
    i = np.arange(130 - L + 1)
    assert np.all(np.abs(bf[u0:u0 + i.size, a] - i) >= L)
    assert np.all(got["cost_out"][u0 + i, c0 + i] == np.inf) and np.isfinite(got["cost_out"][u0, c0 + L])
    again, _ = run(robot, *ti.library(robot, L), *ti.all_bodies(robot), L, min_gap=L)
    assert all(np.array_equal(_bytes(again[k]), _bytes(got[k])) for k in NAMES)              # two calls: identical bytes


# ------------------------------------------------------------------ the other cases
@pytest.mark.parametrize("robot,L,stride", [(G1, 8, 3), (K1, 2, 3), (G1, 1, 3)])
def test_a_source_stride(robot, L, stride):
    q, offs = ti.library(robot, L)
    got, mt = check(robot, q, offs, *ti.all_bodies(robot), L, stride=stride, min_gap=L)
    assert np.diff(mt.src_offsets).tolist() == [tr.source_count(n, L, stride) for n in ti.lens(L)]
    full = main_case(robot, L)[0]                                                           # every third source of the full search, bit for bit
    for a in range(9):
        u, v = int(mt.src_offsets[a]), int(mt.src_offsets[a + 1])
        f0 = int(main_case(robot, L)[1].src_offsets[a])
        assert np.array_equal(_bytes(got["cost_out"][u:v]), _bytes(full["cost_out"][f0:f0 + (v - u) * stride:stride]))


@pytest.mark.parametrize("robot,ids,w", [(G1, [37], [2.0]), (K1, [0], [1.0]), (G1, [3, 20, 11], [1.0, 1.0, 1.0]), (K1, [22, 0, 9], [0.2, 0.5, 0.3]),
                                         (G1, [5, 9, 30, 31], [0.7, 0.0, 0.1, 0.2]), (K1, list(range(23)), [0.0] + [1.0 + 0.1 * k for k in range(22)])])
def test_one_point_three_points_unequal_weights_and_a_zero_weight(robot, ids, w):
    q, offs = ti.library(robot, 8)
    got, mt = check(robot, q, offs, np.asarray(ids, np.int32), np.asarray(w), 8, min_gap=8)
    assert mt.weights.tolist() == (np.asarray(w) / np.asarray(w).sum()).tolist()
    if len(ids) == 1:                                                                       # one point, one frame per window: only the heights differ
        one, _ = check(robot, *ti.library(robot, 1), np.asarray(ids, np.int32), np.asarray(w), 1)
        z = one["points"][:, 0, 2]
        assert np.abs(one["cost_out"] - (z[:, None] - z[None, :]) ** 2).max() <= TR.bound(1, 1, float(np.abs(one["points"][..., :2]).max()) * 2 ** 0.5)


@pytest.mark.parametrize("L", [9, 32])
def test_windows_that_take_the_long_ring(L):
    q, offs = ti.library(K1, L)
    check(K1, q, offs, *ti.all_bodies(K1), L, min_gap=3)
    check(G1, *ti.library(G1, L), np.asarray([0, 16, 29], np.int32), np.ones(3), L, stride=5, min_gap=L)


@pytest.mark.parametrize("robot", ti.ROBOTS)
def test_min_gap_zero_and_larger_than_every_clip(robot):
    L = 8
    q, offs = ti.library(robot, L)
    ids, w = ti.all_bodies(robot)
    got, mt = check(robot, q, offs, ids, w, L, min_gap=0)
    for a, n in enumerate(ti.lens(L)):                                                      # nothing is excluded: a window's best match in its own clip is itself
        u0, u1 = int(mt.src_offsets[a]), int(mt.src_offsets[a + 1])
        assert np.all(got["best_cost"][u0:u1, a] == 0.0)                                     # exactly: D = V bit for bit, C = Z = 0
        assert np.all(np.abs(got["best_frame"][u0:u1, a] - np.arange(u1 - u0)) <= 1)         # (itself, or a neighbour that also rounds to the bound)
    same = [5, 8]
    got, mt = check(robot, q, offs, ids, w, L, src=same, dst=same, min_gap=1000)
    assert np.all(got["best_frame"][:, 0][:56] == -1) and np.all(got["best_cost"][:56, 0] == np.inf)      # every pair of the clip with itself
    assert np.all(got["best_frame"][56:, 1] == -1) and np.all(got["best_frame"][:56, 1] >= 0) and np.all(got["best_frame"][56:, 0] >= 0)
    assert np.all(got["cost_out"][:56, :56] == np.inf) and np.all(got["cost_out"][56:, 56:] == np.inf) and np.isfinite(got["cost_out"][:56, 56:]).all()


def test_a_tie_reports_the_lower_frame():
    """A target clip made of the same rows twice: frame j and frame j + T see the same points, bit for bit."""
    L, T = 8, 40
    q, offs = ti.library(G1, L)
    a = int(offs[8])
    lib = np.concatenate([q[int(offs[6]):int(offs[7])], q[a:a + T], q[a:a + T]])
    lo = np.array([0, 64, 64 + 2 * T], np.int64)
    got, mt = check(G1, lib, lo, *ti.all_bodies(G1), L, src=[0], dst=[1])
    n = T - L + 1
    cost = got["cost_out"]
    assert cost.shape == (57, 2 * T - L + 1) and np.array_equal(_bytes(cost[:, :n]), _bytes(cost[:, T:T + n]))
    bf = got["best_frame"][:, 0]
    assert not np.any((bf >= T) & (bf < T + n)) and np.any(bf < n)                          # never the second copy of a frame
    rev, _ = check(G1, np.concatenate([lib[64:], lib[:64]]), np.array([0, 2 * T, 2 * T + 64], np.int64), *ti.all_bodies(G1), L, src=[1], dst=[0])
    assert np.array_equal(_bytes(rev["cost_out"]), _bytes(cost))                             # where the clips lie in the library changes nothing


@pytest.mark.parametrize("robot", ti.ROBOTS)
def test_source_clips_that_are_no_target_clips_and_the_reverse(robot):
    L = 8
    q, offs = ti.library(robot, L)
    got, mt = check(robot, q, offs, *ti.all_bodies(robot), L, src=[8, 5, 2, 4], dst=[6, 0, 8, 3, 7], min_gap=L)
    full, fm = main_case(robot, L)
    for a, ca in enumerate([8, 5, 2, 4]):
        for b, cb in enumerate([6, 0, 8, 3, 7]):
            rows = slice(int(mt.src_offsets[a]), int(mt.src_offsets[a + 1]))
            frows = slice(int(fm.src_offsets[ca]), int(fm.src_offsets[ca + 1]))
            assert np.array_equal(_bytes(got["best_cost"][rows, b]), _bytes(full["best_cost"][frows, cb])), (ca, cb)
            assert np.array_equal(got["best_frame"][rows, b], full["best_frame"][frows, cb]), (ca, cb)


def test_the_result_does_not_depend_on_the_launch_geometry():
    names = ("GMR_AMD_TRANSITIONS_WAVES", "GMR_AMD_TRANSITIONS_TILE")
    old = {k: os.environ.get(k) for k in names}
    try:
        for robot, L in ((G1, 8), (K1, 2)):
            base = main_case(robot, L)[0]
            for waves, tile in (("1", None), ("3", "7"), (None, "1"), ("2", "200"), ("40", "64")):   # one wavefront does it all; tiles across clips
                for k, v in zip(names, (waves, tile)):
                    os.environ.pop(k, None)
                    if v is not None:
                        os.environ[k] = v
                got, _ = run(robot, *ti.library(robot, L), *ti.all_bodies(robot), L, min_gap=L)
                for k in NAMES:
                    assert np.array_equal(_bytes(got[k]), _bytes(base[k])), (robot, L, waves, tile, k)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


# ------------------------------------------------------------------ the case that fails without the feature
@pytest.mark.parametrize("robot", ti.ROBOTS)
def test_a_clip_cut_in_two_is_found_and_composes_back(robot):
    """X[0:80] and X[60:130], the second turned by 1 rad and shifted by (3, -2).  The deviation of the composed clip from X is held to
    four times what the numpy restatement of the composition shows on this very plan (the existing reproduction test's rule)."""
    from gmr_amd import GeneralMotionRetargeting, dataset
    L = 8
    X, lib, offs = ti.cut_library(robot)
    ids, w = ti.all_bodies(robot)
    got, mt = check(robot, lib, offs, ids, w, L, min_gap=L)
    R = float(np.sqrt((got["points"][..., :2] ** 2).sum(-1)).max())
    bound = TR.bound(len(ids), L, R)
    i = np.arange(60, 73)
    print(f"{robot}: best_cost on the diagonal {got['best_cost'][i, 1].max():.2e}, bound {bound:.2e} (R {R:.2f} m); off it at least "
          f"{np.delete(got['best_cost'][:, 1], i).min():.2e}")
    assert np.array_equal(got["best_frame"][i, 1], i - 60) and np.all(got["best_cost"][i, 1] <= bound)
    g = GeneralMotionRetargeting("smplx", robot, device=0, verbose=False)
    trans, bc, bf = dataset.find_transitions(g, _dev(lib), offs, window=L, src_clips=[0], dst_clips=[1], threshold=bound)
    assert np.array_equal(_bytes(bc), _bytes(got["best_cost"][:73, 1:2])) and np.array_equal(bf, got["best_frame"][:73, 1:2])
    assert trans and all(t.src_clip == 0 and t.dst_clip == 1 and t.dst_frame == t.src_frame - 60 and 60 <= t.src_frame <= 72 for t in trans)
    both, _, _ = dataset.find_transitions(g, _dev(lib), offs, window=L, threshold=bound)     # all clips: the same diagonal, from either side
    assert both and all((t.src_clip, t.dst_clip, t.dst_frame - t.src_frame) in ((0, 1, -60), (1, 0, 60)) for t in both)
    t = trans[0]
    seqs = [[Segment(0, 0, t.src_frame + L), Segment(1, t.dst_frame, 70 - t.dst_frame)]]
    out, out_offs, _ = dataset.compose_clips(g, _dev(lib), offs, seqs, blend=L)
    assert out_offs.tolist() == [0, 130]
    d_ref = float(np.abs(CR.compose(ComposePlan(offs, seqs, L), np.array(lib))[0] - X).max())
    d = float(np.abs(out.cpu().numpy() - X).max())
    print(f"{robot}: |composed - X| {d:.3e}, the restatement's {d_ref:.3e}")
    assert d <= 4.0 * d_ref


# ------------------------------------------------------------------ no work, the refusals
def _struct(robot, q, offs, ids, w, L, out, stride=1, min_gap=0):
    from gmr_amd import _native
    eng = engine(robot)
    src, so, dst, do = ti.tables(offs, L, None, None, stride)
    keep = {"qpos": q, "seq_offsets": _dev(offs), "body_ids": _dev(np.asarray(ids, np.int32)), "weights": _dev(np.asarray(w, np.float64)),
            "src_clips": _dev(src), "src_offsets": _dev(so), "dst_clips": _dev(dst), "dst_offsets": _dev(do)}
    st = _native.TransitionsInput()
    for k, t in list(keep.items()) + list(out.items()):
        setattr(st, k, t.data_ptr())
    st.n_frames, st.n_seq, st.n_bodies, st.window, st.src_stride, st.min_gap = int(q.shape[0]), len(offs) - 1, len(ids), L, stride, min_gap
    st.n_src_clips, st.n_dst_clips, st.n_sources, st.n_targets = len(src), len(dst), int(so[-1]), int(do[-1])
    st.stream = torch.cuda.current_stream(DEV()).cuda_stream
    return eng, st, keep


def test_no_work_returns_without_a_launch_and_every_refusal_returns_its_code():
    L = 8
    qh, offs = ti.library(K1, L)
    ids, w = ti.all_bodies(K1)
    w = w / w.sum()
    q = _dev(qh)
    _, so_, _, do_ = ti.tables(offs, L)
    out = sentinel_out(q.shape[0], len(ids), int(so_[-1]), 9, int(do_[-1]))
    call = lambda eng, st: eng._lib.gmr_motion_transitions(eng._h, C.byref(st))   # noqa: E731
    eng, st, keep = _struct(K1, q, offs, ids, w, L, out, min_gap=L)
    assert call(eng, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bytes(out["cost_out"].cpu().numpy()), _bytes(main_case(K1, L)[0]["cost_out"]))   # the raw call is the engine's call
    for t in out.values():
        t.view(U8).fill_(ti.FILL)
    sets = lambda name, v: (lambda s: setattr(s, name, v))                        # noqa: E731
    cases = [(sets(k, None), EINVAL, "null") for k in ("qpos", "seq_offsets", "body_ids", "weights", "src_clips", "src_offsets", "dst_clips",
                                                        "dst_offsets", "points", "moments", "best_cost", "best_frame")] \
        + [(sets(k, -1), EINVAL, "negative") for k in ("n_frames", "n_seq", "n_src_clips", "n_dst_clips", "n_sources", "n_targets")] \
        + [(sets("window", 0), EINVAL, "window"), (sets("src_stride", 0), EINVAL, "src_stride"), (sets("n_bodies", 0), EINVAL, "n_bodies"),
           (sets("min_gap", -1), EINVAL, "min_gap"), (sets("window", 33), EUNSUPPORTED, "window"), (sets("n_bodies", 65), EUNSUPPORTED, "bodies")]
    for edit, code, text in cases:
        eng, st, keep = _struct(K1, q, offs, ids, w, L, out)
        edit(st)
        assert call(eng, st) == code and text in eng._lib.gmr_last_error(eng._h).decode(), text
    eng, st, keep = _struct(K1, q, offs, ids, w, L, out)                                    # dst_offsets is needed for cost_out only
    st.dst_offsets = st.cost_out = None
    assert call(eng, st) == 0
    torch.cuda.synchronize()
    ref0, _ = run(K1, qh, offs, *ti.all_bodies(K1), L)                                       # (the engine normalises the weights itself)
    assert np.array_equal(_bytes(out["best_cost"].cpu().numpy()), _bytes(ref0["best_cost"])) and np.array_equal(out["best_frame"].cpu().numpy(), ref0["best_frame"])
    assert bool((out["cost_out"].view(U8) == ti.FILL).all())
    for t in out.values():
        t.view(U8).fill_(ti.FILL)
    for field in ("n_frames", "n_seq", "n_src_clips", "n_dst_clips", "n_sources"):           # no work: GMR_OK without a launch, NULL arrays and all
        eng, st, keep = _struct(K1, q, offs, ids, w, L, out)
        setattr(st, field, 0)
        st.qpos = st.seq_offsets = st.src_clips = st.dst_clips = st.points = st.best_cost = None
        assert call(eng, st) == 0
    e = engine(K1)
    none = e.motion_transitions(q, offs, ids, w, L, src_clips=[0, 1, 2], dst_clips=None)      # and through the Python layer: no clip has a window
    assert tuple(none["best_cost"].shape) == (0, 9) and tuple(none["points"].shape) == (q.shape[0], len(ids), 3)
    short = e.motion_transitions(q, offs, ids, w, L, src_clips=[5], dst_clips=[1, 2])         # targets without a frame: +inf and -1 from the kernel
    torch.cuda.synchronize()
    assert bool((short["best_frame"] == -1).all()) and bool(torch.isinf(short["best_cost"]).all()) and tuple(short["best_cost"].shape) == (56, 2)
    assert all(bool((t.view(U8) == ti.FILL).all()) for t in out.values())                     # none of them wrote a byte of these
    assert bool(torch.equal(q.cpu(), torch.from_numpy(np.array(qh))))
    # the Python layer refuses the same before the library is called
    from gmr_amd.engine import EngineError
    with pytest.raises(EngineError, match="qpos"):
        e.motion_transitions(q[:, :-1], offs, ids, w, L)
    with pytest.raises(EngineError, match="out must map"):
        e.motion_transitions(q, offs, ids, w, L, out={k: v for k, v in out.items() if k != "moments"}, dense=True)
    for bad in (dict(body_ids=[0, 99], weights=[1, 1]), dict(body_ids=[0, 1], weights=[1, -1]), dict(body_ids=[0, 1], weights=[0, 0]),
                dict(body_ids=[0, 1], weights=[1]), dict(body_ids=[], weights=[])):
        with pytest.raises(ValueError):
            e.motion_transitions(q, offs, bad["body_ids"], bad["weights"], L)
    with pytest.raises(ValueError):
        e.motion_transitions(q, offs, ids, w, L, min_gap=-1)
    with pytest.raises(EngineError, match="window"):
        e.motion_transitions(q, offs, ids, w, 33)

"""tests/nonfinite_cases.py checked on the host: the dependency sets written from the contract agree with the predictor built on the
oracle, the poison values are what they claim after every conversion, the frame positions are where they claim, and nothing but
data is ever poisoned.  No GPU."""
import numpy as np
import pytest

from tests import nonfinite_cases as NF

ROBOTS2 = ["unitree_g1", "unitree_g1_with_hands"]   # the epilogue and the tracking export also on the largest LDS image


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _agree(call, case, dep, clean, pred):
    """Outside the set the predictor gives the clean bytes; inside it the predicted mask is the whole set, unless the output has a
    named exception -- then it is a part of the set.  Returns the predicted masks."""
    assert dep.keys() == clean.keys() == pred.keys()
    masks = {}
    for k in dep:
        d, m = dep[k], NF.nonfinite(pred[k])
        assert d.shape == m.shape, (call, case, k)
        assert np.array_equal(_bits(pred[k])[~d], _bits(clean[k])[~d]), (call, case, k, "the predictor left the set")
        exc = NF.exception_for(call, case, k)
        if exc is None:
            assert m[d].all(), (call, case, k, "a finite value inside the set", int((~m[d]).sum()))
        else:
            assert exc in NF.EXCEPTIONS
        masks[k] = m
    return masks


def test_poison_values_keep_their_sign_through_every_conversion():
    for name in NF.VALUES:
        v64, v32 = NF.value64(name), NF.value32(name)
        neg = name.startswith("-")
        assert np.isnan(v64) == np.isnan(v32) == name.endswith("nan") and np.isinf(v64) == np.isinf(v32) == name.endswith("inf")
        assert bool(np.signbit(v64)) == bool(np.signbit(v32)) == neg
        q = NF.poisoned_qpos("unitree_g1", NF.Case(name, "root_z", 5))
        assert bool(np.signbit(q[5, 2])) == neg and int(_bits(q)[5, 2]) == NF.BITS64[name]
        rp, rr, dof = NF.fk_inputs(q)   # numpy's float64 -> float32, the only conversion the tests apply
        assert bool(np.signbit(rp[5, 2])) == neg and np.isnan(rp[5, 2]) == np.isnan(v64) and np.isinf(rp[5, 2]) == np.isinf(v64)
        for coord in ("root_qw", "first_hinge"):
            q = NF.poisoned_qpos("unitree_g1", NF.Case(name, coord, 5))
            rp, rr, dof = NF.fk_inputs(q)
            got = rr[5, 3] if coord == "root_qw" else dof[5, 0]
            assert bool(np.signbit(got)) == neg and not np.isfinite(got)
            assert bool(np.signbit(q[:, [4, 5, 6, 3]][5, 3] if coord == "root_qw" else q[:, 7:][5, 0])) == neg
        x = NF.kin_poisoned("unitree_g1", "dof_to_rot", NF.OwnCase(name, (0,), 5))
        assert int(_bits(x)[5, 0]) == NF.BITS32[name]
    torch = pytest.importorskip("torch")   # the upload is a byte copy
    q = NF.poisoned_qpos("unitree_g1", NF.Case("-nan", "root_z", 5))
    assert np.array_equal(_bits(torch.from_numpy(q).clone().numpy()), _bits(q))
    assert np.array_equal(_bits(torch.from_numpy(NF.f32(q)).clone().numpy()), _bits(NF.f32(q)))


def test_frame_positions_are_what_they_say():
    offs, fr, T = NF.OFFS, NF.FRAMES, NF.TILE
    lens = np.diff(offs)
    assert offs[0] == 0 and (lens == 0).any() and (lens == 1).any() and 250 <= NF.N <= 350
    assert all(o % T for o in offs[1:])   # every clip end is off the tile
    a, b = offs[-2], offs[-1]
    whole = [t for t in range(NF.N // T + 1) if a <= t * T and (t + 1) * T <= b]
    assert len(whole) >= 2 and (b - 1) // T - a // T + 1 >= 3   # one clip over three or more tiles, two of them whole
    assert fr["first_of_all"] == 0 == offs[NF.clip_of(0)]
    s = NF.clip_of(fr["one_frame_clip"])
    assert offs[s + 1] - offs[s] == 1
    s = NF.clip_of(fr["clip_first"])
    assert offs[s] == fr["clip_first"] and (offs[s + 1] - 1) // T > fr["clip_first"] // T   # its clip goes on in the next tile
    s = NF.clip_of(fr["before_boundary"])
    assert offs[s + 1] - 1 == fr["before_boundary"] and fr["after_boundary"] == offs[s + 1] == offs[NF.clip_of(fr["after_boundary"])]
    assert fr["before_boundary"] // T == fr["after_boundary"] // T and fr["after_boundary"] % T   # the boundary lies inside a tile
    assert fr["lane63"] % T == T - 1 and fr["lane0"] == fr["lane63"] + 1 and fr["lane63"] // T in whole and fr["lane0"] // T in whole
    s = NF.clip_of(fr["middle"])
    assert offs[s] < fr["middle"] < offs[s + 1] - 1 and 0 < fr["middle"] % T < T - 1
    assert fr["last_of_all"] == NF.N - 1 and NF.N % T   # the last tile has dead lanes
    assert NF.clip_of(offs[1]) == 2   # the empty clip holds no frame
    # every frame position carries root z as +NaN and -NaN, every coordinate every value somewhere, every NaN its twin
    tab = set(NF.TABLE)
    assert all(NF.Case(v, "root_z", f) in tab for f in fr.values() for v in ("+nan", "-nan"))
    assert {(c.value, c.coord) for c in tab} == {(v, c) for v in NF.VALUES for c in NF.COORDS}
    assert all(NF.Case("-" + c.value[1:], c.coord, c.frame) in tab for c in tab if c.value[0] == "+")
    assert NF.Case("+nan", "root_x", fr["clip_first"]) in tab   # ROOT_ORIGIN's frame
    t = NF.robot_tree("unitree_g1")
    j0, j1 = t.dof_body[0], t.dof_body[t.cols["leaf_hinge"] - 7]
    assert t.below[j0][t.dof_body].any() and t.below[j1].any() and not t.below[j1][t.dof_body].any() and t.parent[j0] == 0


@pytest.mark.parametrize("rate", list(NF.TRACK_RATES))
def test_tracking_positions_sit_on_the_tile_edges_and_halos(rate):
    p, fr, W = NF.plan(rate), NF.track_frames(rate), NF.TRACK_TILE
    assert p.M > W   # more than one tile
    edges = NF.track_edges(rate)
    assert len(edges) >= 1
    clip = np.searchsorted(p.out_offs, np.arange(p.M), side="right") - 1
    for n, g in enumerate(edges):
        assert g % W == W - 1 and (g + 1) % W == 0 and clip[g] == clip[g + 1]   # a tile edge inside a clip
        for name, k, nb in ((f"edge{n}_last", g, g + 1), (f"edge{n}_first", g + 1, g)):
            reads = NF.track_reads(rate, fr[name])
            assert reads[k]   # the central lane on the tile's edge reads the frame ...
            assert p.km[nb] == k or p.kp[nb] == k   # ... and is the halo lane of the neighbouring tile, whose difference reads it
            assert nb // W != k // W
    tab = set(NF.track_table(rate))
    assert all(NF.Case(v, "root_z", f) in tab for f in fr.values() for v in ("+nan", "-nan"))
    # the plan itself: weights in [0, 1), rows inside their clips, copies where the contract says
    assert ((p.a >= 0) & (p.a < 1)).all() and (p.src1 - p.src0 <= 1).all() and (p.src0 <= p.src1).all()
    assert ((p.a == 0) | (p.src1 == p.src0 + 1)).all()
    # 30 -> 50 blends two frames in most rows; 120 -> 30 copies every fourth frame and never reads the others
    assert (p.a > 0).any() == (rate == "30to50")
    read = [NF.track_reads(rate, f).any() for f in fr.values()]
    assert any(read) and (all(read) or rate == "120to30")


def test_only_data_is_poisoned():
    """No layout, offset, plan, rate or ratio array ever holds a non-finite value: the cases poison one element of a data array."""
    assert NF.OFFS.dtype == np.int64 and np.isfinite(NF.GROUND)
    for rate in NF.TRACK_RATES:
        p = NF.plan(rate)
        for a in (p.out_offs, p.ratio, p.src0, p.src1, p.a, p.km, p.kp, p.h, np.array([p.fps_in, p.fps_out])):
            assert np.isfinite(np.asarray(a, dtype=np.float64)).all()
        assert (p.ratio > 0).all() and p.out_offs[0] == 0 and (np.diff(p.out_offs) >= 0).all()
    for robot in ROBOTS2:
        clean = NF.clean_qpos(robot)
        assert np.isfinite(clean).all() and np.isfinite(NF.fitted_shape(robot)).all()
        for case in NF.TABLE + NF.track_table("30to50") + NF.track_table("120to30"):
            q = NF.poisoned_qpos(robot, case)
            diff = np.argwhere(_bits(q) != _bits(clean))
            assert diff.tolist() == [[case.frame, NF.robot_tree(robot).cols[case.coord]]] and 0 <= case.frame < NF.N
    pos, quat, sc = NF.keypoints("unitree_g1")
    assert np.isfinite(pos).all() and np.isfinite(quat).all() and np.asarray(sc).dtype.kind == "i"
    for op in ("dof_to_rot", "rot_to_dof", "local_rot_to_global"):
        x, cases = NF.kin_setup("unitree_g1", op)
        assert np.isfinite(x).all()
        for case in cases:
            assert np.argwhere(_bits(NF.kin_poisoned("unitree_g1", op, case)) != _bits(x)).tolist() == [[case.frame, *case.where]]


@pytest.mark.parametrize("shape", [False, True])
def test_fk_sets_agree(shape):
    robot = "unitree_g1"
    sh = NF.fitted_shape(robot) if shape else None
    clean = NF.pred_fk(robot, NF.clean_qpos(robot), sh)
    assert all(np.isfinite(v).all() for v in clean.values())
    for case in NF.TABLE:
        _agree("fk", case, NF.dep_fk(robot, case), clean, NF.pred_fk(robot, NF.poisoned_qpos(robot, case), sh))
    # a hinge turns its own body and moves only what hangs on it
    t = NF.robot_tree(robot)
    j = t.dof_body[t.cols["leaf_hinge"] - 7]
    d = NF.dep_fk(robot, NF.Case("+nan", "leaf_hinge", 3))
    assert not d["pos"][3, j].any() and d["rot"][3, j].all() and d["pos"][3].any(axis=1).sum() == t.below[j].sum()


def test_min_height_sets_agree_and_follow_the_rule():
    robot = "unitree_g1"
    clean = NF.pred_min_height(robot, NF.clean_qpos(robot))
    empty = np.diff(NF.OFFS) == 0
    assert np.isfinite(clean["min_z"][~empty]).all() and (clean["min_z"][empty] == np.inf).all()
    for case in NF.TABLE:
        dep = NF.dep_min_height(robot, case)
        m = _agree("min_height", case, dep, clean, NF.pred_min_height(robot, NF.poisoned_qpos(robot, case)))["min_z"]
        s, low = NF.clip_of(case.frame), NF.pred_min_height(robot, NF.poisoned_qpos(robot, case))["min_z"]
        if case.value.endswith("nan"):
            assert np.isnan(low[s]) == bool(dep["min_z"][s])   # NaN when any height of the clip is NaN, for either sign
        elif case.coord == "root_z":   # inf_in_minimum, as listed: -inf wins, +inf loses unless the clip has no other frame
            one = NF.OFFS[s + 1] - NF.OFFS[s] == 1
            assert low[s] == (-np.inf if case.value == "-inf" else np.inf if one else clean["min_z"][s])
        assert not m[~dep["min_z"] & ~empty].any()
    # root x never reaches a height
    assert not NF.dep_min_height(robot, NF.Case("+nan", "root_x", 3))["min_z"].any()


@pytest.mark.parametrize("height,origin", NF.EPILOGUE_FLAGS)
@pytest.mark.parametrize("robot", ROBOTS2)
def test_epilogue_sets_agree(robot, height, origin):
    clean = NF.pred_epilogue(robot, NF.clean_qpos(robot), height, origin)
    for case in NF.TABLE:
        dep = NF.dep_epilogue(robot, case, height, origin)
        pred = NF.pred_epilogue(robot, NF.poisoned_qpos(robot, case), height, origin)
        m = _agree("epilogue", case, dep, clean, pred)
        s = NF.clip_of(case.frame)
        a, b = NF.OFFS[s], NF.OFFS[s + 1]
        if height and case.coord == "root_z":
            if case.value != "+inf" or b - a == 1:
                assert m["root_pos"][a:b, 2].all()   # a NaN or -inf height lowers the whole clip to a non-finite z
            else:
                assert m["root_pos"][a:b, 2].sum() == 1   # inf_in_minimum, as listed: +inf loses, the clip keeps its heights
        if origin and case.coord == "root_x" and case.frame == a:
            assert m["root_pos"][a:b, 0].all() and not m["root_pos"][:, 1:].any()


@pytest.mark.parametrize("rate", list(NF.TRACK_RATES))
@pytest.mark.parametrize("robot", ROBOTS2)
def test_tracking_sets_agree(robot, rate):
    clean = NF.pred_track(robot, NF.clean_qpos(robot), rate)
    assert all(np.isfinite(v).all() for v in clean.values())
    p = NF.plan(rate)
    for case in NF.track_table(rate):
        dep = NF.dep_track(robot, case, rate)
        m = _agree("track", case, dep, clean, NF.pred_track(robot, NF.poisoned_qpos(robot, case), rate))
        if NF.exception_for("track", case, "root_rot"):   # unit_of_inf, as listed: the poisoned component alone, in copies and blends
            rows = NF.track_reads(rate, case.frame)
            assert m["root_rot"][rows, 3].all() and not m["root_rot"][:, :3].any() and not m["root_rot"][~rows].any()
            assert m["body_quat_w"][rows, 0, 3].all() and not m["body_quat_w"][:, 0, :3].any() and m["body_quat_w"][rows, 1:].all()
        reads = NF.track_reads(rate, case.frame)
        assert reads.any() or p.ratio[0] > 1   # a frame the plan skips (ratio > 1) reaches nothing
        assert dep["root_pos"].any() == (reads.any() and case.coord in ("root_x", "root_z"))


def test_evaluate_rows_agree():
    robot = "unitree_g1"
    clean = NF.pred_evaluate(robot, NF.clean_qpos(robot))
    assert all(np.isfinite(v).all() for v in clean.values())
    for case in NF.TABLE:
        m = _agree("evaluate", case, NF.dep_evaluate(robot, case), clean, NF.pred_evaluate(robot, NF.poisoned_qpos(robot, case)))
        f = case.frame   # evaluate_rows, as listed: part of the frame's rows -- never none of them
        for k in m:   # rsqrt_of_inf, as listed: the root's xquat row, for an infinite root quaternion component, and nothing else
            lm = NF.listed_mask("evaluate", case, k, m[k])
            if k == "xquat" and case.coord == "root_qw" and case.value.endswith("inf"):
                assert m[k][f, 0].sum() == 1 and lm[f, 0].all() and np.array_equal(lm[f, 1:], m[k][f, 1:]) and m[k][f, 1:].all()
            else:
                assert lm is m[k]
        assert m["xpos"][f].any() or m["xquat"][f].any()
        assert m["err"][f].any() == m["task_err"][f].any()


@pytest.mark.parametrize("op", ["dof_to_rot", "rot_to_dof", "local_rot_to_global"])
def test_kin_op_sets_agree(op):
    robot = "unitree_g1"
    x, cases = NF.kin_setup(robot, op)
    clean = NF.pred_kin(robot, op, x)
    assert np.isfinite(clean["out"]).all()
    for case in cases:
        dep = NF.dep_kin(robot, op, case)
        m = _agree(op, case, dep, clean, NF.pred_kin(robot, op, NF.kin_poisoned(robot, op, case)))["out"]
        if op == "rot_to_dof":   # rot_to_dof_select, as listed: only a NaN w comes through
            if dep["out"].any():
                assert m[dep["out"]].all() == (case.value.endswith("nan") and case.where[1] == 3), case
            else:
                assert case.where[0] + 1 in NF.robot_tree(robot).fixed and not m.any()

"""gmr_motion_self_collision on the GPU against the numpy reference (tests/self_collision_reference.py; inputs:
tests/self_collision_inputs.py).

The bound.  self_collision_reference.bound: ten times the numpy reference's own distance to its 50-digit evaluator, measured per
robot on rows of these cases over all their pairs (FLOAT_WORST; tests/test_self_collision_host.py re-measures it), as an absolute
figure in metres with no other factor.  Nothing in the bound was measured on a kernel.

Measured on an MI355X (worst |GPU - numpy| per robot as a fraction of its bound): see DESIGN.md 4.15."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gmr_amd import collision  # noqa: E402
from tests import dynamics_inputs as di  # noqa: E402
from tests import dynamics_reference as R  # noqa: E402
from tests import self_collision_inputs as ci  # noqa: E402
from tests import self_collision_reference as SR  # noqa: E402
from tests.test_gpu_dynamics import DEV, _bytes, _dev, engine  # noqa: E402
from tests.util import compiled  # noqa: E402

FILL = 0xA5
F64, I32, I64, U8 = torch.float64, torch.int32, torch.int64, torch.uint8
FRAME = ("clearance", "pair", "hits")
STATS = ("clearance_min", "worst_frame", "worst_pair", "colliding_frames", "longest_run", "hits_sum", "nonfinite_frames")
COUNTS = ("colliding_frames", "longest_run", "hits_sum", "nonfinite_frames")
EINVAL, EUNSUPPORTED = -1, -3


def shapes(rows=ci.N, clips=ci.S):
    return {"clearance": ((rows,), F64), "pair": ((rows,), I32), "hits": ((rows,), I32), "clearance_min": ((clips,), F64),
            "worst_frame": ((clips,), I32), "worst_pair": ((clips,), I32), "colliding_frames": ((clips,), I32), "longest_run": ((clips,), I32),
            "hits_sum": ((clips,), I64), "nonfinite_frames": ((clips,), I32)}


def sentinel_out(names=None, **kw):
    out = {}
    for k, (sh, dt) in shapes(**kw).items():
        if names is None or k in names:
            out[k] = torch.empty(sh, dtype=dt, device=DEV())
            if out[k].numel():
                out[k].view(U8).fill_(FILL)
    return out


def run(robot, q, offs, caps=None, pairs=None, out=None, **kw):
    if caps is None:
        caps, pairs = ci.tables(robot)
    res = engine(robot).motion_self_collision(_dev(q), offs, caps, pairs, out=out, **kw)
    return {k: t.cpu().numpy() for k, t in res.items()}


@functools.lru_cache(maxsize=None)
def gpu(robot):
    """The GPU's answer to the robot's case into pre-filled caller-owned outputs: computed once, shared."""
    return run(robot, ci.qpos(robot), ci.OFFS, out=sentinel_out())


def check_frames(got, ref, bound, what):
    """The per-frame comparison of the issue: clearance within the bound, equal NaN patterns, the pair equal wherever the reference's
    best-to-second gap exceeds twice the bound (elsewhere the reference clearance of the GPU's pair is within the bound of the
    minimum), equal hits.  Returns the worst |GPU - numpy|."""
    cl = ref["pair_clearance"]
    assert np.array_equal(np.isnan(got["clearance"]), np.isnan(ref["clearance"])), what
    ok = ~np.isnan(ref["clearance"])
    err = np.abs(got["clearance"][ok] - ref["clearance"][ok])
    worst = float(err.max()) if err.size else 0.0
    assert worst <= bound, (what, worst, bound)
    assert np.array_equal(got["pair"][~ok], ref["pair"][~ok]) and np.array_equal(got["hits"], ref["hits"]), what
    gap = ci.second_gap(cl[ok]) if cl.shape[1] > 1 else np.full(int(ok.sum()), np.inf)
    clear = gap > 2.0 * bound
    gp, rp = got["pair"][ok], ref["pair"][ok]
    assert np.array_equal(gp[clear], rp[clear]), what
    assert (gp >= 0).all() and (gp < cl.shape[1]).all()
    near = np.abs(cl[ok][np.arange(gp.size), gp] - ref["clearance"][ok])
    assert near.max() <= bound, what
    return worst


# ------------------------------------------------------------------ 1: accuracy
@pytest.mark.parametrize("robot", ci.ROBOTS)
def test_frames_equal_the_reference(robot):
    got, ref = gpu(robot), ci.reference(robot)
    assert ci.margin_distance(robot) > 1000.0 * SR.bound(robot)       # the precondition of equal hit counts (a condition on the reference)
    worst = check_frames(got, ref, SR.bound(robot), robot)
    print(f"{robot}: worst |GPU - numpy| of the clearance {worst:.2e} ({worst / SR.bound(robot):.3f} of its bound {SR.bound(robot):.0e}), "
          f"{int((ref['hits'] > 0).sum())} colliding frames of {ci.N}")
    assert (ref["hits"] > 0).any() and not (ref["hits"] > 0).all()    # both kinds of frame are in the case
    assert got["pair"].dtype == got["hits"].dtype == np.int32


@pytest.mark.parametrize("robot", ci.ROBOTS)
def test_statistics_equal_the_reference(robot):
    check_statistics(robot)


def check_statistics(robot):
    """Every statistic is, bit for bit, the reference reduction of the GPU's own per-frame arrays.  Against the reference's statistics:
    counts equal, clearance_min within the bound, the worst frame and pair equal where the clip's minimum stands out by more than twice
    the bound."""
    got, ref = gpu(robot), ci.reference(robot)
    own = SR.statistics(got["clearance"], got["pair"], got["hits"], ci.OFFS)
    for k in STATS:
        assert got[k].dtype == own[k].dtype and np.array_equal(_bytes(got[k]), _bytes(own[k])), k
    for k in COUNTS:
        assert np.array_equal(got[k], ref[k]), k
    b = SR.bound(robot)
    assert got["clearance_min"][0] == np.inf and np.abs(got["clearance_min"][1:] - ref["clearance_min"][1:]).max() <= b
    for s, T in enumerate(ci.LENS):
        a = int(ci.OFFS[s])
        c = np.sort(ref["clearance"][a:a + T])
        if T and (T == 1 or c[1] - c[0] > 2.0 * b):
            assert got["worst_frame"][s] == ref["worst_frame"][s], s
    assert got["worst_frame"][0] == -1 and got["worst_pair"][0] == -1 and got["hits_sum"][0] == 0       # the empty clip
    assert np.array_equal(got["worst_pair"][1:], got["pair"][ci.OFFS[1:-1] + got["worst_frame"][1:]])


def test_galaxea_r1pro_runs_and_agrees_with_the_reference():
    """A planar base is accepted: internally it carries a free-joint qpos."""
    from gmr_amd.engine import Engine
    robot = "galaxea_r1pro"
    cm = compiled("smplx", robot)
    rob = R.model(robot)[0]
    assert cm.robot.planar_base and cm.robot.to_dict() == rob.to_dict()
    eng = Engine(cm, device=0)
    caps = collision.skeleton_capsules(rob, 0.03)
    pairs = collision.default_pairs(rob, caps)[0]
    q = np.concatenate([R.Trajectory(rob, s).state([k / 64.0 for k in range(T)])[0] for s, T in ((0, 5), (1, 70))])
    offs = np.array([0, 5, 75], np.int64)
    ref = SR.self_collision(rob, caps, pairs, q, offs)
    got = {k: t.cpu().numpy() for k, t in eng.motion_self_collision(_dev(q), offs, caps, pairs).items()}
    # (no 50-digit floor was measured for this robot: the largest of the three recorded ones, for a tree of the same size and reach)
    worst = check_frames(got, ref, max(SR.FLOAT_WORST.values()) * SR.GPU_FACTOR, robot)
    print(f"{robot}: {len(caps)} capsules, {len(pairs)} pairs, worst |GPU - numpy| {worst:.2e}")
    for k in COUNTS:
        assert np.array_equal(got[k], ref[k]), k


# ------------------------------------------------------------------ 2: the result belongs to the table, not to the schedule
def test_a_reversed_and_a_doubled_pair_table():
    """Reversed table: the same clearance bytes, and the pair maps back -- where several pairs tie, to the highest old index now,
    which is the lowest new one.  Doubled table (every pair twice, P apart): an exact tie in every frame, resolved to the lower index.
    (booster_k1: its best pair stands out in 323 of the 332 frames; on G1 two mirrored pairs at the hips, fixed to each other, are
    within 1e-16 m of one another in 290.)"""
    robot = "booster_k1"
    caps, pairs = ci.tables(robot)
    P = len(pairs)
    base, ref = gpu(robot), ci.reference(robot)
    rev = run(robot, ci.qpos(robot), ci.OFFS, caps, collision.PairTable(pairs.pairs[::-1].copy()))
    assert np.array_equal(_bytes(rev["clearance"]), _bytes(base["clearance"])) and np.array_equal(rev["hits"], base["hits"])
    back = P - 1 - rev["pair"]
    assert (back >= base["pair"]).all()
    clear = ci.second_gap(ref["pair_clearance"]) > 2.0 * SR.bound(robot)
    assert np.array_equal(back[clear], base["pair"][clear]) and clear.sum() > ci.N // 2
    cl = ref["pair_clearance"]
    rows = np.arange(ci.N)
    assert np.abs(cl[rows, back] - cl[rows, base["pair"]]).max() <= 2.0 * SR.bound(robot)
    twice = run(robot, ci.qpos(robot), ci.OFFS, caps, collision.PairTable(np.concatenate([pairs.pairs, pairs.pairs])))
    assert np.array_equal(_bytes(twice["clearance"]), _bytes(base["clearance"])) and np.array_equal(twice["pair"], base["pair"])
    assert np.array_equal(twice["hits"], 2 * base["hits"]) and np.array_equal(twice["hits_sum"], 2 * base["hits_sum"])
    for k in ("clearance_min", "worst_frame", "worst_pair", "colliding_frames", "longest_run"):
        assert np.array_equal(_bytes(twice[k]), _bytes(base[k])), k


def test_pair_counts_around_the_wavefront_width():
    """1, 63, 64 and 65 pairs (the full table is the accuracy test): against the reference, and the minimum over 64 (65) pairs is, byte
    for byte, the smaller of the minimum over the first 63 (64) and the clearance of the last pair computed alone -- in another lane
    and another pass."""
    robot = "booster_k1"
    caps, pairs = ci.tables(robot)
    q, cl = ci.qpos(robot), ci.reference(robot)["pair_clearance"]
    got = {}
    for n in (1, 63, 64, 65):
        got[n] = run(robot, q, ci.OFFS, caps, collision.PairTable(pairs.pairs[:n].copy()))
        ref = SR.frames(cl[:, :n])
        ref["pair_clearance"] = cl[:, :n]
        check_frames(got[n], ref, SR.bound(robot), n)
    for n in (64, 65):
        alone = run(robot, q, ci.OFFS, caps, collision.PairTable(pairs.pairs[n - 1:n].copy()), stats=False)
        assert sorted(alone) == sorted(FRAME) and not alone["pair"].any()
        assert np.array_equal(_bytes(np.minimum(got[n - 1]["clearance"], alone["clearance"])), _bytes(got[n]["clearance"])), n
        want = np.where(alone["clearance"] < got[n - 1]["clearance"], n - 1, got[n - 1]["pair"])
        assert np.array_equal(got[n]["pair"], want) and np.array_equal(got[n]["hits"], got[n - 1]["hits"] + alone["hits"]), n


def _raw_tables(eng, body, p0, p1, radius, pairs):
    host = {"cap_body": np.asarray(body, np.int32), "cap_p0": np.asarray(p0, np.float64), "cap_p1": np.asarray(p1, np.float64),
            "cap_radius": np.asarray(radius, np.float64), "pairs": np.asarray(pairs, np.int32).reshape(-1, 2)}
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV()) for k, v in host.items()}


def raw_call(eng, q, offs, tab, out, margin=0.0, **kw):
    """The entry itself, from device tensors: (return code, message)."""
    from gmr_amd import _native
    st = _native.SelfCollisionInput()
    st.qpos, st.n_frames, st.seq_offsets, st.n_seq = q.data_ptr(), int(q.shape[0]), offs.data_ptr(), int(offs.shape[0]) - 1
    st.n_caps, st.n_pairs, st.margin = int(tab["cap_body"].shape[0]), int(tab["pairs"].shape[0]), margin
    for k, t in tab.items():
        setattr(st, k, t.data_ptr())
    for k, t in out.items():
        setattr(st, k + "_out", t.data_ptr())
    for k, v in kw.items():
        setattr(st, k, v)
    st.stream = torch.cuda.current_stream(DEV()).cuda_stream
    rc = eng._lib.gmr_motion_self_collision(eng._h, C.byref(st))
    return rc, eng._lib.gmr_last_error(eng._h)


@pytest.mark.parametrize("n_caps", [1, 64, 65, 256])
def test_capsule_counts_with_synthetic_tables(n_caps):
    """1, 64, 65 and 256 capsules on random bodies, ends within 0.2 m of the body's origin (no farther than the skeleton's links
    reach, so the skeleton's bound holds), every pair of them: 1 (a capsule against itself), 2 016, 2 080 and 32 640 pairs -- the
    last is beyond what is staged in LDS and takes the instance that re-reads the pair table."""
    robot = "unitree_g1"
    rob, eng = ci.robot_model(robot), engine(robot)
    rng = np.random.default_rng(n_caps)
    body = rng.integers(0, rob.nbody, n_caps)
    p0, p1 = rng.uniform(-0.2, 0.2, (n_caps, 3)), rng.uniform(-0.2, 0.2, (n_caps, 3))
    p1[::5] = p0[::5]                                                    # every fifth a sphere
    radius = rng.uniform(0.005, 0.03, n_caps)
    prs = np.array([(a, b) for a in range(n_caps) for b in range(a + 1, n_caps)] or [(0, 0)], np.int32)
    rows = slice(int(ci.OFFS[6]), int(ci.OFFS[6]) + 40)                  # 40 rows of the 64-frame clip, as clips of 0, 3 and 37
    q, offs = np.array(ci.qpos(robot)[rows]), np.array([0, 0, 3, 40], np.int64)
    out = sentinel_out(rows=40, clips=3)
    rc, msg = raw_call(eng, _dev(q), _dev(offs), _raw_tables(eng, body, p0, p1, radius, prs), out)
    assert rc == 0, msg
    got = {k: t.cpu().numpy() for k, t in out.items()}
    caps = collision.CapsuleTable(body, p0, p1, radius, [str(i) for i in range(n_caps)])
    pt = collision.PairTable.__new__(collision.PairTable)
    pt.pairs = prs                                                       # ((0, 0) is not a pair a PairTable admits)
    ref = SR.self_collision(rob, caps, pt, q, offs)
    if n_caps == 1:
        assert np.array_equal(got["clearance"], np.full(40, -2.0 * radius[0])) and not got["pair"].any() and (got["hits"] == 1).all()
    check_frames(got, ref, SR.bound(robot), n_caps)
    own = SR.statistics(got["clearance"], got["pair"], got["hits"], offs)
    for k in STATS:
        assert np.array_equal(_bytes(got[k]), _bytes(own[k])), k


def test_wavefronts_per_clip_and_where_the_pairs_live_change_no_byte(monkeypatch):
    """One wavefront per clip, seven, and the host's own choice; the pair table staged in LDS and re-read from memory; a 130-frame
    clip alone and inside the batch."""
    robot = "booster_k1"            # (two frames side by side in a wavefront: the odd clips leave an idle half)
    base = gpu(robot)
    for env in ({"GMR_AMD_COLLISION_WAVES": "1"}, {"GMR_AMD_COLLISION_WAVES": "7"}, {"GMR_AMD_COLLISION_PAIRS": "global"},
                {"GMR_AMD_COLLISION_PAIRS": "global", "GMR_AMD_COLLISION_WAVES": "3"}):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            got = run(robot, ci.qpos(robot), ci.OFFS, out=sentinel_out())
        for k in got:
            assert np.array_equal(_bytes(got[k]), _bytes(base[k])), (env, k)
    a = int(ci.OFFS[8])
    alone = run(robot, ci.qpos(robot)[a:a + 130], [0, 130])
    for k in FRAME:
        assert np.array_equal(_bytes(alone[k]), _bytes(base[k][a:a + 130])), k
    for k in STATS:
        assert np.array_equal(_bytes(alone[k][0]), _bytes(base[k][8])), k


@pytest.mark.parametrize("robot", ["unitree_g1", "booster_k1"])
def test_two_calls_give_identical_bytes(robot):
    a, b = run(robot, ci.qpos(robot), ci.OFFS, out=sentinel_out()), gpu(robot)
    c = run(robot, ci.qpos(robot), ci.OFFS)                          # without out the call allocates the same answer
    d = c
    if robot == "unitree_g1":                                        # the default proxies are the case's table: the skeleton at 0.03 m
        d = {k: t.cpu().numpy() for k, t in engine(robot).motion_self_collision(_dev(ci.qpos(robot)), ci.OFFS).items()}
    for k in a:
        assert np.array_equal(_bytes(a[k]), _bytes(b[k])) and np.array_equal(_bytes(a[k]), _bytes(c[k])) and np.array_equal(_bytes(a[k]), _bytes(d[k])), k
    eng = engine(robot)
    assert eng.collision_device(*ci.tables(robot)) is eng.collision_device(*ci.tables(robot))          # uploaded once per (capsules, pairs)


# ------------------------------------------------------------------ 3: known answers
def test_the_standing_pose_is_free_and_the_hand_built_clip_hits_the_head():
    robot = "unitree_g1"
    caps, pairs = ci.tables(robot)
    stand = run(robot, di.standing(robot, 5), [0, 5])
    assert stand["colliding_frames"].tolist() == [0] and stand["clearance_min"][0] > 0.0 and stand["longest_run"].tolist() == [0]
    assert not stand["hits"].any() and stand["worst_frame"].tolist() == [0]                            # five equal frames: the earliest
    q = ci.reach_pose()
    ref = SR.self_collision(ci.robot_model(robot), caps, pairs, q, [0, q.shape[0]])
    got = run(robot, q, [0, q.shape[0]])
    a, b = collision.pair_names(caps, pairs)[int(got["worst_pair"][0])]
    assert "head" in a and (b.startswith("right_wrist") or b.startswith("right_rubber_hand")), (a, b)
    assert got["worst_frame"].tolist() == ref["worst_frame"].tolist() == [5] and got["worst_pair"].tolist() == ref["worst_pair"].tolist()
    assert got["colliding_frames"].tolist() == [1] and got["hits"].tolist() == ref["hits"].tolist() and got["clearance_min"][0] < -0.01
    assert abs(got["clearance_min"][0] - ref["clearance_min"][0]) <= SR.bound(robot)


def test_moving_and_turning_the_root_changes_the_clearance_by_no_more_than_the_bound():
    """The clearance is a property of the hinges: the same rows under other roots (within 1.5 m of the origin, any orientation, a
    quaternion that is not unit -- it is divided by its norm) give it again to within the bound, and the same hit counts."""
    robot = "unitree_g1"
    q = np.array(ci.qpos(robot))
    base = gpu(robot)
    rng = np.random.default_rng(11)
    moved = q.copy()
    moved[:, 0:3] = rng.uniform(-1.5, 1.5, (ci.N, 3))
    quat = rng.normal(size=(ci.N, 4))
    moved[:, 3:7] = quat / np.linalg.norm(quat, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (ci.N, 1))   # (not unit: divided by its norm)
    got = run(robot, moved, ci.OFFS)
    d = np.abs(got["clearance"] - base["clearance"]).max()
    print(f"{robot}: another root changes the clearance by at most {d:.2e} (bound {SR.bound(robot):.0e})")
    assert d <= SR.bound(robot) and np.array_equal(got["hits"], base["hits"])
    assert np.abs(got["clearance"] - ci.reference(robot)["clearance"]).max() <= SR.bound(robot)


# ------------------------------------------------------------------ 4: non-finite rows
def test_a_non_finite_row_reaches_its_own_frame_and_its_own_clip_only():
    robot = "unitree_g1"
    a = int(ci.OFFS[8])
    q0 = np.array(ci.qpos(robot)[a:a + 18])
    offs = np.array([0, 6, 12, 18], np.int64)
    clean = run(robot, q0, offs)
    rob = ci.robot_model(robot)
    caps, pairs = ci.tables(robot)
    for col, val in ((0, np.nan), (1, np.inf), (4, np.nan), (5, -np.inf), (7 + 3, np.nan), (rob.nq - 1, np.inf), ("zero quaternion", 0.0)):
        q1 = q0.copy()
        if col == "zero quaternion":
            q1[8, 3:7] = 0.0
        else:
            q1[8, col] = val
        got = run(robot, q1, offs)
        ref = SR.self_collision(rob, caps, pairs, q1, offs)
        assert np.isnan(got["clearance"][8]) and got["pair"][8] == -1 and got["hits"][8] == 0, col
        keep = np.arange(18) != 8
        for k in FRAME:
            assert np.array_equal(_bytes(got[k][keep]), _bytes(clean[k][keep])), (col, k)       # no other frame changes
            assert np.array_equal(np.isnan(got["clearance"]), np.isnan(ref["clearance"])), col
        for k in STATS:
            assert np.array_equal(_bytes(got[k][[0, 2]]), _bytes(clean[k][[0, 2]])), (col, k)     # no byte of another clip changes
        own = SR.statistics(got["clearance"], got["pair"], got["hits"], offs)
        for k in STATS:
            assert np.array_equal(_bytes(got[k]), _bytes(own[k])), (col, k)
        assert got["nonfinite_frames"].tolist() == [0, 1, 0] and np.array_equal(got["colliding_frames"], ref["colliding_frames"])


# ------------------------------------------------------------------ 5: outputs left out, sentinels
def test_outputs_left_out_are_not_computed_and_rows_outside_every_clip_are_not_written():
    robot = "booster_k1"
    q, full = ci.qpos(robot), gpu(robot)
    for k, t in full.items():
        assert not bool((_bytes(t) == FILL).all()) or t.size == 0, k           # every element of a non-NULL output was written
    frames_only = run(robot, q, ci.OFFS, out=sentinel_out(names=FRAME))
    assert sorted(frames_only) == sorted(FRAME)
    for k in FRAME:
        assert np.array_equal(_bytes(frames_only[k]), _bytes(full[k])), k
    for k in FRAME:                                                              # a single per-frame output
        one = run(robot, q, ci.OFFS, out=sentinel_out(names=(k,)))
        assert list(one) == [k] and np.array_equal(_bytes(one[k]), _bytes(full[k])), k
    for k in STATS:                                                              # every statistic alone with the three per-frame arrays
        some = run(robot, q, ci.OFFS, out=sentinel_out(names=FRAME + (k,)))
        assert sorted(some) == sorted(FRAME + (k,)) and np.array_equal(_bytes(some[k]), _bytes(full[k])), k
    offs = ci.OFFS.copy()
    offs[-1] -= 7                                                                # the last clip ends seven rows early
    got = run(robot, q, offs, out=sentinel_out())
    for k in FRAME:
        assert bool((_bytes(got[k][-7:]) == FILL).all()) and np.array_equal(_bytes(got[k][:-7]), _bytes(full[k][:-7])), k
    own = SR.statistics(got["clearance"][:-7], got["pair"][:-7], got["hits"][:-7], offs)
    for k in STATS:
        assert np.array_equal(_bytes(got[k]), _bytes(own[k])), k
    with pytest.raises(Exception, match="clearance, pair and hits"):
        run(robot, q, ci.OFFS, out=sentinel_out(names=("clearance", "hits", "longest_run")))
    wide = run(robot, q, ci.OFFS, margin=0.02)                                   # a margin counts near misses as hits
    assert np.array_equal(_bytes(wide["clearance"]), _bytes(full["clearance"])) and (wide["hits"] >= full["hits"]).all()
    assert np.array_equal(wide["hits"], SR.frames(ci.reference(robot)["pair_clearance"], 0.02)["hits"]) and wide["hits"].sum() > full["hits"].sum()


# ------------------------------------------------------------------ 6: errors and empty calls
def test_bad_arguments_are_refused_with_their_code_and_empty_calls_return_ok():
    robot = "booster_k1"
    eng = engine(robot)
    caps, pairs = ci.tables(robot)
    tab = eng.collision_device(caps, pairs)
    q, offs = _dev(ci.qpos(robot)), _dev(ci.OFFS)
    out = sentinel_out()
    nan, inf = float("nan"), float("inf")
    for kw, code, word in (({"margin": nan}, EINVAL, b"margin"), ({"margin": inf}, EINVAL, b"margin"), ({"n_caps": 0}, EINVAL, b"at least 1"),
                           ({"n_pairs": 0}, EINVAL, b"at least 1"), ({"n_frames": -1}, EINVAL, b"negative"), ({"n_seq": -1}, EINVAL, b"negative"),
                           ({"n_caps": -1}, EINVAL, b"negative"), ({"n_pairs": -2}, EINVAL, b"negative"), ({"qpos": None}, EINVAL, b"null"),
                           ({"seq_offsets": None}, EINVAL, b"null"), ({"cap_body": None}, EINVAL, b"null"), ({"cap_p0": None}, EINVAL, b"null"),
                           ({"cap_p1": None}, EINVAL, b"null"), ({"cap_radius": None}, EINVAL, b"null"), ({"pairs": None}, EINVAL, b"null"),
                           ({"clearance_out": None}, EINVAL, b"all three"), ({"pair_out": None}, EINVAL, b"all three"),
                           ({"hits_out": None}, EINVAL, b"all three"), ({"n_caps": 257}, EUNSUPPORTED, b"capsules"),
                           ({"n_pairs": 32769}, EUNSUPPORTED, b"pairs")):
        rc, msg = raw_call(eng, q, offs, tab, out, **kw)
        assert rc == code and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    for k, t in out.items():
        assert bool((t.view(U8) == FILL).all()), k       # nothing was launched
    # the empty calls: no frames, no clips -- GMR_OK without a launch, whatever else the struct holds
    for kw in ({"n_frames": 0}, {"n_seq": 0}, {"n_frames": 0, "qpos": None, "pairs": None, "n_caps": 0}, {"n_seq": 0, "seq_offsets": None, "n_pairs": 0}):
        rc, msg = raw_call(eng, q, offs, tab, out, **kw)
        assert rc == 0, (kw, msg)
    torch.cuda.synchronize()
    for k, t in out.items():
        assert bool((t.view(U8) == FILL).all()), k
    empty = eng.motion_self_collision(torch.zeros((0, eng.nq), dtype=F64, device=DEV()), [0, 0, 0], caps, pairs)
    assert empty["clearance"].numel() == 0 and empty["clearance_min"].tolist() == [inf, inf] and empty["worst_frame"].tolist() == [-1, -1]
    assert empty["worst_pair"].tolist() == [-1, -1] and not empty["hits_sum"].any() and not empty["colliding_frames"].any()
    assert raw_call(eng, q, offs, tab, out)[0] == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bytes(out["clearance"].cpu().numpy()), _bytes(gpu(robot)["clearance"]))
    # (no model of the registry has more than 64 bodies or a body in front of its parent: those two refusals are not exercised)
    from gmr_amd.engine import EngineError
    with pytest.raises(ValueError, match="capsules"):
        eng.motion_self_collision(q, offs, collision.CapsuleTable(np.zeros(257, np.int32), np.zeros((257, 3)), np.zeros((257, 3)), np.full(257, 0.01),
                                                                  [""] * 257), pairs)
    with pytest.raises(EngineError, match="qpos"):
        eng.motion_self_collision(q.float(), offs, caps, pairs)


# ------------------------------------------------------------------ 7: the Python layers
def test_dataset_functions_and_the_class_method_return_the_engines_answer(tmp_path):
    from gmr_amd import GeneralMotionRetargeting, MultiRobotRetargeting, dataset
    robot = "unitree_g1"
    g = GeneralMotionRetargeting("smplx", robot, verbose=False)
    q, want = _dev(ci.qpos(robot)), gpu(robot)
    caps, pairs = ci.tables(robot)
    clips = dataset.self_collision_from_qpos(g, q, ci.OFFS)                    # the defaults: the skeleton at 0.03 m, the case's table
    assert len(clips) == ci.S and [c["clearance"].shape[0] for c in clips] == ci.LENS
    for s, c in enumerate(clips):
        a, b = int(ci.OFFS[s]), int(ci.OFFS[s + 1])
        for k in FRAME:
            assert np.array_equal(_bytes(c[k]), _bytes(want[k][a:b])), k
        for k in STATS:
            assert np.array_equal(_bytes(c[k]), _bytes(want[k][s])), k
        assert c["pair_names"] == collision.pair_names(caps, pairs)
    rep = dataset.self_collision_report(g, q, ci.OFFS)
    assert sorted(rep) == sorted(STATS + ("worst_pair_names", "penetration_max"))
    for k in STATS:
        assert np.array_equal(_bytes(rep[k]), _bytes(want[k])), k
    assert np.array_equal(rep["penetration_max"], np.maximum(0.0, -want["clearance_min"])) and rep["penetration_max"][0] == 0.0
    names = collision.pair_names(caps, pairs)
    assert rep["worst_pair_names"] == [names[p] if p >= 0 else ("", "") for p in want["worst_pair"]]
    again = g.self_collision_report(np.array(ci.qpos(robot)), ci.OFFS)          # the class method takes numpy too
    assert np.array_equal(_bytes(again["clearance_min"]), _bytes(want["clearance_min"]))
    thin = g.self_collision_report(q, ci.OFFS, radius=0.01)
    assert thin["colliding_frames"].sum() < rep["colliding_frames"].sum()
    collision.save_proxies(str(tmp_path / "g1.json"), caps, pairs)
    c2, p2 = collision.load_proxies(str(tmp_path / "g1.json"))
    filed = g.self_collision_report(q, ci.OFFS, capsules=c2, pairs=p2)
    for k in STATS:
        assert np.array_equal(_bytes(filed[k]), _bytes(want[k])), k
    dataset.write_collision_csv(str(tmp_path / "col.csv"), [f"clip{s}" for s in range(ci.S)], rep)
    assert len((tmp_path / "col.csv").read_text().splitlines()) == ci.S + 1
    assert dataset.collision_hard_mask(rep, 0.03).tolist() == (rep["penetration_max"] > 0.03).tolist() and dataset.collision_hard_mask(rep, 0.03).any()
    robots = ["unitree_g1", "booster_k1"]
    mr = MultiRobotRetargeting("smplx", robots)
    reps = mr.self_collision_report({r: _dev(ci.qpos(r)) for r in robots}, ci.OFFS, radius=0.03)
    assert sorted(reps) == sorted(robots)
    for k in STATS:
        assert np.array_equal(_bytes(reps["unitree_g1"][k]), _bytes(want[k])), k
    k1 = engine("booster_k1").motion_self_collision(_dev(ci.qpos("booster_k1")), ci.OFFS, *engine("booster_k1").default_proxies(0.03))
    assert np.array_equal(reps["booster_k1"]["clearance_min"], k1["clearance_min"].cpu().numpy())

"""The three kernels that sweep a pose with LANE = BODY -- motion_dynamics_kernel, motion_self_collision_kernel and
motion_transitions_points_kernel -- on synthetic trees of every wavefront packing (tests/synthetic_trees.py): 64, 32, 16, 8, 4 and 2
frames side by side and one frame per pass, trees that fill their group to the last lane and trees one body past a power of two,
sweeps of one level (a star) and of 63 (the chain of 64 bodies).  The registry robots reach two packings (23 bodies: two frames side
by side; 38 and 52: one frame).

The inputs are the existing ones by name (dynamics_inputs, self_collision_inputs, transitions_inputs): clips of 0, 1, 2, 3, 4, 63, 64,
65 and 130 frames at 64 Hz.  With 8 frames side by side the 63-frame clip ends in a pass of 7 live groups, the 3-frame clip is a
pass of 3, and the 130-frame clip makes every wavefront take several passes.

The bounds.  As for the registry robots: GPU_FACTOR (10) times the numpy reference's own distance to its 50-digit evaluator,
measured per tree on the frames compared (FLOAT_WORST of dynamics_reference and self_collision_reference; re-measured by
tests/test_synthetic_trees_host.py); the transition search's costs within transitions_reference.bound.  Nothing in a bound was
measured on a kernel.  The last tests have no tolerance at all: the same mechanics in another packing must give the same bytes.

Stars never collide and trees of fewer than 9 bodies have few pairs: their self-collision case need not hold colliding and free
frames (synthetic_trees.collides).  Twelve trees -- the chains of up to 4 bodies, every star, the combs of up to 17 -- are never
unloaded, so their dynamics cases need not hold frames without a ZMP; the ten of synthetic_trees.UNLOADED must hold both kinds and
a positive unloaded_frames count.  The NaN patterns are compared for every tree.  The trees carry no torque limit: the limit
counters are 0 on all of them and their comparison covers nothing here.

Measured on an MI355X (worst |GPU - numpy| per tree family as a share of its bound): see DESIGN.md 4.14, 4.15 and 4.18."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import dynamics_inputs as di  # noqa: E402
from tests import dynamics_reference as R  # noqa: E402
from tests import self_collision_inputs as ci  # noqa: E402
from tests import self_collision_reference as SR  # noqa: E402
from tests import synthetic_trees as T  # noqa: E402
from tests import test_gpu_dynamics as GD  # noqa: E402
from tests import test_gpu_self_collision as GC  # noqa: E402
from tests import test_gpu_transitions as GT  # noqa: E402
from tests import transitions_inputs as ti  # noqa: E402
from tests import transitions_reference as TR  # noqa: E402
from tests.test_gpu_dynamics import _bytes  # noqa: E402

L = 4
COLLISION_TREES = [t for t in T.TREES if T.parse(t)[1] >= 3]        # at least one capsule pair
TRANSITION_TREES = [t for t in T.TREES if T.parse(t)[1] >= 2]
PACKINGS = [(base, k) for base in T.PACKING_BASES for k in (1, T.parse(base)[1])]     # one body more; as many again: the next jp, full


def test_the_engines_tree_is_the_packing_the_name_promises():
    for tree in T.TREES:
        eng, n = GD.engine(tree), T.parse(tree)[1]
        assert eng.nbody == n == R.model(tree)[0].nbody and eng.nq == R.model(tree)[0].nq
    assert sorted({T.geom(GD.engine(t).nbody)[1] for t in T.TREES}) == [1, 2, 4, 8, 16, 32, 64]


# ------------------------------------------------------------------ inverse dynamics
@pytest.mark.parametrize("case", ["explicit", "diff"])
@pytest.mark.parametrize("tree", T.TREES)
def test_dynamics_frames_equal_the_reference(tree, case):
    """tau, root_wrench, com and zmp within the tree's bound, NaN patterns equal.  tree/chain/1, a floating base alone, is answered
    (the contract above gmr_dynamics_input): tau has no column, the rest is one rigid body's."""
    got, ref = GD.check_frames(tree, case)
    rob = R.model(tree)[0]
    assert got["tau"].shape == (di.N, rob.nq - 7) and got["root_wrench"].shape == (di.N, 6)
    unloaded = np.isnan(ref["zmp"]).any(axis=1)
    assert (unloaded.any() and not unloaded.all()) == (tree in T.UNLOADED)    # both kinds of frame, wherever the tree has them
    for k in GD.FRAME:                                              # every row of every clip was written over the sentinel
        if got[k].shape[1]:
            assert not (_bytes(got[k]).reshape(di.N, -1) == GD.FILL).all(axis=1).any(), k


@pytest.mark.parametrize("tree", T.TREES)
def test_dynamics_velocities_pass_through_and_differences_are_exact(tree):
    GD.check_pass_through(tree)
    GD.check_differences(tree)


@pytest.mark.parametrize("case", ["explicit", "diff"])
@pytest.mark.parametrize("tree", T.TREES)
def test_dynamics_statistics_equal_the_reference(tree, case):
    got, ref = GD.check_statistics(tree, case)
    assert (ref["unloaded_frames"].sum() > 0) == (tree in T.UNLOADED) and np.array_equal(got["unloaded_frames"], ref["unloaded_frames"])


@pytest.mark.parametrize("tree", T.TREES)
def test_dynamics_rows_outside_every_clip_stay_untouched(tree):
    q, v, a = di.explicit(tree)
    full = GD.gpu(tree, "explicit")
    offs = di.OFFS.copy()
    offs[-1] -= 7                                                   # the last clip ends seven rows early: with 8 groups, inside a pass
    got = GD.run(tree, q, offs, v, a, out=GD.sentinel_out(tree))
    for k in ("tau", "root_wrench", "com", "zmp", "qvel", "qacc"):
        assert bool((_bytes(got[k][-7:]) == GD.FILL).all()) and np.array_equal(_bytes(got[k][:-7]), _bytes(full[k][:-7])), k


# ------------------------------------------------------------------ self-collision
@pytest.mark.parametrize("tree", COLLISION_TREES)
def test_self_collision_frames_equal_the_reference(tree):
    got, ref = GC.gpu(tree), ci.reference(tree)
    b = SR.bound(tree)
    assert ci.margin_distance(tree) > 1000.0 * b                    # the precondition of equal hit counts (a condition on the reference)
    worst = GC.check_frames(got, ref, b, tree)
    caps, pairs = ci.tables(tree)
    print(f"{tree}: {len(caps)} capsules, {len(pairs)} pairs: worst |GPU - numpy| of the clearance {worst:.2e} ({worst / b:.3f} of its bound {b:.0e}), "
          f"{int((ref['hits'] > 0).sum())} colliding frames of {ci.N}")
    if T.collides(tree):
        assert (ref["hits"] > 0).any() and not (ref["hits"] > 0).all()
    assert got["pair"].dtype == got["hits"].dtype == np.int32
    for k in GC.FRAME:
        assert not (_bytes(got[k]).reshape(ci.N, -1) == GC.FILL).all(axis=1).any(), k


@pytest.mark.parametrize("tree", COLLISION_TREES)
def test_self_collision_statistics_equal_the_reference(tree):
    GC.check_statistics(tree)


# ------------------------------------------------------------------ the transition search
@pytest.mark.parametrize("tree", TRANSITION_TREES)
def test_transition_points_moments_and_search_equal_the_restatement(tree):
    """Every body a point, unit weights, a self-search with min_gap = L.  test_gpu_transitions.check: the points against the numpy FK
    within the tree's bound, and -- fed the kernel's own points -- the moments, costs and the reduction bit for bit.  Then against
    the search of the numpy FK's own points: best_cost within transitions_reference.bound, and the kernel's best frame is a
    minimiser of the reference's costs to within twice that bound."""
    q, offs = ti.library(tree, L)
    ids, w = ti.all_bodies(tree)
    got, mt = GT.check(tree, q, offs, ids, w, L, min_gap=L)
    assert len(ids) == T.parse(tree)[1]
    pts = TR.points(ti.model(tree), q, offs, ids)
    dense, best, frame = TR.search(pts, mt.weights, offs, L, mt.src_clips, mt.src_offsets, 1, mt.dst_clips, mt.dst_offsets, L)
    radius = float(np.sqrt((pts[..., :2] ** 2).sum(-1)).max())
    b = TR.bound(len(ids), L, radius)
    fin = np.isfinite(best)
    assert np.array_equal(fin, np.isfinite(got["best_cost"])) and np.array_equal(frame < 0, got["best_frame"] < 0) and fin.any()
    err = float(np.abs(got["best_cost"][fin] - best[fin]).max())
    u, d = np.nonzero(fin)
    at = dense[u, np.asarray(mt.dst_offsets)[d] + got["best_frame"][u, d]]
    print(f"{tree}: best_cost worst |GPU - numpy| {err:.2e} ({err / b:.2f} of its bound {b:.1e}, R {radius:.1f} m), "
          f"{int((got['best_frame'] != frame).sum())} of {frame.size} best frames differ")
    assert err <= b and np.all(at - best[fin] <= 2.0 * b)


# ------------------------------------------------------------------ packing must not change a bit
@pytest.mark.parametrize("base,k", PACKINGS)
def test_dynamics_bytes_do_not_depend_on_the_packing(base, k):
    """The base tree plus k bodies without a joint, mass or inertia as the last children of the base: another jp, another number of
    frames per wavefront, the same mechanics.  The extra bodies add exact zeros at the end of the root's sums only, so every output
    must keep its bytes -- unless a wrench component were a negative zero, which the reference shows none is."""
    wide = T.padded(base, k)
    assert T.geom(T.parse(base)[1])[1] > T.geom(T.parse(base)[1] + k)[1] and GD.engine(wide).nbody == T.parse(base)[1] + k
    tab = R.model(wide)[1]
    n = T.parse(base)[1]
    assert not tab.mass[n:].any() and not tab.inertia[n:].any() and np.array_equal(tab.mass[:n], R.model(base)[1].mass)
    q, v, a = di.explicit(base)
    for case, args in (("explicit", (q, di.OFFS, v, a)), ("diff", (di.quantised(base), di.OFFS))):
        ref = di.reference(base, case)["root_wrench"]
        assert not np.any((ref == 0.0) & np.signbit(ref))
        want = GD.gpu(base, case)
        got = GD.run(wide, *args, out=GD.sentinel_out(wide))
        assert sorted(got) == sorted(want)
        for name in want:
            assert np.array_equal(_bytes(got[name]), _bytes(want[name])), (case, name)


@pytest.mark.parametrize("base,k", PACKINGS)
def test_clearances_and_points_do_not_depend_on_the_packing(base, k):
    """The capsule, pair and point tables of the base tree, which name none of the extra bodies, on the wider model."""
    wide = T.padded(base, k)
    want = GC.gpu(base)
    got = GC.run(wide, ci.qpos(base), ci.OFFS, *ci.tables(base), out=GC.sentinel_out())
    for name in GC.FRAME + GC.STATS:
        assert np.array_equal(_bytes(got[name]), _bytes(want[name])), name
    q, offs = ti.library(base, L)
    ids, w = ti.all_bodies(base)
    a, _ = GT.run(base, q, offs, ids, w, L, min_gap=L)
    b, _ = GT.run(wide, q, offs, ids, w, L, min_gap=L)
    for name in GT.NAMES:
        assert np.array_equal(_bytes(a[name]), _bytes(b[name])), name

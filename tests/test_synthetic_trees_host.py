"""tests/synthetic_trees.py without a GPU: the trees cover every packing of chain_geom, their models plan in the stand-alone planner,
the recorded floors under the GPU bounds (FLOAT_WORST of dynamics_reference and self_collision_reference) are no smaller than what
is re-measured here, and the numpy reference meets the conditions under which tests/test_gpu_tree_packing.py may ask for equal
counts.  Everything here is a statement about the reference and the inputs; nothing was measured on a kernel."""
import numpy as np
import pytest

from tests import dynamics_inputs as di
from tests import dynamics_reference as R
from tests import model_plan_cases as mp
from tests import self_collision_inputs as ci
from tests import self_collision_reference as SR
from tests import synthetic_trees as T

PADDED = [T.padded(base, k) for base in T.PACKING_BASES for k in (1, T.parse(base)[1])]


# ------------------------------------------------------------------ 1: the trees
def test_geom_restates_chain_geom_and_the_trees_cover_every_packing():
    want = {1: (1, 64), 2: (2, 32), 3: (4, 16), 4: (4, 16), 5: (8, 8), 8: (8, 8), 9: (16, 4), 16: (16, 4), 17: (32, 2), 32: (32, 2),
            33: (64, 1), 63: (64, 1), 64: (64, 1)}
    assert {n: T.geom(n) for n in want} == want
    sizes = {shape: sorted(T.parse(t)[1] for t in T.TREES if T.parse(t)[0] == shape) for shape in T.SHAPES}
    assert sizes == {"chain": list(T.CHAIN_SIZES), "star": list(T.BRANCHED_SIZES), "comb": list(T.BRANCHED_SIZES)} and len(T.TREES) == 22
    assert sorted({T.geom(T.parse(t)[1])[1] for t in T.TREES}) == [1, 2, 4, 8, 16, 32, 64]
    chain = set(T.CHAIN_SIZES)
    for jp in (2, 4, 8, 16, 32):                                    # both sides of every jp edge: a full group and one body more
        assert jp in chain and (jp + 1 in chain or jp == 2 and 3 in chain)
    assert 64 in chain and 33 in chain and 1 in chain               # every lane a body; the first tree of the one-frame path; the base alone
    assert sorted({T.geom(T.parse(t)[1] + T.parse(t)[2])[1] for t in PADDED}) == [1, 2, 4, 8]
    assert set(T.UNLOADED) <= set(T.TREES) and len(T.UNLOADED) == 10
    assert {T.geom(T.parse(t)[1])[1] for t in T.UNLOADED} == {8, 4, 2, 1}     # (no tree of 4 bodies or fewer is ever unloaded)


@pytest.mark.parametrize("tree", T.TREES)
def test_the_model_is_the_tree_the_name_promises(tree):
    shape, n, _ = T.parse(tree)
    rob, tab = R.model(tree)
    par = [int(p) for p in rob.parent]
    depth = [0] * n
    for b in range(1, n):
        assert 0 <= par[b] < b
        depth[b] = depth[par[b]] + 1
    assert rob.nbody == tab.nbody == n and max(depth) == {"chain": n - 1, "star": min(1, n - 1), "comb": (n - 1 + 3) // 4}[shape]
    hinged = [b for b in range(n) if rob.jnt_type[b] == R.JNT_HINGE]
    assert hinged == [b for b in range(1, n) if b % 4] and rob.nq == 7 + len(hinged) and not tab.missing and (tab.mass > 0.0).all()
    assert all(np.linalg.eigvalsh(I).min() > 0.0 for I in tab.inertia)
    link = np.linalg.norm(rob.body_pos[1:], axis=1)
    assert np.all((link > 0.0599) & (link < 0.1201))
    with open(T.xml_path(tree)) as f:                               # the file is a function of the name alone
        assert f.read() == T.mjcf_text(T.tree_parents(tree), T.tree_seed(tree), n)
    assert T.compiled(tree).robot.to_dict() == rob.to_dict()


@pytest.mark.parametrize("wide", PADDED)
def test_a_padded_tree_is_its_base_tree_and_the_reference_keeps_its_bytes(wide):
    """The appended bodies hang on the base, come last, carry no joint, no mass and no inertia; the first bodies are the base tree's,
    digit for digit.  On the same rows the numpy reference gives the base tree's bytes -- what the GPU test asks of the kernels."""
    shape, n, k = T.parse(wide)
    base = f"tree/{shape}/{n}"
    (rob, tab), (rob0, tab0) = R.model(wide), R.model(base)
    assert rob.nbody == n + k and rob.nq == rob0.nq and [int(p) for p in rob.parent[n:]] == [0] * k and not np.any(rob.jnt_type[n:] == R.JNT_HINGE)
    for a, b in ((rob.body_pos[:n], rob0.body_pos), (rob.body_quat[:n], rob0.body_quat), (rob.jnt_axis[:n], rob0.jnt_axis), (tab.mass[:n], tab0.mass),
                 (tab.com[:n], tab0.com), (tab.inertia[:n], tab0.inertia), (rob.qpos_adr[:n], rob0.qpos_adr)):
        assert np.array_equal(a, b)
    assert not tab.mass[n:].any() and not tab.inertia[n:].any() and tab.total_mass == tab0.total_mass
    q, v, a = di.explicit(base)
    want, got = di.reference(base, "explicit"), R.dynamics(rob, tab, q, v, a)
    for key in got:
        assert np.array_equal(got[key].view(np.int64), want[key].view(np.int64)), key
    assert not np.any((want["root_wrench"] == 0.0) & np.signbit(want["root_wrench"]))     # no wrench component is a negative zero
    caps, pairs = ci.tables(base)
    assert np.array_equal(SR.pair_clearance(rob, caps, pairs, q), ci.reference(base)["pair_clearance"])


# ------------------------------------------------------------------ 2: the planner
def test_every_tree_plans_in_the_stand_alone_planner(tmp_path):
    cxx, rocm = mp.toolchain()
    if cxx is None or not rocm:
        pytest.skip("no C++ compiler or no ROCm headers")
    exe = mp.build_program(cxx, tmp_path / "model_plan_host", ["-O2"])
    names = T.TREES + PADDED
    res = mp.run_cases(exe, [(name, T.compiled(name).blob, 0, 0) for name in names], tmp_path, dump=False)
    assert {name: (res[name]["code"], res[name]["message"]) for name in names} == {name: (0, "") for name in names}


# ------------------------------------------------------------------ 3: the floors under the bounds
@pytest.mark.parametrize("tree", T.TREES)
def test_the_recorded_dynamics_floor_covers_the_trees_own_frames(tree):
    """The recorded figures are of all 332 rows of the tree's explicit case; re-measured here on every clip's first row and the
    extremes of every output (dynamics_inputs.floor_rows, as tests/test_dynamics_host.py takes them)."""
    rows = di.floor_rows(tree)
    worst = di.measure_floor(tree, rows)
    print(f"{tree}: {len(rows)} rows: worst |numpy - 50 digits|: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= R.FLOAT_WORST[tree][k], f"{k}: the recorded floor {R.FLOAT_WORST[tree][k]:.1e} is below the measured {v:.2e}"


@pytest.mark.parametrize("tree", [t for t in T.TREES if T.parse(t)[1] >= 2])
def test_the_recorded_clearance_floor_covers_the_trees_own_rows(tree):
    """The recorded figures are of all pairs of all 332 rows; re-measured here on self_collision_inputs.floor_rows.  tree/chain/2 has
    no capsule pair: its figure, the bound of the transition search's points, is that of the body origins."""
    if T.parse(tree)[1] == 2:
        rows = [int(ci.OFFS[s]) for s, n in enumerate(ci.LENS) if n] + [ci.N - 1]
        worst = ci.measure_origin_floor(tree, rows)
    else:
        rows = ci.floor_rows(tree)
        worst = ci.measure_floor(tree, rows)
    print(f"{tree}: {len(rows)} rows: worst |numpy - 50 digits| {worst:.2e} (recorded {SR.FLOAT_WORST[tree]:.0e})")
    assert worst <= SR.FLOAT_WORST[tree], f"the recorded floor {SR.FLOAT_WORST[tree]:.1e} is below the measured {worst:.2e}"
    assert SR.FLOAT_WORST[tree] <= 64 * np.finfo(float).eps * 16.0    # rounding of coordinates of up to 16 m, not a modelling difference


# ------------------------------------------------------------------ 4: the conditions on the inputs
@pytest.mark.parametrize("tree", T.TREES)
def test_the_reference_keeps_its_distance_from_every_counted_threshold(tree):
    """frames_over_limit and unloaded_frames (both cases), hits and colliding_frames are compared for equality: the reference's own
    values stay clear of their thresholds by the margins the existing GPU tests ask for.  Chains and combs of at least 9 bodies hold
    colliding and free frames at the tree's radius."""
    n = T.parse(tree)[1]
    for case in ("explicit", "diff"):
        ref = di.reference(tree, case)
        m_tau, m_fz = di.margins(tree, ref)
        assert m_tau > 1e-9 and m_fz > 1e-9, case
        # unloaded frames (no ZMP) beside loaded ones in exactly the trees of T.UNLOADED: the NaN-pattern and unloaded_frames
        # comparisons of the GPU test are not vacuous there, and the exempt set cannot grow unnoticed
        unloaded = np.isnan(ref["zmp"]).any(axis=1)
        assert (unloaded.any() and not unloaded.all()) == (tree in T.UNLOADED) == (ref["unloaded_frames"].sum() > 0), case
        assert not ref["frames_over_limit"].any() and not np.isfinite(R.model(tree)[1].torque_limit).any()   # (no limits: see synthetic_trees)
    if n >= 3:
        ref = ci.reference(tree)
        assert len(ci.tables(tree)[1]) >= 1 and ci.margin_distance(tree) > 1000.0 * SR.bound(tree)
        assert ci.case_radius(tree) in (0.01, 0.02, 0.03, 0.05)
        hit = ref["hits"] > 0
        assert not T.collides(tree) or (hit.any() and not hit.all())
    else:
        assert len(ci.tables(tree)[1]) == 0
    assert (T.parse(tree)[0] in ("chain", "comb") and n >= 9) == T.collides(tree)


def test_the_largest_star_takes_the_pair_table_from_memory():
    """More pairs than the self-collision kernel stages in LDS (kColPairsLdsMax, self_collision_kernel.hip.h)."""
    import os
    import re
    with open(os.path.join(R.ROOT, "gmr_amd", "csrc", "self_collision_kernel.hip.h")) as f:
        limit = int(re.search(r"kColPairsLdsMax\s*=\s*(\d+)", f.read()).group(1))
    assert len(ci.tables("tree/star/64")[1]) > limit >= len(ci.tables("tree/chain/64")[1])

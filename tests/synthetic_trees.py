"""Synthetic model trees of every wavefront packing, for the three kernels that sweep a pose with LANE = BODY (inverse dynamics,
self-collision, the transition search's points).  Host only, plain numpy; no torch and no native code here.

tree_chain.hip.h's chain_geom pads a tree of up to 32 bodies to jp, the next power of two, and puts 64 / jp frames side by side in a
wavefront; a tree of 33 to 64 bodies takes one frame per pass.  The registry robots only reach groups 1 and 2.  TREES holds

  chain   body k hangs on body k - 1: depth nbody - 1, the longest sweep a tree of that size can ask for
  star    every body hangs on the base: depth 1, every lane of every group reads its frame's root slot in the same round
  comb    four limbs (chains of equal length, the first ones one longer) off the base

at sizes on both sides of every jp edge, so that every groups value in {64, 32, 16, 8, 4, 2, 1} occurs (`geom`, asserted in
tests/test_synthetic_trees_host.py).  comb/5 is the tree of star/5 with other offsets and inertias.

A tree is named ``tree/<shape>/<nbody>``; ``tree/<shape>/<nbody>+<k>`` is the same tree with k more bodies appended as the last
children of the base (`padded`: another packing of the same mechanics).  tests/dynamics_reference.model resolves these names, so the
input modules (dynamics_inputs, self_collision_inputs, transitions_inputs) work for them as for a registry robot.

The MJCF of a tree is written by `mjcf_text`: a free joint on the base; every other body hinged about an axis cycling x, y, z with
range -1.2 .. 1.4, except every fourth, which has no joint (a fixed body inside a path); an <inertial> with a full inertia on every
body; body offsets of random direction and 0.06 .. 0.12 m length.  Every number comes from np.random.default_rng(seed of the tree)
and is written with six decimals, so the file is the same everywhere.  The file gives no torque limit (no actuator, no
actuatorfrcrange): frames_over_limit and frames_any_over_limit are 0 for every tree, so comparing them is no coverage of the limit
counters -- those are the registry robots' (tests/test_gpu_dynamics.py)."""
import functools
import os
import tempfile

import numpy as np

SHAPES = ("chain", "star", "comb")
CHAIN_SIZES = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)
BRANCHED_SIZES = (5, 9, 17, 33, 64)
TREES = [f"tree/chain/{n}" for n in CHAIN_SIZES] + [f"tree/{s}/{n}" for s in ("star", "comb") for n in BRANCHED_SIZES]
PACKING_BASES = [f"tree/chain/{n}" for n in (4, 8, 16, 32)]
AXES = ("1 0 0", "0 1 0", "0 0 1")

# The capsule radius of a tree's self-collision case, from {0.01, 0.02, 0.03, 0.05}: for chains and combs of at least 9 bodies the
# first of them at which the reference sees colliding and free frames (self_collision_inputs.reference asserts both kinds).  Stars
# never collide (their bodies do not move against each other) and the smaller trees have too few pairs: for those the requirement
# is dropped and the radius is 0.01.  Chosen on the CPU from the numpy reference alone: 0.01 m serves every tree (33 to 325
# colliding frames of 332) but comb/9, which is free in every frame at 0.01, collides in 2 at 0.02 and in 86 at 0.03.
RADIUS = {"tree/comb/9": 0.03}
# The clips follow the trajectory seeds of the registry robots' cases (clip s: dynamics_reference.Trajectory(rob, s)).  With them the
# reference of every tree keeps the distance from the thresholds of the counted statistics that equal counts need
# (dynamics_inputs.margins, self_collision_inputs.margin_distance; asserted in tests/test_synthetic_trees_host.py).  A tree that
# came too near would get another tree seed, not an exemption.
#
# The trees whose dynamics cases (explicit and differenced alike) hold unloaded frames, without a ZMP, beside loaded ones: 9 to
# 137 of 332 rows in the reference.  The other twelve -- the chains of up to 4 bodies, every star, the combs of up to 17 -- are light
# and compact enough never to fall below the threshold: for them, and for them only, the "both kinds of frame" assertion is
# dropped.  tests/test_synthetic_trees_host.py pins this set against the reference.
UNLOADED = [f"tree/chain/{n}" for n in (5, 8, 9, 16, 17, 32, 33, 64)] + ["tree/comb/33", "tree/comb/64"]


def is_tree(name):
    return name.startswith("tree/")


def parse(name):
    """(shape, nbody, extra) of ``tree/<shape>/<nbody>[+<extra>]``."""
    _, shape, size = name.split("/")
    n, _, k = size.partition("+")
    if shape not in SHAPES or int(n) < 1:
        raise KeyError(name)
    return shape, int(n), int(k or 0)


def padded(name, k):
    """The name of the tree with k more jointless bodies as the last children of the base."""
    shape, n, extra = parse(name)
    assert extra == 0
    return f"tree/{shape}/{n}+{k}"


def parents(shape, nbody):
    """The parent list of a shape, depth first (a parent precedes its child, a subtree is a run of indices)."""
    if shape == "chain":
        return [-1] + list(range(nbody - 1))
    if shape == "star":
        return [-1] + [0] * (nbody - 1)
    par, m = [-1], nbody - 1
    for limb in range(4):
        for i in range(m // 4 + (1 if limb < m % 4 else 0)):
            par.append(0 if i == 0 else len(par) - 1)
    return par


def tree_parents(name):
    shape, n, extra = parse(name)
    return parents(shape, n) + [0] * extra


def tree_seed(name):
    shape, n, _ = parse(name)
    return 1000 * (1 + SHAPES.index(shape)) + n


def radius(name):
    shape, n, _ = parse(name)
    return RADIUS.get(f"tree/{shape}/{n}", 0.01)


def collides(name):
    """Whether the tree's self-collision case must hold colliding and free frames: chains and combs of at least 9 bodies."""
    shape, n, _ = parse(name)
    return shape in ("chain", "comb") and n >= 9


def geom(nbody):
    """(jp, groups) of chain_geom (gmr_amd/csrc/tree_chain.hip.h), restated."""
    if nbody > 32:
        return 64 * ((nbody + 63) // 64), 1
    p = 1
    while p < nbody:
        p <<= 1
    return p, 64 // p


def mjcf_text(par, seed, n_hinged=None):
    """The MJCF of the tree with the parent list `par`.  Bodies from index `n_hinged` on (default: none) carry no joint whatever
    their index: the appended bodies of a padded tree.  The random numbers of body b are drawn in body order, so a padded tree's
    first bodies are the base tree's, digit for digit."""
    nb = len(par)
    n_hinged = nb if n_hinged is None else n_hinged
    rng = np.random.default_rng(seed)
    fmt = lambda xs: " ".join(f"{x:.6f}" for x in xs)   # noqa: E731
    open_tag = []
    for b in range(nb):
        d = rng.normal(size=3)
        off = d / np.linalg.norm(d) * rng.uniform(0.06, 0.12)
        mass, com = rng.uniform(0.2, 2.0), rng.uniform(-0.02, 0.02, 3)
        diag, offd = rng.uniform(1e-3, 5e-3, 3), rng.uniform(-2e-4, 2e-4, 3)      # (diagonally dominant: positive definite)
        inertial = f'<inertial pos="{fmt(com)}" mass="{mass:.6f}" fullinertia="{fmt(np.concatenate([diag, offd]))}"/>'
        if b == 0:
            open_tag.append(f'<body name="base" pos="0 0 1"><freejoint/>{inertial}')
        else:
            joint = f'<joint name="j{b}" axis="{AXES[b % 3]}" range="-1.2 1.4"/>' if b < n_hinged and b % 4 else ""
            open_tag.append(f'<body name="b{b}" pos="{fmt(off)}">{joint}{inertial}')
    children = [[] for _ in range(nb)]
    for b in range(1, nb):
        children[par[b]].append(b)
    out, stack = [], [(0, False)]
    while stack:                                         # (no recursion: a chain of 64 is 64 levels deep)
        b, closing = stack.pop()
        if closing:
            out.append("</body>")
            continue
        out.append(open_tag[b])
        stack.append((b, True))
        stack.extend((c, False) for c in reversed(children[b]))
    return '<mujoco model="tree"><compiler angle="radian"/><worldbody>' + "".join(out) + "</worldbody></mujoco>\n"


@functools.lru_cache(maxsize=None)
def _directory():
    """The temp directory of this process's MJCF files, made once and removed with the process."""
    d = tempfile.TemporaryDirectory(prefix="gmr_trees_")
    _directory.keep = d
    return d.name


@functools.lru_cache(maxsize=None)
def xml_path(name):
    shape, n, extra = parse(name)
    path = os.path.join(_directory(), name.replace("/", "_").replace("+", "p") + ".xml")
    with open(path, "w") as f:
        f.write(mjcf_text(tree_parents(name), tree_seed(name), n))
    return path


@functools.lru_cache(maxsize=None)
def model(name):
    """(RobotModel, InertialTable) of a tree.  The appended bodies of a padded tree have zero mass and zero inertia."""
    import dataclasses
    from gmr_amd.inertial import load_inertial
    from gmr_amd.mjcf import load_mjcf
    shape, n, extra = parse(name)
    rob, tab = load_mjcf(xml_path(name), name=name), load_inertial(xml_path(name))
    assert rob.nbody == n + extra and [int(p) for p in rob.parent] == tree_parents(name)
    if extra:
        mass, com, inertia = tab.mass.copy(), tab.com.copy(), tab.inertia.copy()
        mass[n:], com[n:], inertia[n:] = 0.0, 0.0, 0.0
        tab = dataclasses.replace(tab, mass=mass, com=com, inertia=inertia)
    return rob, tab


@functools.lru_cache(maxsize=None)
def compiled(name):
    """The compiled model of a tree (the pattern of tests/footlock_inputs.synthetic_limb): IK tasks on `base` and `b1`, on `base`
    alone for a tree of one body."""
    from gmr_amd.ik_config import IKConfig, IKTask
    from gmr_amd.model import compile_model
    rob = model(name)[0]
    frames = [("base", "h_base")] + ([("b1", "h_tip")] if rob.nbody > 1 else [])
    tasks = [IKTask(f, h, 50.0, 10.0, [0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]) for f, h in frames]
    cfg = IKConfig("base", "h_base", 0.0, 1.8, True, True, {h: 1.0 for _, h in frames}, tasks, list(tasks), source="synthetic")
    return compile_model(rob, cfg)

"""The inputs of the torque-retiming tests (tests/retime_torque_reference.py restates the contracts).

Two layouts: RAGGED is tests/nonfinite_cases.py's [0, 37, 37, 38, 101, 310] -- an empty clip, a one-row clip, clip boundaries inside a
64-row tile -- and LENS is tests/dynamics_inputs.py's clips of 0, 1, 2, 3, 4, 63, 64, 65 and 130 rows: the short clips and the edges
of the kernels' tiles, of the need kernel's batches and of the alignment's 64 intervals.  Seven models give nh = 0, 1, 24, 29, 32,
43 and 48 hinge columns (every fourth body of a synthetic tree carries no joint: tree/chain/33 has 24 hinges, tree/chain/43 has 32
and tree/chain/64 has 48).  ``wide_model`` is a chain of 64 bodies with a hinge on every one but the base: nq 70, for the refusal of a
row that does not fit one wavefront.  tau and tau_static are random: the entry does not ask where they come
from.  The limits are drawn so that every branch of the contract is taken in every case: torques under and over the limit on either
side, gravity alone beyond the scaled limit with the dynamic part helping and hurting, and hinges without a limit."""
import functools
from typing import NamedTuple, Optional

import numpy as np

from tests import dynamics_inputs as di
from tests import nonfinite_cases as nc
from tests import retime_torque_reference as TR

RAGGED = nc.OFFS
LENS, OFFS = di.LENS, di.OFFS
LAYOUTS = {"ragged": RAGGED, "lens": OFFS}
MODELS = {"tree/chain/1": 0, "tree/chain/2": 1, "unitree_g1": 29, "tree/chain/33": 24, "unitree_g1_with_hands": 43, "tree/chain/64": 48,
          "tree/chain/43": 32}   # name -> nh
WIDE_BODIES, WIDE_NQ = 64, 70
FILL = 0xA5
WINDOW, MAX_STRETCH, SCALE = 12, 8.0, 0.95   # the defaults of gmr_amd.dataset.retime_to_torque_limits
VARIANTS = [(False, False), (True, False), (False, True), (True, True)]   # (floor, align_end)
G1 = "unitree_g1"
LOOP_SEEDS, LOOP_FRAMES, LOOP_FPS = (0, 1, 2, 5), 120, 30.0


class Case(NamedTuple):
    tau: np.ndarray
    tau_static: np.ndarray
    offs: np.ndarray
    limit: np.ndarray
    scale: float
    window: int
    max_stretch: float
    floor: Optional[np.ndarray]
    align: bool


@functools.lru_cache(maxsize=None)
def case(model, layout, floor=False, align=True):
    nh, offs = MODELS[model], LAYOUTS[layout]
    n = int(offs[-1])
    rng = np.random.default_rng(100 * nh + len(layout))
    lim = rng.uniform(20.0, 90.0, nh)
    lim[rng.random(nh) < 0.15] = np.inf                                  # hinges without a limit
    base = np.where(np.isfinite(lim), lim, 50.0)
    g = rng.uniform(-0.7, 0.7, (n, nh)) * base
    g[rng.random((n, nh)) < 0.02] *= 2.0                                 # gravity alone at 0 .. 1.4 of the limit: some beyond it
    d = rng.normal(0.0, 0.25, (n, nh)) * base
    d[rng.random((n, nh)) < 0.03] *= 6.0                                 # bursts: needs of 2 .. 4
    d[rng.random((n, nh)) < 0.004] *= 300.0                              # ... and a few beyond the cap of 8
    tau = g + d
    fl = None
    if floor:
        fl = rng.uniform(0.0, 2.5, n)                                    # above and below the torque need
    for a in (tau, g, lim) + ((fl,) if floor else ()):
        a.setflags(write=False)
    return Case(tau, g, offs, lim, SCALE, WINDOW, MAX_STRETCH, fl, bool(align))


@functools.lru_cache(maxsize=None)
def reference(model, layout, floor=False, align=True):
    c = case(model, layout, floor, align)
    p = TR.plan(c.tau, c.tau_static, c.offs, c.limit, c.scale, c.window, c.max_stretch, c.floor, c.align)
    for a in p.values():
        a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def loop_clips(quiet=True):
    """(rob, tab, qpos, offsets): dynamics_reference.Trajectory(G1, seed) for LOOP_SEEDS, 120 frames at 30 fps, as four clips, and --
    with ``quiet`` -- a fifth that stands still: under every limit."""
    from tests import dynamics_reference as DR
    rob, tab = DR.model(G1)
    t = [k / LOOP_FPS for k in range(LOOP_FRAMES)]
    parts = [DR.Trajectory(rob, seed).state(t)[0] for seed in LOOP_SEEDS]
    if quiet:
        parts.append(di.standing(G1, 40))
    q = np.concatenate(parts)
    q.setflags(write=False)
    return rob, tab, q, np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def wide_model():
    """The compiled model of a chain of WIDE_BODIES bodies, every one but the base on a hinge: nq = 7 + 63 = WIDE_NQ, more columns
    than a wavefront has lanes.  MJCF text of this module's own, in the manner of tests/synthetic_trees.mjcf_text and .compiled."""
    import os
    import tempfile
    from gmr_amd.ik_config import IKConfig, IKTask
    from gmr_amd.mjcf import load_mjcf
    from gmr_amd.model import compile_model
    inertial = '<inertial pos="0 0 0" mass="0.5" fullinertia="0.002 0.002 0.002 0 0 0"/>'
    axes = ("1 0 0", "0 1 0", "0 0 1")
    body = lambda b: f'<body name="b{b}" pos="0.02 0 0.05"><joint name="j{b}" axis="{axes[b % 3]}" range="-1.2 1.4"/>{inertial}'   # noqa: E731
    text = ('<mujoco model="wide"><compiler angle="radian"/><worldbody><body name="base" pos="0 0 1"><freejoint/>' + inertial
            + "".join(body(b) for b in range(1, WIDE_BODIES)) + "</body>" * WIDE_BODIES + "</worldbody></mujoco>\n")
    wide_model.keep = d = tempfile.TemporaryDirectory(prefix="gmr_wide_")
    path = os.path.join(d.name, "wide.xml")
    with open(path, "w") as f:
        f.write(text)
    rob = load_mjcf(path, name="wide")
    assert rob.nbody == WIDE_BODIES and rob.nq == WIDE_NQ
    tasks = [IKTask(f, h, 50.0, 10.0, [0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]) for f, h in (("base", "h_base"), ("b1", "h_tip"))]
    cfg = IKConfig("base", "h_base", 0.0, 1.8, True, True, {"h_base": 1.0, "h_tip": 1.0}, tasks, list(tasks), source="synthetic")
    return compile_model(rob, cfg)

"""The inputs of the retiming tests and their reference answers, each computed once (tests/retime_reference.py).

The library is tests/dynamics_inputs.explicit's: clips of 0, 1, 2, 3, 4, 63, 64, 65 and 130 frames at 64 Hz, 332 rows -- the empty
clip, the short ones, and the edges of the kernels' 64-row tiles and 16-row batches -- on unitree_g1 (nq 36) and booster_k1 (nq 29).
``top`` is the library's largest hinge speed, ``col_top`` each hinge's own.  A case is a named (qpos, offsets, fps, vmax, window,
max_stretch)."""
import functools
from typing import NamedTuple

import numpy as np

from tests import dynamics_inputs as di
from tests import dynamics_reference as DR
from tests import retime_reference as RR

LENS, OFFS, N, S, FPS = di.LENS, di.OFFS, di.N, di.S, di.FPS
ROBOTS = ["unitree_g1", "booster_k1"]
FILL = 0xA5
C63, C64, C65, C130 = 5, 6, 7, 8          # the clips of 63, 64, 65 and 130 frames
LONG = (C63, C64, C65, C130)
WINDOW, MAX_STRETCH = 4, 8.0              # the defaults of gmr_amd.dataset.retime_to_limits
CASES = ["identity", "uniform", "columns", "wide", "cap", "burst", "striding"]   # a .. g
STRIDING_CLIPS, STRIDING_SHORT, STRIDING_LONG = 300, 5, 1000


class Case(NamedTuple):
    q: np.ndarray
    offs: np.ndarray
    fps: float
    vmax: np.ndarray
    window: int
    max_stretch: float


def qpos(robot, seed0=0):
    """[N, nq] float64, read-only."""
    return di.explicit(robot, seed0)[0]


def speeds(q, offs, fps):
    """[nh]: every hinge's largest |dq| fps over the intervals of the clips."""
    top = np.zeros(q.shape[1] - 7)
    for a, b in zip(offs[:-1], offs[1:]):
        if b - a > 1:
            top = np.maximum(top, (np.abs(np.diff(q[a:b, 7:], axis=0)) * fps).max(axis=0))
    return top


@functools.lru_cache(maxsize=None)
def col_top(robot):
    return speeds(qpos(robot), OFFS, FPS)


def top(robot):
    return float(col_top(robot).max())


def wander(robot, frames, seed):
    """[frames, nq]: hinges on sines inside their ranges, a root that drifts and turns about z -- plain float64, no reference needed."""
    rob = DR.model(robot)[0]
    rng = np.random.default_rng(1000 + seed)
    hinges = sorted((int(b) for b in rob.hinge_bodies()), key=lambda b: int(rob.qpos_adr[b]))
    lo = np.array([rob.jnt_range[b, 0] if rob.jnt_limited[b] else -1.0 for b in hinges])
    hi = np.array([rob.jnt_range[b, 1] if rob.jnt_limited[b] else 1.0 for b in hinges])
    t = np.arange(frames)[:, None] / FPS
    q = np.zeros((frames, rob.nq))
    q[:, :3] = rng.uniform(-1, 1, 3) + t * rng.uniform(-0.5, 0.5, 3) + [0.0, 0.0, 0.9]
    yaw = rng.uniform(-3, 3) + t[:, 0] * rng.uniform(-1.5, 1.5)
    q[:, 3], q[:, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
    q[:, 7:] = 0.5 * (lo + hi) + 0.45 * (hi - lo) * rng.uniform(0.3, 1.0, len(hinges)) * np.sin(rng.uniform(2.0, 9.0, len(hinges)) * t + rng.uniform(0, 6.28, len(hinges)))
    return q


@functools.lru_cache(maxsize=None)
def striding_library(robot):
    """STRIDING_CLIPS clips of five frames and, in their middle, one of a thousand: with one wavefront per clip every wavefront of the
    long clip's row strides over 16 tiles."""
    lens = [STRIDING_SHORT] * (STRIDING_CLIPS // 2) + [STRIDING_LONG] + [STRIDING_SHORT] * (STRIDING_CLIPS - STRIDING_CLIPS // 2)
    q = np.concatenate([wander(robot, n, s) for s, n in enumerate(lens)])
    q.setflags(write=False)
    return q, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def burst_library(robot):
    """130 standing frames whose last hinge steps by 0.5 rad between rows 63 and 64: one fast interval, on the tile's edge."""
    q = di.standing(robot, 130)
    q[64:, -1] += 0.5
    q.setflags(write=False)
    return q, np.array([0, 130], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def case(robot, name):
    q, offs = qpos(robot), OFFS
    nh = q.shape[1] - 7
    if name == "identity":       # a: limits nothing reaches
        return Case(q, offs, FPS, np.full(nh, 2.0 * top(robot)), WINDOW, MAX_STRETCH)
    if name == "uniform":        # b: one limit, no window
        return Case(q, offs, FPS, np.full(nh, 0.6 * top(robot)), 0, MAX_STRETCH)
    if name == "columns":        # c: half of each column's own top speed
        return Case(q, offs, FPS, np.where(col_top(robot) > 0.0, 0.5 * col_top(robot), np.inf), WINDOW, MAX_STRETCH)
    if name == "wide":           # d: b with the widest window: wider than the short clips, across the 64-row edge
        return Case(q, offs, FPS, np.full(nh, 0.6 * top(robot)), 32, MAX_STRETCH)
    if name == "cap":            # e: a cap that binds
        return Case(q, offs, FPS, np.full(nh, 0.3 * top(robot)), WINDOW, 1.5)
    if name == "burst":          # f
        q, offs = burst_library(robot)
        return Case(q, offs, FPS, np.full(nh, 3.0 * np.pi), 8, MAX_STRETCH)
    if name == "striding":       # g
        q, offs = striding_library(robot)
        return Case(q, offs, FPS, np.full(nh, 0.6 * float(speeds(q, offs, FPS).max())), WINDOW, MAX_STRETCH)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(robot, name):
    """(plan dict, qpos_out, src_time, out_offsets, slerped) of the numpy restatement, read-only."""
    c = case(robot, name)
    p, out, st, oo, sl = RR.retime(c.q, c.offs, c.fps, c.vmax, c.window, c.max_stretch)
    for a in list(p.values()) + [out, st, oo, sl]:
        a.setflags(write=False)
    return p, out, st, oo, sl

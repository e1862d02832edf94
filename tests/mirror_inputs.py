"""The inputs of the mirror-augmentation tests and their reference answers, each computed once (tests/mirror_reference.py).

The trajectories of tests/dynamics_inputs.explicit: clips of 0, 1, 2, 3, 4, 63, 64, 65 and 130 frames in one call, 332 rows -- the
empty clip, the short ones, and the edges of the kernel's 64-row tile and 16-row batches -- on unitree_g1 (nq 36), booster_k1 (nq 29,
the fewest columns: 35 idle lanes) and unitree_g1_with_hands (nq 50)."""
import functools

import numpy as np

from gmr_amd.symmetry import plan_symmetry
from tests import dynamics_inputs as di
from tests import dynamics_reference as R
from tests import mirror_reference as MR

LENS, OFFS, N, S, ROBOTS = di.LENS, di.OFFS, di.N, di.S, di.ROBOTS
FILL = 0xA5
MODES = ("world", "start")


@functools.lru_cache(maxsize=None)
def plan(robot):
    return plan_symmetry(R.model(robot)[0])


def qpos(robot, seed0=0):
    """[N, nq] float64, read-only."""
    return di.explicit(robot, seed0)[0]


@functools.lru_cache(maxsize=None)
def reference(robot, mode, seed0=0):
    q = qpos(robot, seed0)
    out = MR.world_clips(plan(robot), q, OFFS) if mode == "world" else MR.clip_start(plan(robot), q, OFFS)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def vertical(robot):
    """Two clips of 5 rows whose first rows point the root's x axis straight up and straight down (f_xy = 0 exactly: a rotation
    about y by -+ 90 degrees written with w = y = 2^-1/2 rounded, for which 1 - 2 (y y + z z) and x y + w z are below 1e-6), the
    other rows taken from the trajectories: the psi = 0 branch."""
    q = np.array(qpos(robot)[int(OFFS[5]):int(OFFS[5]) + 10])
    h = np.sqrt(0.5)
    q[0, 3:7] = [h, 0.0, -h, 0.0]
    q[5, 3:7] = [h, 0.0, h, 0.0]
    q.setflags(write=False)
    return q, np.array([0, 5, 10], np.int64)

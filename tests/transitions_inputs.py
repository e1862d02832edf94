"""The inputs of the transition-search GPU tests.  No torch here.

The library of a window L holds clips of 0, 1, L - 1, L, L + 1, 63, 64, 65 and 130 frames: the empty clip, clips shorter than, equal
to and one longer than the window, and the edges of the pair kernel's 64 diagonals and 64-row ring.  Its rows are those of
tests/dynamics_inputs.explicit (seeds 0.. and 9..: analytic trajectories rounded once from 50 digits), cut anew: which row follows
which does not matter to the search."""
import functools

import numpy as np

from gmr_amd import transitions as tr
from tests import dynamics_inputs as di
from tests import dynamics_reference as R

ROBOTS = ["unitree_g1", "booster_k1"]
WINDOWS = [1, 2, 8]
FILL = 0xA5


def lens(L):
    return [0, 1, L - 1, L, L + 1, 63, 64, 65, 130]


@functools.lru_cache(maxsize=None)
def rows(robot):
    """[664, nq] float64, read-only."""
    q = np.concatenate([di.explicit(robot, 0)[0], di.explicit(robot, 9)[0]])
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def library(robot, L):
    """(q [N, nq] read-only, seq_offsets int64 [10])."""
    offs = np.concatenate([[0], np.cumsum(lens(L))]).astype(np.int64)
    return rows(robot)[:int(offs[-1])], offs


def model(robot):
    return R.model(robot)[0]


def all_bodies(robot):
    nb = model(robot).nbody
    return np.arange(nb, dtype=np.int32), np.ones(nb)


def tables(offs, L, src=None, dst=None, stride=1):
    return tr.search_tables(offs, src, dst, L, stride)


def written_moments(offs, n_rows, L):
    """[N, 6] bool: what the library writes of `moments`."""
    m = np.zeros((n_rows, 6), bool)
    for s in range(len(offs) - 1):
        a, b = int(offs[s]), int(offs[s + 1])
        m[a:b, :3] = True
        m[a:max(a, b - L + 1), 3:] = True
    return m


def turned(q, angle, shift):
    """qpos rows turned by ``angle`` about z and shifted by ``shift`` in xy (float64, rounded once per operation)."""
    q = np.array(q)
    c, s = np.cos(angle), np.sin(angle)
    x, y = q[:, 0].copy(), q[:, 1].copy()
    q[:, 0], q[:, 1] = c * x - s * y + shift[0], s * x + c * y + shift[1]
    hw, hz = np.cos(angle / 2.0), np.sin(angle / 2.0)
    w, qx, qy, qz = (q[:, 3 + i].copy() for i in range(4))
    q[:, 3], q[:, 4], q[:, 5], q[:, 6] = hw * w - hz * qz, hw * qx - hz * qy, hw * qy + hz * qx, hw * qz + hz * w
    return q


@functools.lru_cache(maxsize=None)
def cut_library(robot):
    """The case that fails without the feature: X, the 130-frame clip, as [X[0:80], X[60:130] turned by 1 rad and shifted by
    (3, -2)].  Returns (X, q [150, nq], seq_offsets)."""
    q, offs = library(robot, 8)
    X = np.array(q[int(offs[8]):int(offs[9])])
    assert X.shape[0] == 130
    lib = np.concatenate([X[:80], turned(X[60:], 1.0, (3.0, -2.0))])
    lib.setflags(write=False)
    X.setflags(write=False)
    return X, lib, np.array([0, 80, 150], np.int64)

"""The inputs of the clip-composition tests and their reference answers, each computed once (tests/compose_reference.py).

The library is tests/dynamics_inputs.explicit's: clips of 0, 1, 2, 3, 4, 63, 64, 65 and 130 frames, 332 rows -- the empty clip, the
short ones, and the edges of the kernel's 64-row tile and 16-row batches -- on unitree_g1 (nq 36: 28 idle lanes) and booster_k1
(nq 29: 35 idle lanes).  A case is a named (library, plan)."""
import functools

import numpy as np

from gmr_amd.compose import ComposePlan, Segment
from tests import compose_reference as CR
from tests import dynamics_inputs as di

LENS, OFFS, N, S = di.LENS, di.OFFS, di.N, di.S
ROBOTS = ["unitree_g1", "booster_k1"]
FILL = 0xA5
C63, C64, C65, C130 = 5, 6, 7, 8          # the clips of 63, 64, 65 and 130 frames
EDGE_FRAMES = 20


def qpos(robot, seed0=0):
    """[N, nq] float64, read-only."""
    return di.explicit(robot, seed0)[0]


def _yaw(angle):
    return np.stack([np.cos(angle / 2.0), np.zeros_like(angle), np.zeros_like(angle), np.sin(angle / 2.0)], -1)


@functools.lru_cache(maxsize=None)
def edge_library(robot):
    """Six clips of 20 frames (the rows of the 130-frame clip) whose root quaternions are rewritten: 0 faces +x exactly, (1, 0, 0, 0)
    in every row; 1 faces -x exactly, (0, 0, 0, 1): a relative turn of exactly pi; 2 and 3 wobble about the headings pi - 1e-3 and
    -pi + 1e-3, on the two sides of +-pi; 4 keeps its rows but points the root's x axis straight up in its anchor row 2 (f_xy = 0:
    the psi = 0 convention); 5 wobbles about the heading 2.5 (cos < 0, a half angle by the other branch)."""
    a = int(OFFS[C130])
    q = np.array(qpos(robot)[a:a + 6 * EDGE_FRAMES])
    k = np.arange(EDGE_FRAMES)
    wob = 0.01 * np.sin(0.7 * k)
    q[0:20, 3:7] = [1.0, 0.0, 0.0, 0.0]
    q[20:40, 3:7] = [0.0, 0.0, 0.0, 1.0]
    q[40:60, 3:7] = _yaw(np.pi - 1e-3 + wob)
    q[60:80, 3:7] = _yaw(-np.pi + 1e-3 + wob)
    h = np.sqrt(0.5)
    q[82, 3:7] = [h, 0.0, -h, 0.0]
    q[100:120, 3:7] = _yaw(2.5 + wob)
    q.setflags(write=False)
    return q, np.arange(7, dtype=np.int64) * EDGE_FRAMES


@functools.lru_cache(maxsize=None)
def negated_library(robot):
    """The library with every root quaternion of the 64-frame clip negated: the same rotations."""
    q = np.array(qpos(robot))
    q[int(OFFS[C64]):int(OFFS[C64 + 1]), 3:7] *= -1.0
    q.setflags(write=False)
    return q


def _whole(s):
    return Segment(s, 0, LENS[s])


def _long_chain():
    """130 segments of 12 frames of the four long clips, begins moving, blend 3."""
    return [Segment((C63, C64, C65, C130)[i % 4], (5 * i) % 50, 12) for i in range(130)]


@functools.lru_cache(maxsize=None)
def case(robot, name):
    """(q [n, nq] read-only, ComposePlan) of a named case."""
    q, offs = qpos(robot), OFFS
    if name == "whole":          # a: one segment = a whole clip, every clip with frames in its order: the input's bytes
        plan = ComposePlan(offs, [[_whole(s)] for s in range(S) if LENS[s]])
    elif name == "blend1":       # b: two segments, blend 1; also two one-frame segments that are all overlap
        plan = ComposePlan(offs, [[_whole(C63), _whole(C64)], [Segment(1, 0, 1), Segment(1, 0, 1)]], 1)
    elif name == "blend8":       # c: blend 8 across segments of 63 / 64 / 65 / 130 frames, and a second output clip
        plan = ComposePlan(offs, [[_whole(C63), _whole(C64), _whole(C65), _whole(C130), Segment(C63, 10, 40)],
                                  [Segment(C130, 20, 60), Segment(C65, 0, 30)]], 8)
    elif name == "overlap":      # d: a segment that is all overlap (6 + 4 == 10), and a blend as long as the segment before (3 == 3)
        plan = ComposePlan(offs, [[Segment(C130, 0, 20), Segment(C65, 5, 10), Segment(C64, 0, 30)], [_whole(3), Segment(C63, 0, 20)],
                                  [Segment(C130, 0, 70), _whole(C64)]], [[6, 4], [3], [64]])
    elif name == "edges":        # e: a turn of exactly pi, headings on both sides of +-pi, a root pointing straight up
        q, offs = edge_library(robot)
        plan = ComposePlan(offs, [[Segment(0, 0, 20), Segment(1, 0, 20), Segment(2, 0, 20), Segment(3, 0, 20), Segment(4, 0, 20),
                                   Segment(5, 0, 20), Segment(0, 0, 20)], [Segment(1, 0, 20), Segment(0, 0, 20)]], 4)
    elif name == "negated":      # f: a source clip with every quaternion negated
        q = negated_library(robot)
        plan = ComposePlan(offs, [[_whole(C63), _whole(C64), _whole(C65)]], 8)
    elif name == "long":         # g: 130 segments in one output clip, an output clip without segments, one of a single frame
        plan = ComposePlan(offs, [_long_chain(), [], [Segment(1, 0, 1)]], 3)
    elif name == "pieces":       # the reproduction case: the 130-frame clip cut into overlapping pieces of itself
        plan = ComposePlan(offs, [[Segment(C130, 0, 50), Segment(C130, 42, 50), Segment(C130, 84, 46)]], 8)
    else:
        raise KeyError(name)
    return q, plan


CASES = ["whole", "blend1", "blend8", "overlap", "edges", "negated", "long", "pieces"]


@functools.lru_cache(maxsize=None)
def reference(robot, name):
    """(qpos_out, seg_transform) of the numpy restatement, read-only."""
    q, plan = case(robot, name)
    out, T = CR.compose(plan, q)
    out.setflags(write=False)
    T.setflags(write=False)
    return out, T


def readers(plan, row):
    """The output rows that read source row ``row``, and of them those that read it into a blend."""
    res = []
    for o in range(plan.n_out):
        k0, k1 = int(plan.clip_segs[o]), int(plan.clip_segs[o + 1])
        for k in range(k0, k1):
            src, L, B, dst = int(plan.seg_src[k]), int(plan.seg_len[k]), int(plan.seg_blend[k]), int(plan.seg_out[k])
            nxt = int(plan.seg_blend[k + 1]) if k + 1 < k1 else 0
            j = row - src
            if 0 <= j < L - nxt:
                res.append(dst + j)
            if B:
                j = row - (int(plan.seg_src[k - 1]) + int(plan.seg_len[k - 1]) - B)
                if 0 <= j < B:
                    res.append(dst + j)
    return sorted(set(res))


# The reproduction case's deviation from the clip it was cut from, as the restatement shows it (tests/test_compose_host.py re-measures
# it: the figure covers the measurement and is less than four times it): the largest |composed - clip| over all columns.
PIECES_D = {"unitree_g1": 2.3e-16, "booster_k1": 2.3e-16}

"""Transitions between clips: the host side of the transition search (``Engine.motion_transitions``, ``gmr_motion_transitions``).
Host only: numpy, no torch.

The definition of the cost is the contract above ``gmr_transitions_input`` in include/gmr_amd.h.  Here are the tables the library
trusts (:func:`search_tables`), the choice of transitions from its result (:func:`select_transitions`) and plans for
:class:`gmr_amd.compose.ComposePlan` drawn from them (:func:`transition_walks`).

A transition ``(A, i, B, j)`` found with a window of ``L`` frames is, in a composition, ``Segment(A, a0, i + L - a0)`` followed by
``Segment(B, j, n)`` with ``blend = L``: the rows ``A[i + k]`` are cross-faded with ``B[j + k]``, ``k = 0 .. L - 1``.
"""
from __future__ import annotations

from typing import NamedTuple, Sequence

import numpy as np

from .compose import ComposeError, Segment

# Conventions, not measured on a robot: the cost is a weighted mean squared distance in m^2, so 0.0025 is points that lie 5 cm apart
# (rms) after the best planar alignment, the scale at which a cross-fade of 8 frames at 30 Hz stays within the speeds of the clips it
# joins.  The radius keeps one transition per neighbourhood of a window's length.
DEFAULT_WINDOW = 8          # matches the default blend of gmr_amd.compose.ComposePlan
DEFAULT_THRESHOLD = 0.0025  # m^2


class Transition(NamedTuple):
    """From frame ``src_frame`` of clip ``src_clip`` to frame ``dst_frame`` of clip ``dst_clip`` (window starts), at ``cost``."""

    src_clip: int
    src_frame: int
    dst_clip: int
    dst_frame: int
    cost: float


def source_count(frames: int, window: int, stride: int) -> int:
    """The sources of a clip of ``frames`` frames: the frames ``0, s, 2s, ... <= frames - window``."""
    return (int(frames) - int(window)) // int(stride) + 1 if frames >= window else 0


def search_tables(seq_offsets: Sequence[int], src_clips, dst_clips, window: int, stride: int):
    """``(src_clips int32, src_offsets int64, dst_clips int32, dst_offsets int64)`` of ``gmr_transitions_input`` for the clips of
    ``seq_offsets``: the library trusts them, so they are checked here.  ``None`` for a clip list means every clip."""
    offs = np.ascontiguousarray(seq_offsets, dtype=np.int64)
    if offs.ndim != 1 or offs.size < 1 or offs[0] != 0 or np.any(np.diff(offs) < 0):
        raise ValueError("seq_offsets must start at 0 and not go back")
    n_clips = offs.size - 1
    if int(window) < 1 or int(stride) < 1:
        raise ValueError("window and stride must be at least 1")
    frames = np.diff(offs)
    tabs = []
    for name, clips, step in (("src_clips", src_clips, int(stride)), ("dst_clips", dst_clips, 1)):
        c = np.arange(n_clips, dtype=np.int32) if clips is None else np.ascontiguousarray(clips, dtype=np.int32).reshape(-1)
        if c.size and (c.min() < 0 or c.max() >= n_clips):
            raise ValueError(f"{name} names a clip outside the {n_clips} clips")
        counts = [source_count(frames[k], window, step) for k in c]
        tabs += [c, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)]
    return tuple(tabs)


def select_transitions(best_cost, best_frame, src_clips, src_offsets, stride: int, dst_clips, threshold: float, radius: int):
    """The transitions worth taking, from the result of the search.  For every (source clip, target clip) the candidates are the
    local minima of ``best_cost`` along the source axis that are ``<= threshold``: a run of equal values whose neighbours on both
    sides are higher (or missing, or NaN) is one candidate, at its earliest frame.  A candidate is dropped when another candidate
    of the same pair of clips lies within ``radius`` source frames and is lower -- or equal and earlier.  Sources without a target
    frame (``best_frame < 0``) and NaN costs are never candidates.  Returns a list of :class:`Transition` sorted by ``(src_clip,
    src_frame, dst_clip)``."""
    cost = np.asarray(best_cost, dtype=np.float64)
    frame = np.asarray(best_frame)
    src_clips, dst_clips = np.asarray(src_clips).reshape(-1), np.asarray(dst_clips).reshape(-1)
    src_offsets = np.asarray(src_offsets, dtype=np.int64)
    if cost.ndim != 2 or cost.shape != frame.shape or cost.shape[1] != dst_clips.size or src_offsets.size != src_clips.size + 1 \
            or (cost.shape[0] != int(src_offsets[-1]) if src_offsets.size else cost.shape[0] != 0):
        raise ValueError("best_cost and best_frame must be [src_offsets[-1], len(dst_clips)]")
    stride, radius = int(stride), int(radius)
    out = []
    for a, ca in enumerate(src_clips):
        u0, u1 = int(src_offsets[a]), int(src_offsets[a + 1])
        for b, cb in enumerate(dst_clips):
            c, fr = cost[u0:u1, b], frame[u0:u1, b]
            n = c.size
            if n == 0:
                continue
            ok = ~np.isnan(c) & (fr >= 0)
            with np.errstate(invalid="ignore"):
                # runs of equal admissible values: `first` marks where one begins, `last` where it ends
                first = np.concatenate([[True], ~(ok[1:] & ok[:-1] & (c[1:] == c[:-1]))])
                u, v = np.flatnonzero(first), np.flatnonzero(np.concatenate([first[1:], [True]]))
                high = np.concatenate([[np.inf], np.where(ok, c, np.inf), [np.inf]])   # (what a neighbour counts as; a missing one too)
                cu = c[u]
                cand = u[ok[u] & (cu <= threshold) & ((u == 0) | (high[u] > cu)) & ((v == n - 1) | (high[v + 2] > cu))]
            # a candidate loses to a lower one within the radius, or to an equal and earlier one: local minima lie at least two sources
            # apart, so candidates m places apart are at least 2 m sources apart and few shifts reach across the radius
            cc, keep = c[cand], np.ones(cand.size, bool)
            for m in range(1, cand.size):
                near = (cand[m:] - cand[:-m]) * stride <= radius
                if not near.any():
                    break
                keep[:-m] &= ~(near & (cc[m:] < cc[:-m]))
                keep[m:] &= ~(near & (cc[:-m] <= cc[m:]))
            out += [Transition(int(ca), int(k) * stride, int(cb), int(fr[k]), float(c[k])) for k in cand[keep]]
    return sorted(out, key=lambda t: (t.src_clip, t.src_frame, t.dst_clip))


def transition_walks(transitions, seq_offsets: Sequence[int], n_out: int, n_segments: int, window: int, min_len: int, rng=None):
    """``n_out`` chains of ``n_segments`` segments, each a random walk along ``transitions`` (found with a window of ``window``
    frames): the result is ``ComposePlan``'s ``sequences`` for ``blend=window``, and every chain satisfies its invariants.  A walk
    starts at a uniformly drawn frame of a transition's source clip, leaves every clip through a uniformly drawn transition whose
    source frame is at least ``max(window, min_len - window)`` frames after the frame it entered at (the two blends of a segment may
    not overlap), and ends with a uniformly drawn length.  Every segment has at least ``max(min_len, window)`` frames.  Dead ends
    are backed out of; raises :class:`gmr_amd.compose.ComposeError` when no walk exists.  ``rng``: a ``numpy.random.Generator``, a
    seed or ``None``."""
    offs = np.ascontiguousarray(seq_offsets, dtype=np.int64)
    rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
    L, n_segments = int(window), int(n_segments)
    if L < 1 or n_segments < 1:
        raise ComposeError("a walk has at least one segment and a window of at least one frame")
    need = max(int(min_len), L, 1)
    frames = np.diff(offs)
    trans = [Transition(*t) for t in transitions]
    for t in trans:
        for clip, fr in ((t.src_clip, t.src_frame), (t.dst_clip, t.dst_frame)):
            if not 0 <= clip < frames.size or fr < 0 or fr + L > frames[clip]:
                raise ComposeError(f"{t}: no window of {L} frames there")
    by_src = {}
    for t in trans:
        by_src.setdefault(t.src_clip, []).append(t)
    dead = set()   # (clip, entry frame, segment index) from which no walk completes

    def extend(clip, entry, k):
        """The segments k .. n_segments - 1 of a chain that enters ``clip`` at ``entry`` with a blend (k > 0), or None."""
        if (clip, entry, k) in dead:
            return None
        if k == n_segments - 1:
            room = int(frames[clip]) - entry
            if room >= need:
                return [Segment(clip, entry, int(rng.integers(need, room + 1)))]
        else:
            exits = [t for t in by_src.get(clip, []) if t.src_frame >= entry + max(L, need - L)]
            for n in rng.permutation(len(exits)):
                t = exits[n]
                rest = extend(t.dst_clip, t.dst_frame, k + 1)
                if rest is not None:
                    return [Segment(clip, entry, t.src_frame + L - entry)] + rest
        dead.add((clip, entry, k))
        return None

    res = []
    for _ in range(int(n_out)):
        chain = None
        if n_segments == 1:
            ok = np.flatnonzero(frames >= need)
            if ok.size:
                c = int(rng.choice(ok))
                n = int(rng.integers(need, int(frames[c]) + 1))
                chain = [Segment(c, int(rng.integers(0, int(frames[c]) - n + 1)), n)]
        else:
            firsts = [t for t in trans if t.src_frame + L >= need]
            for n in rng.permutation(len(firsts)):
                t = firsts[n]
                rest = extend(t.dst_clip, t.dst_frame, 1)
                if rest is not None:
                    begin = int(rng.integers(0, t.src_frame + L - need + 1))
                    chain = [Segment(t.src_clip, begin, t.src_frame + L - begin)] + rest
                    break
        if chain is None:
            raise ComposeError(f"no walk of {n_segments} segments of at least {need} frames exists along the {len(trans)} transitions")
        res.append(chain)
    return res

"""The plan of a clip composition (``Engine.motion_compose``, ``gmr_motion_compose``): which segments of which clips follow each
other in every output clip, and over how many frames each is cross-faded into the one before it.  Host only: numpy, no torch.

The definition is the contract above ``gmr_compose_input`` in include/gmr_amd.h.  The library trusts the five tables a
:class:`ComposePlan` holds (its kernels only clamp), so every invariant of the contract is checked here, with a message that names
the segment, before a table is uploaded.
"""
from __future__ import annotations

from typing import NamedTuple, Sequence

import numpy as np


class ComposeError(ValueError):
    """A composition plan that breaks an invariant of the contract."""


class Segment(NamedTuple):
    """``length`` frames of clip ``clip``, from its frame ``begin``."""

    clip: int
    begin: int
    length: int


def _transition_blends(blend, counts):
    """One blend per transition, per output clip: ``blend`` is one int, a flat sequence over all transitions in order, or one
    sequence per output clip."""
    total = int(sum(counts))
    if not isinstance(blend, (list, tuple, np.ndarray)):
        flat = [blend] * total
    else:
        items = list(blend)
        if any(isinstance(b, (list, tuple, np.ndarray)) for b in items):
            if len(items) != len(counts):
                raise ComposeError(f"blend holds {len(items)} lists for {len(counts)} output clips")
            flat = []
            for o, (b, n) in enumerate(zip(items, counts)):
                b = list(np.atleast_1d(b))
                if len(b) != n:
                    raise ComposeError(f"output clip {o}: {len(b)} blends for {n} transitions")
                flat += b
        else:
            flat = items
    if len(flat) != total:
        raise ComposeError(f"{len(flat)} blends for {total} transitions")
    for b in flat:
        if isinstance(b, (bool, np.bool_)) or not isinstance(b, (int, np.integer)):
            raise ComposeError(f"a blend must be an int, not {b!r}")
    out, at = [], 0
    for n in counts:
        out.append([int(b) for b in flat[at:at + n]])
        at += n
    return out


class ComposePlan:
    """The tables of ``gmr_compose_input`` for ``sequences`` over the clips of ``seq_offsets``.

    ``sequences``: a list of output clips, each a list of :class:`Segment` (or ``(clip, begin, length)`` tuples); an empty list is
    an output clip without frames.  ``blend``: the frames every segment but an output clip's first overlaps with the one before it:
    one int, or one per transition (a flat sequence in order, or one sequence per output clip).

    Attributes: ``seg_src`` int64, ``seg_len`` int32, ``seg_blend`` int32, ``seg_out`` int64 ``[n_seg]``, ``clip_segs`` int64
    ``[n_out + 1]`` -- the five tables --, ``out_offsets`` int64 ``[n_out + 1]`` (the result's ``seq_offsets``), ``n_out_frames``,
    ``n_seg``, ``n_out``, ``n_frames`` (the source rows the plan was made for) and ``segments`` (the resolved ``Segment`` of every
    table row).  Raises :class:`ComposeError` naming the segment that breaks an invariant."""

    def __init__(self, seq_offsets: Sequence[int], sequences, blend=8):
        offs = np.ascontiguousarray(seq_offsets, dtype=np.int64)
        if offs.ndim != 1 or offs.size < 1 or offs[0] != 0 or np.any(np.diff(offs) < 0):
            raise ComposeError("seq_offsets must start at 0 and not go back")
        n_clips = offs.size - 1
        chains = [[Segment(*(int(v) for v in seg)) for seg in chain] for chain in sequences]
        blends = _transition_blends(blend, [max(len(c) - 1, 0) for c in chains])
        src, length, bl, out, clip_segs, out_offsets, flat = [], [], [], [], [0], [0], []
        for o, chain in enumerate(chains):
            row = out_offsets[-1]
            for i, seg in enumerate(chain):
                what = f"output clip {o}, segment {i} (clip {seg.clip}, begin {seg.begin}, length {seg.length})"
                if not 0 <= seg.clip < n_clips:
                    raise ComposeError(f"{what}: there are {n_clips} clips")
                frames = int(offs[seg.clip + 1] - offs[seg.clip])
                if seg.length < 1:
                    raise ComposeError(f"{what}: a segment has at least one frame")
                if seg.begin < 0 or seg.begin + seg.length > frames:
                    raise ComposeError(f"{what}: the clip has {frames} frames")
                b = blends[o][i - 1] if i else 0
                b_next = blends[o][i] if i + 1 < len(chain) else 0
                if i and b < 1:
                    raise ComposeError(f"{what}: a blend of {b}; a transition overlaps at least one frame")
                if b_next > seg.length:
                    raise ComposeError(f"output clip {o}, segment {i + 1}: a blend of {b_next} frames is longer than the segment "
                                       f"before it ({seg.length})")
                if b + b_next > seg.length:
                    raise ComposeError(f"{what}: the blends before and after it, {b} + {b_next} frames, are more than its length")
                if i:
                    row = out[-1] + length[-1] - b
                src.append(int(offs[seg.clip]) + seg.begin)
                length.append(seg.length)
                bl.append(b)
                out.append(row)
                flat.append(seg)
            out_offsets.append(out[-1] + length[-1] if chain else out_offsets[-1])
            clip_segs.append(len(src))
        if length and max(length) > np.iinfo(np.int32).max:
            raise ComposeError("a segment longer than 2^31 - 1 frames")
        self.seg_src = np.asarray(src, dtype=np.int64)
        self.seg_len = np.asarray(length, dtype=np.int32)
        self.seg_blend = np.asarray(bl, dtype=np.int32)
        self.seg_out = np.asarray(out, dtype=np.int64)
        self.clip_segs = np.asarray(clip_segs, dtype=np.int64)
        self.out_offsets = np.asarray(out_offsets, dtype=np.int64)
        self.n_out_frames = int(out_offsets[-1])
        self.n_seg, self.n_out, self.n_frames = len(src), len(chains), int(offs[-1])
        self.segments = flat
        for a in (self.seg_src, self.seg_len, self.seg_blend, self.seg_out, self.clip_segs, self.out_offsets):
            a.setflags(write=False)

    def tables(self):
        """The five tables by the names of ``gmr_compose_input``'s fields."""
        return {"seg_src": self.seg_src, "seg_len": self.seg_len, "seg_blend": self.seg_blend, "seg_out": self.seg_out,
                "clip_segs": self.clip_segs}

    def blended_rows(self) -> np.ndarray:
        """``[n_out_frames]`` bool: the output rows that lie in an overlap (they read two source rows)."""
        m = np.zeros(self.n_out_frames, bool)
        for o, b in zip(self.seg_out, self.seg_blend):
            m[int(o):int(o) + int(b)] = True
        return m


def random_sequences(seq_offsets: Sequence[int], n_out: int, n_segments: int, min_len: int, blend: int, rng=None):
    """``n_out`` chains of ``n_segments`` segments for augmentation: every segment a uniformly drawn clip among those of at least
    ``max(min_len, 2 blend, 1)`` frames, a uniformly drawn length from that figure up to the clip's, and a uniformly drawn begin.
    ``rng``: a ``numpy.random.Generator``, a seed or ``None``.  The result is ``ComposePlan``'s ``sequences`` for that ``blend``."""
    offs = np.ascontiguousarray(seq_offsets, dtype=np.int64)
    rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
    if int(blend) < 1:
        raise ComposeError("a transition overlaps at least one frame")
    need = max(int(min_len), 2 * int(blend), 1)
    frames = np.diff(offs)
    ok = np.flatnonzero(frames >= need)
    if ok.size == 0:
        raise ComposeError(f"no clip has the {need} frames a segment needs (min_len {min_len}, blend {blend})")
    clips = rng.choice(ok, size=(int(n_out), int(n_segments)))
    res = []
    for row in clips:
        chain = []
        for c in row:
            n = int(rng.integers(need, int(frames[c]) + 1))
            chain.append(Segment(int(c), int(rng.integers(0, int(frames[c]) - n + 1)), n))
        res.append(chain)
    return res

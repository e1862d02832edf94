"""What the BVH and SMPL-X folder loaders share: the batch they return, page-locked staging, the staged read of a group of
files and the read-ahead loop over a folder's groups.  Each loader brings its own per-file parser and its own device work."""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Dict, List, Tuple

import numpy as np
import torch

# what ``skip_errors`` leaves out: a file that cannot be read or that the loader does not understand (anything else is a bug and raises)
SKIPPABLE = (OSError, ValueError, NotImplementedError)


class ClipBatch:
    """Several clips on the GPU as one batch: ``pos [N, B, 3]``, ``quat [N, B, 4]`` (concatenated clips), ``seq_offsets``, one height
    estimate per clip -- the arguments ``retarget_batch(..., seq_offsets=..., human_heights=...)`` takes.  ``files`` are the clips' files
    in batch order; ``skipped`` lists (file, reason) of files left out (``skip_errors=True``)."""

    def __init__(self, pos, quat, names, seq_offsets, heights, files, skipped=None):
        self.pos, self.quat, self.body_names = pos, quat, names
        self.seq_offsets, self.human_heights, self.files = seq_offsets, heights, files
        self.skipped = skipped or []

    def __len__(self):
        return len(self.files)

    @classmethod
    def empty(cls, dev, skipped):
        """A batch without clips (every file of its group was left out).  The subclasses take their per-clip list between
        ``heights`` and ``files``."""
        z = lambda k: torch.empty((0, 0, k), dtype=torch.float64, device=dev)
        return cls(z(3), z(4), [], np.zeros(1, dtype=np.int64), [], [], [], list(skipped))


_PINNED: Dict[Tuple[str, int], torch.Tensor] = {}


def pinned(owner: str, slot: int) -> Callable[[int], torch.Tensor]:
    """``alloc`` for ``read_files``: a grow-only page-locked byte buffer per (owner, slot) -- two slots alternate when groups are read
    ahead.  Page-locking is what a fresh pinned allocation costs, so it is paid once per process, not once per batch."""
    def alloc(n: int) -> torch.Tensor:
        t = _PINNED.get((owner, slot))
        if t is None or t.numel() < n:
            t = torch.empty(max(n, 1 << 20) * 5 // 4, dtype=torch.uint8, pin_memory=True)
            _PINNED[(owner, slot)] = t
        return t
    return alloc


class Staged:
    """A group of files in one byte buffer: the files that survived, where each one starts and how long it is, what ``parse_one``
    made of it, the bytes staged (skipped files' included: one copy of ``buf[:total]`` moves the group) and the (file, reason) left out."""

    def __init__(self, files, buf, starts, sizes, parsed, total, skipped):
        self.files, self.buf, self.starts, self.sizes, self.parsed, self.total, self.skipped = files, buf, starts, sizes, parsed, total, skipped


def read_files(files: List[str], alloc: Callable[[int], torch.Tensor], align: int, parse_one: Callable, threads: int, skip_errors: bool) -> Staged:
    """Read the files into one byte buffer from ``alloc(nbytes)`` (``readinto``: no intermediate bytes objects), each at an
    ``align``-byte boundary, and run ``parse_one(view, path)`` on each, on ``threads`` host threads (file reads and the native
    parsers release the GIL).  ``skip_errors``: a file that cannot be read or parsed (``SKIPPABLE``) is left out and reported in
    ``.skipped`` -- the reference scripts' per-file ``try / except: print; continue`` -- instead of failing the group."""
    skipped, ok = [], []
    for f in files:
        try:
            ok.append((f, os.path.getsize(f)))
        except OSError as ex:
            if not skip_errors:
                raise
            skipped.append((f, str(ex)))
    sizes = np.array([n for _, n in ok], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum((sizes + align - 1) // align * align)]).astype(np.int64)
    buf = alloc(int(starts[-1]) + align)
    host = buf.numpy()

    def one(k):
        (f, n), a = ok[k], int(starts[k])
        view = host[a:a + n]
        try:
            with open(f, "rb", buffering=0) as fh:
                got = 0
                while got < n:
                    r = fh.readinto(memoryview(view)[got:])
                    if not r:
                        raise ValueError(f"{f}: file shrank while it was read")
                    got += r
            return parse_one(view, f)
        except SKIPPABLE as ex:
            if not skip_errors:
                raise
            return ex

    with ThreadPoolExecutor(max_workers=max(1, min(threads, len(ok)))) as ex:
        parsed = list(ex.map(one, range(len(ok))))
    keep = [k for k, p in enumerate(parsed) if not isinstance(p, Exception)]
    skipped += [(ok[k][0], str(p)) for k, p in enumerate(parsed) if isinstance(p, Exception)]
    return Staged([ok[k][0] for k in keep], buf, starts[:-1][keep], sizes[keep], [parsed[k] for k in keep], int(starts[-1]), skipped)


def read_ahead(groups: List[List[str]], read: Callable, finish: Callable):
    """Yield ``finish(read(group, slot))`` for each group in order, where group k uses slot ``k & 1``: while the caller's thread runs
    ``finish`` on group k (and the caller works on its result), one background thread reads group k + 1 into the other slot."""
    if not groups:
        return
    with ThreadPoolExecutor(max_workers=1) as bg:
        nxt = bg.submit(read, groups[0], 0)
        for k in range(len(groups)):
            got = nxt.result()
            if k + 1 < len(groups):
                nxt = bg.submit(read, groups[k + 1], (k + 1) & 1)
            yield finish(got)


def read_planned(files: List[str], alloc: Callable[[int], torch.Tensor], align: int, plan_one: Callable, fill_one: Callable, threads: int,
                 skip_errors: bool) -> Staged:
    """``read_files`` for loaders that want PARTS of their files: ``plan_one(path) -> (parsed, nbytes)`` looks at a file's directory and
    says how many bytes of the buffer it needs, then ``fill_one(path, parsed, view)`` reads just those parts into its ``nbytes``-long,
    ``align``-ed region (both on ``threads`` host threads).  ``sizes`` of the result are the regions' lengths; a file that fails in
    either step is left out with ``skip_errors`` exactly as ``read_files`` leaves it out."""
    def guarded(fn):
        def run(*a):
            try:
                return fn(*a)
            except SKIPPABLE as ex:
                if not skip_errors:
                    raise
                return ex
        return run
    with ThreadPoolExecutor(max_workers=max(1, min(threads, len(files)))) as ex:
        plans = list(ex.map(guarded(plan_one), files))
        ok = [k for k, p in enumerate(plans) if not isinstance(p, Exception)]
        sizes = np.array([plans[k][1] for k in ok], dtype=np.int64)
        starts = np.concatenate([[0], np.cumsum((sizes + align - 1) // align * align)]).astype(np.int64)
        buf = alloc(int(starts[-1]) + align)
        host = buf.numpy()
        filled = list(ex.map(guarded(lambda i: fill_one(files[ok[i]], plans[ok[i]][0], host[int(starts[i]):int(starts[i]) + int(sizes[i])])), range(len(ok))))
    bad = {ok[i]: f for i, f in enumerate(filled) if isinstance(f, Exception)}
    bad.update({k: p for k, p in enumerate(plans) if isinstance(p, Exception)})
    keep = [i for i in range(len(ok)) if ok[i] not in bad]
    skipped = [(files[k], str(bad[k])) for k in sorted(bad)]
    return Staged([files[ok[i]] for i in keep], buf, starts[:-1][keep], sizes[keep], [plans[ok[i]][0] for i in keep], int(starts[-1]), skipped)

"""Mirror augmentation: the time of one Engine.motion_mirror call (one kernel) in both modes, the bytes it moves and its share of the
HBM roofline.

    python tools/mirror_bench.py [--clips 2048] [--frames 3000] [--repeats 21] [--warmup 3] [--out profiles/mirror_bench.json]

Workload: unitree_g1 (nq 36) with its own symmetry plan, `clips` clips x `frames` frames of the random-walk qpos of
tools/track_bench.py (the figure is a time, not a result).  Timed between two HIP events on an otherwise idle stream, a caller-owned
output, the cached plan and device-resident offsets (no allocation, no upload inside the window), the two modes alternating.  Every
figure is the median of `repeats` after `warmup`, with min and max.

The bytes are stated, not measured: every row is read once and written once, 2 x 8 x nq bytes (the seven doubles of a clip's first
row that GMR_MIRROR_CLIP_START reads per wavefront come out of the cache and are not counted).  The roofline is the 8.0 TB/s HBM3E
peak of the MI355X; a plain device-to-device copy of the same bytes (torch's copy_) is timed beside it as the yardstick of what a
copy reaches on the day.  Informational: nothing gates on it.  Prints one JSON line and writes it to --out."""
from __future__ import annotations

import argparse
import datetime
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.contact_bench import _stats, _timed  # noqa: E402
from tools.track_bench import smooth_qpos  # noqa: E402

HBM_PEAK_BYTES_PER_S = 8.0e12


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--robot", default="unitree_g1")
    ap.add_argument("--out", default=os.path.join("profiles", "mirror_bench.json"))
    args = ap.parse_args(argv)
    from gmr_amd import GeneralMotionRetargeting
    g = GeneralMotionRetargeting("smplx", args.robot, device=0)
    eng = g._engine
    dev = eng.device
    plan = eng.symmetry_plan()
    offs = np.arange(args.clips + 1, dtype=np.int64) * args.frames
    offs_dev = torch.from_numpy(offs).to(dev)
    qpos = smooth_qpos(eng.nq, args.clips, args.frames, dev)
    N = int(qpos.shape[0])
    out = torch.empty_like(qpos)
    runs = {"world": lambda: eng.motion_mirror(qpos, offs_dev, plan=plan, about="world", out=out),
            "start": lambda: eng.motion_mirror(qpos, offs_dev, plan=plan, about="start", out=out),
            "copy": lambda: out.copy_(qpos)}
    for _ in range(args.warmup):
        for fn in runs.values():
            fn()
    ms = {k: [] for k in runs}
    for _ in range(args.repeats):  # alternating
        for k, fn in runs.items():
            ms[k].append(_timed(fn))
    # what was timed is the mirror: twice over in the world plane it is the input again, bit for bit
    once = eng.motion_mirror(qpos, offs_dev, plan=plan, about="world")
    twice = eng.motion_mirror(once, offs_dev, plan=plan, about="world")
    torch.cuda.synchronize()
    involution = bool(torch.equal(twice.view(torch.uint8), qpos.view(torch.uint8))) and not bool(torch.equal(once, qpos))
    st = {k: _stats(v) for k, v in ms.items()}
    moved = 2 * 8 * eng.nq * N
    rate = lambda k: moved / (st[k]["ms_median"] * 1e-3)   # noqa: E731
    line = {"workload": f"{args.robot}, nq {eng.nq}, {args.clips} clips x {args.frames} frames ({N} frames)",
            "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "warmup": args.warmup,
            "frames": N, "bytes_moved": moved, "bytes_per_row": 2 * 8 * eng.nq,
            "world_device_events": st["world"], "clip_start_device_events": st["start"], "torch_copy_device_events": st["copy"],
            "world_bytes_per_s": round(rate("world"), 1), "clip_start_bytes_per_s": round(rate("start"), 1), "torch_copy_bytes_per_s": round(rate("copy"), 1),
            "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
            "world_fraction_of_hbm_roofline": round(rate("world") / HBM_PEAK_BYTES_PER_S, 4),
            "clip_start_fraction_of_hbm_roofline": round(rate("start") / HBM_PEAK_BYTES_PER_S, 4),
            "torch_copy_fraction_of_hbm_roofline": round(rate("copy") / HBM_PEAK_BYTES_PER_S, 4),
            "frames_per_s_world": round(N / (st["world"]["ms_median"] * 1e-3), 1), "frames_per_s_clip_start": round(N / (st["start"]["ms_median"] * 1e-3), 1),
            "mirrored_twice_is_the_input": involution}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

"""Foot locking: the time of one Engine.motion_footlock call next to the Engine.motion_track call on the same qpos.

    python tools/footlock_bench.py [--clips 2048] [--frames 3000] [--repeats 21] [--warmup 5] [--out profiles/footlock_bench.json]

Workload: that of tools/contact_bench.py -- unitree_g1, `clips` clips x `frames` frames of smooth qpos, the two ankle roll links as
contact bodies -- with synthetic labels at qpos's own frames: each foot planted for 24 of every 48 frames, the two feet half a
period apart, so every frame is solved for one foot or the other or lies on a ramp.  The default parameters (W = 5, min_run = 2,
8 iterations).  The foot-locking call alone and the export (30 fps -> 50 Hz) alone are timed in the same process, alternating, each
between two HIP events on an otherwise idle stream, caller-owned outputs and device-resident offsets (no allocation, no upload
inside the window).  Every figure is the median of `repeats` after `warmup`, with min and max.  The bytes the call needs are
counted from the shapes: qpos in and out, the labels, pos and shift written by the first kernel, read and written by the second
and read by the third.  Informational: nothing gates on it.  Prints one JSON line and writes it to --out."""
from __future__ import annotations

import argparse
import datetime
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.contact_bench import FEET, HBM_BYTES_PER_S, _stats, _timed  # noqa: E402
from tools.track_bench import smooth_qpos  # noqa: E402

PERIOD = 48


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--robot", default="unitree_g1")
    ap.add_argument("--out", default=os.path.join("profiles", "footlock_bench.json"))
    args = ap.parse_args(argv)
    if args.repeats < 20:
        ap.error("--repeats must be at least 20")
    from gmr_amd import GeneralMotionRetargeting
    g = GeneralMotionRetargeting("smplx", args.robot, device=0)
    eng = g._engine
    dev = eng.device
    names = list(g.model.body_names)
    ids = [names.index(b) for b in FEET]
    offs = np.arange(args.clips + 1, dtype=np.int64) * args.frames
    offs_dev = torch.from_numpy(offs).to(dev)
    qpos = smooth_qpos(eng.nq, args.clips, args.frames, dev)
    N, S, Cn = int(qpos.shape[0]), args.clips, len(FEET)
    k = torch.arange(N, device=dev) % args.frames
    labels = torch.stack([(k % PERIOD) < PERIOD // 2, ((k + PERIOD // 2) % PERIOD) < PERIOD // 2], dim=1).to(torch.uint8).contiguous()
    res = eng.motion_footlock(qpos, offs_dev, labels, ids)
    out = {k: torch.empty_like(v) for k, v in res.items()}
    track = eng.motion_track(qpos, offs, 30.0, 50.0)
    lock = lambda: eng.motion_footlock(qpos, offs_dev, labels, ids, out=out)  # noqa: E731
    export = lambda: eng.motion_track(qpos, offs, 30.0, 50.0, out=dict(track))  # noqa: E731
    for _ in range(args.warmup):
        lock(), export()
    l_ms, t_ms = [], []
    for _ in range(args.repeats):  # alternating
        l_ms.append(_timed(lock))
        t_ms.append(_timed(export))
    torch.cuda.synchronize()
    same = all(torch.equal(out[k].view(torch.uint8), res[k].view(torch.uint8)) for k in res)   # bit-reproducible
    solved = int((res["shift"].abs().amax(dim=2) > 0).sum())
    bytes_needed = N * eng.nq * 8 * 2 + N * Cn + N * Cn * 3 * 8 * (2 + 3 + 2) + solved * 6 * 8
    Ls, Ts = _stats(l_ms), _stats(t_ms)
    line = {"workload": f"{args.robot}, {args.clips} clips x {args.frames} frames ({N} frames), contact bodies {FEET}, synthetic labels "
                        f"(each foot planted {PERIOD // 2} of every {PERIOD} frames), default parameters",
            "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "warmup": args.warmup,
            "frames": N, "solved_frame_columns": solved, "motion_footlock_device_events": Ls, "motion_track_device_events": Ts,
            "footlock_over_track": round(Ls["ms_median"] / Ts["ms_median"], 4),
            "footlock_frames_per_s": round(N / (Ls["ms_median"] * 1e-3), 1),
            "footlock_algorithmic_bytes": bytes_needed,
            "footlock_fraction_of_8TBps_hbm": round(bytes_needed / (Ls["ms_median"] * 1e-3) / HBM_BYTES_PER_S, 5),
            "residual_max": float(res["residual_max"].max()), "shift_max": float(res["shift_max"].max()),
            "limit_frames": int(res["limit_frames"].sum()), "repeated_calls_identical": bool(same)}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

"""Contact labels: the time of one Engine.motion_contacts call next to the Engine.motion_track call whose arrays it reads.

    python tools/contact_bench.py [--clips 2048] [--frames 3000] [--repeats 21] [--warmup 5] [--out profiles/contact_bench.json]

Workload: unitree_g1, `clips` clips x `frames` frames at 30 fps exported at 50 Hz (the export's benchmark workload), the two ankle
roll links as contact bodies, the default thresholds, ground "clip_min" (two passes over the clip's heights).  The export runs
once into buffers that stay; then the contacts call alone and the export alone are timed in the same process, alternating, each
between two HIP events on an otherwise idle stream, caller-owned outputs and device-resident offsets and ids (no allocation, no
upload inside the window).  Every figure is the median of `repeats` after `warmup`, with min and max.  The bytes the contacts call
needs are counted from the shapes: per frame and body z twice (the minimum pass, then the labels), x, y and the velocity once,
one label byte out.  Informational: nothing gates on it.  Prints one JSON line and writes it to --out."""
from __future__ import annotations

import argparse
import datetime
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.track_bench import smooth_qpos  # noqa: E402

HBM_BYTES_PER_S = 8e12  # the figure DESIGN uses for the MI355X roofline
FEET = ["left_ankle_roll_link", "right_ankle_roll_link"]


def _stats(ms):
    ms = sorted(ms)
    return {"ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--robot", default="unitree_g1")
    ap.add_argument("--out", default=os.path.join("profiles", "contact_bench.json"))
    args = ap.parse_args(argv)
    if args.repeats < 20:
        ap.error("--repeats must be at least 20")
    from gmr_amd import GeneralMotionRetargeting
    g = GeneralMotionRetargeting("smplx", args.robot, device=0)
    eng = g._engine
    dev = eng.device
    names = list(g.model.body_names)
    offs = np.arange(args.clips + 1, dtype=np.int64) * args.frames
    qpos = smooth_qpos(eng.nq, args.clips, args.frames, dev)
    track = eng.motion_track(qpos, offs, 30.0, 50.0)
    out_offs = torch.from_numpy(track.out_offsets).to(dev)
    ids = torch.tensor([names.index(b) for b in FEET], dtype=torch.int32, device=dev)
    M, S, Cn = int(track.out_offsets[-1]), args.clips, len(FEET)
    res = eng.motion_contacts(track, out_offs, ids)
    out = {k: torch.empty_like(v) for k, v in res.items()}
    contacts = lambda: eng.motion_contacts(track, out_offs, ids, out=out)  # noqa: E731
    export = lambda: eng.motion_track(qpos, offs, 30.0, 50.0, out=dict(track))  # noqa: E731
    for _ in range(args.warmup):
        contacts(), export()
    c_ms, t_ms = [], []
    for _ in range(args.repeats):  # alternating
        c_ms.append(_timed(contacts))
        t_ms.append(_timed(export))
    torch.cuda.synchronize()
    same = all(torch.equal(out[k].view(torch.uint8), res[k].view(torch.uint8)) for k in res)   # bit-reproducible
    bytes_needed = M * Cn * (4 + 6 * 4 + 1) + S * Cn * (2 * 4 + 3 * 8) + S * 12
    Cs, Ts = _stats(c_ms), _stats(t_ms)
    line = {"workload": f"{args.robot}, {args.clips} clips x {args.frames} frames at 30 fps -> 50 Hz ({M} output frames), contact bodies {FEET}, "
                        "default thresholds, ground clip_min", "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0),
            "repeats": args.repeats, "warmup": args.warmup, "output_frames": M,
            "motion_contacts_device_events": Cs, "motion_track_device_events": Ts,
            "contacts_over_track": round(Cs["ms_median"] / Ts["ms_median"], 4),
            "contacts_frames_per_s": round(M / (Cs["ms_median"] * 1e-3), 1),
            "contacts_algorithmic_bytes": bytes_needed,
            "contacts_fraction_of_8TBps_hbm": round(bytes_needed / (Cs["ms_median"] * 1e-3) / HBM_BYTES_PER_S, 5),
            "contact_share_of_frames": round(float(res["contact"].to(torch.float64).mean()), 4),
            "repeated_calls_identical": bool(same)}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

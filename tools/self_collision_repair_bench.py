"""Self-collision repair: the time of one Engine.motion_self_collision_repair call beside one Engine.motion_self_collision call on
the same rows.

    python tools/self_collision_repair_bench.py [--clips 2048] [--frames 3000] [--repeats 21] [--warmup 3] [--out profiles/self_collision_repair_bench.json]

Workload: that of tools/self_collision_bench.py -- unitree_g1 with the default proxies (the skeleton's capsules of 0.03 m and their
default pairs), `clips` clips x `frames` frames of the random-walk qpos of tools/track_bench.py -- at the repair's defaults (16
passes, damping 1e-6 m^2, step cap 0.2 rad: conventions, not measured on a robot).  Timed between two HIP events on an otherwise idle
stream, caller-owned outputs, cached tables and device-resident offsets (no allocation, no upload inside the window): the repair
(two kernels), the repair without statistics (kernel a alone) and the report (two kernels), alternating.  Every figure is the median
of `repeats` after `warmup`, with min and max.  A frame without a violation costs the repair one evaluation, a colliding frame up
to seventeen, so the figure depends on the share of colliding frames, which is printed.  Informational: nothing gates on it.  Prints
one JSON line and writes it to --out."""
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


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--robot", default="unitree_g1")
    ap.add_argument("--out", default=os.path.join("profiles", "self_collision_repair_bench.json"))
    args = ap.parse_args(argv)
    from gmr_amd import GeneralMotionRetargeting
    g = GeneralMotionRetargeting("smplx", args.robot, device=0)
    eng = g._engine
    dev = eng.device
    caps, pairs = eng.default_proxies()
    offs_dev = torch.from_numpy(np.arange(args.clips + 1, dtype=np.int64) * args.frames).to(dev)
    qpos = smooth_qpos(eng.nq, args.clips, args.frames, dev)
    N = int(qpos.shape[0])
    res = eng.motion_self_collision_repair(qpos, offs_dev, caps, pairs)
    rep = eng.motion_self_collision(qpos, offs_dev, caps, pairs)
    out = {k: torch.empty_like(v) for k, v in res.items()}
    frame_out = {k: out[k] for k in ("qpos", "clearance_before", "clearance_after", "move")}
    rep_out = {k: torch.empty_like(v) for k, v in rep.items()}
    runs = {"repair": lambda: eng.motion_self_collision_repair(qpos, offs_dev, caps, pairs, out=out),
            "repair_kernel_a": lambda: eng.motion_self_collision_repair(qpos, offs_dev, caps, pairs, out=frame_out),
            "report": lambda: eng.motion_self_collision(qpos, offs_dev, caps, pairs, out=rep_out)}
    for _ in range(args.warmup):
        for fn in runs.values():
            fn()
    ms = {k: [] for k in runs}
    for _ in range(args.repeats):  # alternating
        for k, fn in runs.items():
            ms[k].append(_timed(fn))
    torch.cuda.synchronize()
    same = all(torch.equal(out[k].view(torch.uint8), res[k].view(torch.uint8)) for k in res)
    st = {k: _stats(v) for k, v in ms.items()}
    repaired, unresolved = int(res["repaired_frames"].sum()), int(res["unresolved_frames"].sum())
    line = {"workload": f"{args.robot}, {len(caps)} capsules, {len(pairs)} pairs, {args.clips} clips x {args.frames} frames ({N} frames)",
            "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "warmup": args.warmup,
            "frames": N, "repair_device_events": st["repair"], "repair_kernel_a_device_events": st["repair_kernel_a"],
            "report_device_events": st["report"], "repair_over_report": round(st["repair"]["ms_median"] / st["report"]["ms_median"], 2),
            "frames_per_s": round(N / (st["repair"]["ms_median"] * 1e-3), 1),
            "colliding_frames_before": int(rep["colliding_frames"].sum()), "repaired_frames": repaired, "unresolved_frames": unresolved,
            "move_max": float(res["move_max"].max()), "clearance_min_after": float(res["clearance_min_after"].min()),
            "nonfinite_frames": int(res["nonfinite_frames"].sum()), "repeated_calls_identical": bool(same)}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

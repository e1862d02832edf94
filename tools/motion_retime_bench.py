"""Retiming to velocity limits: the time of one Engine.motion_retime_plan / motion_retime_apply call pair (four kernels) and its
share of the HBM roofline.

    python tools/motion_retime_bench.py [--clips 2048] [--frames 3000] [--fps 30] [--limit 1.0] [--window 4] [--max_stretch 8]
                                        [--repeats 21] [--warmup 5] [--out profiles/motion_retime_bench.json]

Workload: unitree_g1 (nq 36), a library of `clips` clips x `frames` frames of the random-walk qpos of tools/track_bench.py (the
figure is a time, not a result): its hinges step by up to 0.05 rad a frame, 1.5 rad/s at 30 Hz, so that one limit of `limit` rad/s on
every hinge stretches most intervals a little and the output is longer than the input.  The plan, the apply and the pair back to back
alternate in one process, each timed between two HIP events on an otherwise idle stream, caller-owned outputs, offsets and limits on
the device before the window; the read-back of out_len between the two calls -- the pair's one host synchronisation -- is made once,
before the window, and is not in any figure.  Every figure is the median of `repeats` after `warmup`, with min and max.

The bytes are stated, not measured, N source rows, M output rows:
  plan    N (8 nq + 48): the need kernel reads a row and writes need; the ticks kernel reads need and writes ticks; the scan kernel
          reads ticks and need and writes cum (halo re-reads and the per-clip results are not counted)
  apply   N 8 nq + M (8 nq + 24): every source row read once (the second read of a row comes out of the cache), every output row
          written with its src_time, and ticks and cum of its interval read (the binary search's other probes are not counted)
The roofline is the 8.0 TB/s HBM3E peak of the MI355X.  Informational: nothing gates on it.  Prints one JSON line and writes it to
--out."""
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
    ap.add_argument("--fps", type=float, default=30.0)
    ap.add_argument("--limit", type=float, default=1.0, help="rad/s on every hinge")
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--max_stretch", type=float, default=8.0)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--robot", default="unitree_g1")
    ap.add_argument("--out", default=os.path.join("profiles", "motion_retime_bench.json"))
    args = ap.parse_args(argv)
    from gmr_amd import GeneralMotionRetargeting
    g = GeneralMotionRetargeting("smplx", args.robot, device=0)
    eng = g._engine
    dev, nq = eng.device, eng.nq
    offs = torch.arange(args.clips + 1, dtype=torch.int64, device=dev) * args.frames
    qpos = smooth_qpos(nq, args.clips, args.frames, dev)
    N, S = int(qpos.shape[0]), args.clips
    vmax = torch.full((nq - 7,), float(args.limit), dtype=torch.float64, device=dev)
    f64, i64 = torch.float64, torch.int64
    pout = {"need": torch.empty(N, dtype=f64, device=dev), "ticks": torch.empty(N, dtype=i64, device=dev), "cum": torch.empty(N, dtype=i64, device=dev),
            "out_len": torch.empty(S, dtype=i64, device=dev), "clip_stats": torch.empty((S, 4), dtype=i64, device=dev),
            "need_max": torch.empty(S, dtype=f64, device=dev)}
    plan_call = lambda: eng.motion_retime_plan(qpos, offs, args.fps, vmax, args.window, args.max_stretch, out=pout)   # noqa: E731
    plan = plan_call()
    out_len = plan["out_len"].cpu().numpy()                                  # the read-back, outside every window
    oo = torch.from_numpy(np.concatenate([[0], np.cumsum(out_len)]).astype(np.int64)).to(dev)
    M = int(out_len.sum())
    aout = {"qpos": torch.empty((M, nq), dtype=f64, device=dev), "src_time": torch.empty(M, dtype=f64, device=dev)}
    apply_call = lambda: eng.motion_retime_apply(qpos, offs, plan, oo, out=aout)   # noqa: E731

    def pair():
        plan_call()
        apply_call()
    runs = {"plan": plan_call, "apply": apply_call, "pair": pair}
    for _ in range(args.warmup):
        for fn in runs.values():
            fn()
    ms = {k: [] for k in runs}
    for _ in range(args.repeats):  # alternating
        for k, fn in runs.items():
            ms[k].append(_timed(fn))
    stats = plan["clip_stats"].cpu().numpy()
    st = {k: _stats(v) for k, v in ms.items()}
    moved = {"plan": N * (8 * nq + 48), "apply": N * 8 * nq + M * (8 * nq + 24)}
    moved["pair"] = moved["plan"] + moved["apply"]
    sec = lambda k: st[k]["ms_median"] * 1e-3   # noqa: E731
    line = {"workload": f"{args.robot}, nq {nq}, {S} clips x {args.frames} frames ({N} frames) at {args.fps:g} Hz, {args.limit:g} rad/s on every hinge, "
                        f"window {args.window}, max_stretch {args.max_stretch:g}: {M} output rows",
            "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "warmup": args.warmup,
            "source_rows": N, "output_rows": M, "stretch": round(M / N, 4), "stretched_intervals": int(stats[:, 0].sum()),
            "capped_intervals": int(stats[:, 1].sum()), "need_max": round(float(plan["need_max"].max()), 4),
            "plan_device_events": st["plan"], "apply_device_events": st["apply"], "pair_device_events": st["pair"],
            "bytes_moved": moved, "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
            "plan_fraction_of_hbm_roofline": round(moved["plan"] / sec("plan") / HBM_PEAK_BYTES_PER_S, 4),
            "apply_fraction_of_hbm_roofline": round(moved["apply"] / sec("apply") / HBM_PEAK_BYTES_PER_S, 4),
            "pair_fraction_of_hbm_roofline": round(moved["pair"] / sec("pair") / HBM_PEAK_BYTES_PER_S, 4),
            "source_rows_per_s": round(N / sec("pair"), 1)}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

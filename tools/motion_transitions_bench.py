"""Transition search: the time of one Engine.motion_transitions call (three kernels) beside the same result written as chunked torch
ops.

    python tools/motion_transitions_bench.py [--clips 64] [--frames 3000] [--window 8] [--stride 1] [--repeats 21] [--warmup 5]
                                             [--torch-repeats 3] [--out profiles/motion_transitions_bench.json]

Workload: unitree_g1, all bodies with equal weights, a library of `clips` clips x `frames` frames of the random-walk qpos of
tools/track_bench.py (the figure is a time, not a result) searched against itself, min_gap = window, no dense output: 64 x 3 000 frames
are 3.7e10 frame pairs.  Each thing is timed between two HIP events on an otherwise idle stream with caller-owned outputs; every
figure is the median of its repeats after `warmup`, with min and max:

  transitions  Engine.motion_transitions: points, windowed moments and the pair kernel (the tables, a few integers per clip, are
               uploaded inside the window: they are part of the call)
  torch        the pair stage alone, from the points and weights the call left: per source clip and chunk of target clips three
               float64 batched matrix products for the grams, L shifted adds for the windows, the cost, and torch.min over the
               target frames.  Its sums run in the matrix products' order, so it agrees with the kernel to rounding, not bit for bit;
               it materialises chunk x frames x frames doubles per gram, which is what the kernel exists not to do

The flops are stated, not measured, counted from the definition: per frame pair one new per-row gram (14 P: five per point for Gd
and for Gc, four for Gz), 3 L window adds and 20 for the cost.  The roofline is the 78.6 TFLOP/s float64 vector peak of the MI355X.
Informational: nothing gates on it.  Prints one JSON line and writes it to --out."""
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

FP64_VECTOR_PEAK_FLOPS = 78.6e12


def torch_pairs(points, w, clips, frames, L, min_gap, chunk):
    """(best_cost, best_frame) [clips * (frames - L + 1), clips] of equal-length clips, from points [N, P, 3]."""
    n = frames - L + 1
    X = points.view(clips, frames, -1, 3)
    wx, wy, wz = (X[..., c] * w for c in range(3))
    x, y, z = X[..., 0], X[..., 1], X[..., 2]

    def windows(t):   # [.., frames, frames] -> [.., n, n]: sums along the diagonals
        s = t[..., 0:n, 0:n].clone()
        for k in range(1, L):
            s += t[..., k:k + n, k:k + n]
        return s / L

    def rows(t):      # [clips, frames] -> [clips, n]
        s = t[:, 0:n].clone()
        for k in range(1, L):
            s += t[:, k:k + n]
        return s / L
    mx, my, q = rows(wx.sum(-1)), rows(wy.sum(-1)), rows((w * (x * x + y * y)).sum(-1))
    v = q - (mx * mx + my * my)
    zz = (wz * z).sum(-1)
    best = torch.empty((clips * n, clips), dtype=points.dtype, device=points.device)
    frame = torch.empty((clips * n, clips), dtype=torch.int64, device=points.device)
    i = torch.arange(n, device=points.device)
    band = (i[:, None] - i[None, :]).abs() < min_gap
    for a in range(clips):
        for b0 in range(0, clips, chunk):
            b1 = min(b0 + chunk, clips)
            xt, yt, zt = x[b0:b1].transpose(1, 2), y[b0:b1].transpose(1, 2), z[b0:b1].transpose(1, 2)
            gd = windows(wx[a] @ xt + wy[a] @ yt)
            gc = windows(wx[a] @ yt - wy[a] @ xt)
            gz = windows(zz[a][None, :, None] + zz[b0:b1][:, None, :] - 2.0 * (wz[a] @ zt))
            D = gd - (mx[a][None, :, None] * mx[b0:b1][:, None, :] + my[a][None, :, None] * my[b0:b1][:, None, :])
            C = gc - (mx[a][None, :, None] * my[b0:b1][:, None, :] - my[a][None, :, None] * mx[b0:b1][:, None, :])
            cost = ((v[a][None, :, None] + v[b0:b1][:, None, :]) - 2.0 * torch.sqrt(D * D + C * C) + gz).clamp_(min=0.0)
            if b0 <= a < b1:
                cost[a - b0].masked_fill_(band, float("inf"))
            m, j = cost.min(dim=2)
            best[a * n:(a + 1) * n, b0:b1], frame[a * n:(a + 1) * n, b0:b1] = m.t(), j.t()
    return best, frame


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--torch-repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--robot", default="unitree_g1")
    ap.add_argument("--out", default=os.path.join("profiles", "motion_transitions_bench.json"))
    args = ap.parse_args(argv)
    from gmr_amd import GeneralMotionRetargeting
    from gmr_amd.transitions import search_tables
    g = GeneralMotionRetargeting("smplx", args.robot, device=0)
    eng = g._engine
    dev = eng.device
    L = args.window
    offs = np.arange(args.clips + 1, dtype=np.int64) * args.frames
    qpos = smooth_qpos(eng.nq, args.clips, args.frames, dev)
    N, P = int(qpos.shape[0]), eng.nbody
    ids, w = np.arange(P, dtype=np.int32), np.ones(P)
    _, so, _, do = search_tables(offs, None, None, L, args.stride)
    E, D = int(so[-1]), args.clips
    f64 = torch.float64
    out = {"points": torch.empty((N, P, 3), dtype=f64, device=dev), "moments": torch.empty((N, 6), dtype=f64, device=dev),
           "best_cost": torch.empty((E, D), dtype=f64, device=dev), "best_frame": torch.empty((E, D), dtype=torch.int32, device=dev)}
    call = lambda: eng.motion_transitions(qpos, offs, ids, w, L, stride=args.stride, min_gap=L, out=out)   # noqa: E731
    for _ in range(args.warmup):
        call()
    ms = [_timed(call) for _ in range(args.repeats)]
    st = {"transitions": _stats(ms)}
    pairs = E * int(do[-1])
    flops = pairs * (14 * P + 3 * L + 20)
    sec = st["transitions"]["ms_median"] * 1e-3
    line = {"workload": f"{args.robot}, {P} bodies, {args.clips} clips x {args.frames} frames against themselves, window {L}, stride {args.stride}, "
                        f"min_gap {L}, no dense output: {E} sources x {int(do[-1])} target frames",
            "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "warmup": args.warmup,
            "frame_pairs": pairs, "flops_from_the_definition": flops, "transitions_device_events": st["transitions"],
            "pairs_per_s": round(pairs / sec, 1), "flops_per_s": round(flops / sec, 1), "fp64_vector_peak_flops_per_s": FP64_VECTOR_PEAK_FLOPS,
            "fraction_of_fp64_vector_peak": round(flops / sec / FP64_VECTOR_PEAK_FLOPS, 4)}
    if args.torch_repeats > 0 and args.stride == 1:
        wd = torch.from_numpy(w / w.sum()).to(dev)
        user = lambda: torch_pairs(out["points"], wd, args.clips, args.frames, L, L, args.chunk)   # noqa: E731
        user()
        tms = [_timed(user) for _ in range(args.torch_repeats)]
        t_best, t_frame = user()
        torch.cuda.synchronize()
        fin = torch.isfinite(out["best_cost"])
        line.update({"torch_pair_stage_device_events": _stats(tms), "torch_repeats": args.torch_repeats, "torch_chunk_target_clips": args.chunk,
                     "torch_over_transitions_time": round(_stats(tms)["ms_median"] * 1e-3 / sec, 2),
                     "torch_agrees": {"best_cost_max_abs": float((t_best[fin] - out["best_cost"][fin]).abs().max()),
                                      "best_frame_equal_fraction": float((t_frame == out["best_frame"]).double().mean())}})
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Retiming to torque limits: the time of one Engine.motion_retime_plan_torque call, of the cubic Engine.motion_retime_apply and of one
whole pass of dataset.retime_to_torque_limits, each beside the velocity plan / the linear apply in the same process.

    python tools/motion_retime_torque_bench.py [--clips 2048] [--frames 3000] [--fps 30] [--limit_scale 0.95] [--window 12]
                                               [--max_stretch 8] [--repeats 11] [--warmup 3] [--out profiles/motion_retime_torque_bench.json]

Workload: unitree_g1 (nq 36, 29 hinges), a library of `clips` clips x `frames` frames of the random-walk qpos of tools/track_bench.py
(the figure is a time, not a result), the torque limits of its MJCF file.  tau and tau_static are Engine.motion_dynamics' of that
qpos, made once before the windows.  plan_torque (four kernels), the velocity plan (three; 1 rad/s on every hinge, the workload of
tools/motion_retime_bench.py), the cubic and the linear apply along the torque plan alternate, each timed between two HIP events
on an otherwise idle stream with caller-owned outputs and device tables.  The pass -- two motion_dynamics calls, the plan, the
read-back of out_len and clip_stats, the cubic apply -- synchronises with the host, so it is timed on the host's clock around a device
synchronisation, allocations included.  Every figure is the median of `repeats` after `warmup`, with min and max.

The bytes are stated, not measured, N source rows, M output rows, nh hinges:
  plan_torque   N (16 nh + 52): the need kernel reads a row of tau and of tau_static and writes need and static_over; ticks and scan
                as in the velocity plan (N 40); the alignment touches 64 rows a clip and is not counted
  apply         N 8 nq + M (8 nq + 24), cubic and linear alike: the cubic's two more rows per output row are its neighbours' and are
                expected to come out of the cache (not measured)
The roofline is the 8.0 TB/s HBM3E peak of the MI355X.  Informational: nothing gates on it, and where the time goes is not claimed
without a trace.  Prints one JSON line and writes it to --out."""
from __future__ import annotations

import argparse
import datetime
import json
import os
import sys
import time

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
    ap.add_argument("--limit_scale", type=float, default=0.95)
    ap.add_argument("--window", type=int, default=12)
    ap.add_argument("--max_stretch", type=float, default=8.0)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--robot", default="unitree_g1")
    ap.add_argument("--out", default=os.path.join("profiles", "motion_retime_torque_bench.json"))
    args = ap.parse_args(argv)
    from gmr_amd import GeneralMotionRetargeting, dataset, params
    from gmr_amd.inertial import load_inertial
    g = GeneralMotionRetargeting("smplx", args.robot, device=0)
    eng = g._engine
    dev, nq = eng.device, eng.nq
    nh = nq - 7
    table = None if g.model.xml_path else load_inertial(os.path.join(ROOT, "tests", "golden", "gmr_root", "assets", params._ROBOT_XML_REL[args.robot]))
    offs = torch.arange(args.clips + 1, dtype=torch.int64, device=dev) * args.frames
    offs_host = offs.cpu().numpy()
    qpos = smooth_qpos(nq, args.clips, args.frames, dev)
    N, S = int(qpos.shape[0]), args.clips
    f64, i64 = torch.float64, torch.int64
    limit = eng.inertial_device(table)["torque_limit"]
    tau = eng.motion_dynamics(qpos, offs, args.fps, table=table, out={"tau": torch.empty((N, nh), dtype=f64, device=dev)})["tau"]
    zero = torch.zeros((N, nq - 1), dtype=f64, device=dev)
    rest = eng.motion_dynamics(qpos, offs, args.fps, qvel=zero, qacc=zero, table=table, out={"tau": torch.empty((N, nh), dtype=f64, device=dev)})["tau"]
    del zero
    vmax = torch.ones(nh, dtype=f64, device=dev)
    new = lambda: {"need": torch.empty(N, dtype=f64, device=dev), "ticks": torch.empty(N, dtype=i64, device=dev),   # noqa: E731
                   "cum": torch.empty(N, dtype=i64, device=dev), "out_len": torch.empty(S, dtype=i64, device=dev),
                   "clip_stats": torch.empty((S, 4), dtype=i64, device=dev), "need_max": torch.empty(S, dtype=f64, device=dev)}
    tout, vout = new(), new()
    tout["static_over"] = torch.empty(N, dtype=torch.int32, device=dev)
    torque_call = lambda: eng.motion_retime_plan_torque(tau, rest, offs, limit, args.limit_scale, args.window, args.max_stretch, None, True, out=tout)   # noqa: E731
    velocity_call = lambda: eng.motion_retime_plan(qpos, offs, args.fps, vmax, 4, args.max_stretch, out=vout)   # noqa: E731
    plan = torque_call()
    velocity_call()
    out_len = plan["out_len"].cpu().numpy()                                  # the read-back, outside the event windows
    oo = torch.from_numpy(np.concatenate([[0], np.cumsum(out_len)]).astype(np.int64)).to(dev)
    M = int(out_len.sum())
    aout = {"qpos": torch.empty((M, nq), dtype=f64, device=dev), "src_time": torch.empty(M, dtype=f64, device=dev)}
    cubic_call = lambda: eng.motion_retime_apply(qpos, offs, plan, oo, out=aout, interp="cubic")    # noqa: E731
    linear_call = lambda: eng.motion_retime_apply(qpos, offs, plan, oo, out=aout, interp="linear")  # noqa: E731
    runs = {"plan_torque": torque_call, "plan_velocity": velocity_call, "apply_cubic": cubic_call, "apply_linear": linear_call}
    for _ in range(args.warmup):
        for fn in runs.values():
            fn()
    ms = {k: [] for k in runs}
    for _ in range(args.repeats):  # alternating
        for k, fn in runs.items():
            ms[k].append(_timed(fn))
    stats = plan["clip_stats"].cpu().numpy()
    del aout, tout, vout, tau, rest
    torch.cuda.empty_cache()

    def one_pass():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = dataset.retime_to_torque_limits(g, qpos, offs_host, args.fps, table=table, limit_scale=args.limit_scale, window=args.window,
                                              max_stretch=args.max_stretch, passes=1)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, res
    wall = []
    for k in range(2 + min(args.repeats, 5)):
        t, res = one_pass()
        if k >= 2:
            wall.append(t)
    info = res[2]
    st = {k: _stats(v) for k, v in ms.items()}
    moved = {"plan_torque": N * (16 * nh + 52), "plan_velocity": N * (8 * nq + 48), "apply": N * 8 * nq + M * (8 * nq + 24)}
    sec = lambda k: st[k]["ms_median"] * 1e-3   # noqa: E731
    line = {"workload": f"{args.robot}, nq {nq}, {S} clips x {args.frames} frames ({N} frames) at {args.fps:g} Hz, {args.limit_scale:g} of the MJCF torque limits, "
                        f"window {args.window}, max_stretch {args.max_stretch:g}, aligned ends: {M} output rows",
            "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "warmup": args.warmup,
            "source_rows": N, "output_rows": M, "stretch": round(M / N, 4), "stretched_intervals": int(stats[:, 0].sum()),
            "capped_intervals": int(stats[:, 1].sum()), "need_max": round(float(plan["need_max"].max()), 4),
            "plan_torque_device_events": st["plan_torque"], "plan_velocity_device_events": st["plan_velocity"],
            "apply_cubic_device_events": st["apply_cubic"], "apply_linear_device_events": st["apply_linear"],
            "one_pass_host_clock": _stats(wall), "one_pass_is": "two motion_dynamics calls (tau, root_wrench and the ratio; tau alone), plan_torque, one read-back, cubic apply, one more motion_dynamics for the ratio after; allocations included",
            "one_pass_tau_ratio_before_max": round(float(info["tau_ratio_before"].max()), 4), "one_pass_tau_ratio_after_max": round(float(info["tau_ratio_after"].max()), 4),
            "bytes_moved": moved, "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
            "plan_torque_fraction_of_hbm_roofline": round(moved["plan_torque"] / sec("plan_torque") / HBM_PEAK_BYTES_PER_S, 4),
            "plan_velocity_fraction_of_hbm_roofline": round(moved["plan_velocity"] / sec("plan_velocity") / HBM_PEAK_BYTES_PER_S, 4),
            "apply_cubic_fraction_of_hbm_roofline": round(moved["apply"] / sec("apply_cubic") / HBM_PEAK_BYTES_PER_S, 4),
            "apply_linear_fraction_of_hbm_roofline": round(moved["apply"] / sec("apply_linear") / HBM_PEAK_BYTES_PER_S, 4)}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

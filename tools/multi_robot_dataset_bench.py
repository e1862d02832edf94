#!/usr/bin/env python3
"""The dataset epilogue for several robots: (a) dataset.motions_from_qpos looped over the robots (two FK launches and the torch ops
per robot) against (b) MultiRobotRetargeting.motions_from_qpos (gmr_group_motion_epilogue: one grid for every robot's tiles), on
identical qpos, for the five config-4 robots at 5 x 64 x 1000 and 5 x 1024 x 3000 frames.

    python tools/multi_robot_dataset_bench.py [--out FILE] [--repeats 7] [--sizes 64x1000,1024x3000]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/multi_robot_dataset_bench.py --trace-only
    python tools/multi_robot_dataset_bench.py --from-stats DIR/.../run_kernel_stats.csv [--out FILE]

device: both paths up to their device results, synchronised (no host copy); to_host: the full calls, motion dicts over pinned host
arrays.  Each is the median of --repeats timed runs after two warm-up runs, with min and max.  --from-stats turns a kernel-stats CSV
of a --trace-only run (both paths once at the large size) into per-kernel totals and pass 1's achieved HBM fraction.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROBOTS = ["unitree_g1", "booster_t1", "stanford_toddy", "fourier_n1", "engineai_pm01"]
HBM_PEAK = 8.0e12  # MI355X HBM3E, bytes/s


def _qpos(cm, n, seed):
    import torch
    r = cm.robot
    rng = np.random.default_rng(seed)
    hb = sorted(r.hinge_bodies(), key=lambda b: r.qpos_adr[b])
    lim = np.array(r.jnt_range, dtype=np.float64)[hb]
    q = torch.empty((n, r.nq), dtype=torch.float64, device="cuda")
    q[:, :3] = torch.randn((n, 3), dtype=torch.float64, device="cuda") * 0.5 + torch.tensor([0.0, 0.0, 0.8], device="cuda", dtype=torch.float64)
    w = torch.randn((n, 4), dtype=torch.float64, device="cuda")
    q[:, 3:7] = w / w.norm(dim=1, keepdim=True)
    u = torch.rand((n, len(hb)), dtype=torch.float64, device="cuda")
    q[:, 7:] = torch.from_numpy(lim[:, 0]).cuda() + u * torch.from_numpy(lim[:, 1] - lim[:, 0]).cuda()
    return q


def _single_device(g, qpos, offs):
    """The device part of dataset.motions_from_qpos (everything before its host copy), same calls in the same order."""
    import torch
    eng = g._engine
    N = int(qpos.shape[0])
    root_pos = qpos[:, 0:3].clone()
    root_rot = qpos[:, [4, 5, 6, 3]].contiguous()
    dof_pos = qpos[:, 7:].contiguous()
    dof32 = dof_pos.to(torch.float32)
    zeros = torch.zeros((N, 3), dtype=torch.float32, device=qpos.device)
    ident = torch.zeros((N, 4), dtype=torch.float32, device=qpos.device)
    ident[:, 3] = 1.0
    local_body_pos, _ = eng.fk(zeros, ident, dof32, want_rot=False)
    lowest = eng.fk_min_height(root_pos.to(torch.float32), root_rot.to(torch.float32), dof32, offs).to(torch.float64)
    lens = torch.from_numpy(np.diff(offs)).to(qpos.device)
    root_pos[:, 2] = root_pos[:, 2] - torch.repeat_interleave(lowest, lens) + 0.0
    nonempty = np.diff(offs) > 0
    first = torch.zeros((len(offs) - 1, 2), dtype=torch.float64, device=qpos.device)
    first[torch.from_numpy(nonempty).to(qpos.device)] = root_pos[torch.from_numpy(offs[:-1][nonempty]).to(qpos.device), :2]
    root_pos[:, :2] = root_pos[:, :2] - torch.repeat_interleave(first, lens, dim=0)
    return root_pos, root_rot, dof_pos, local_body_pos


def _time(fn, repeats):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def run(sizes, repeats, trace_only):
    import torch
    from gmr_amd import GeneralMotionRetargeting, MultiRobotRetargeting, dataset
    mr = MultiRobotRetargeting("smplx", ROBOTS, device=0)
    singles = [GeneralMotionRetargeting("smplx", r, device=0) for r in ROBOTS]
    rows = []
    for n_clips, T in sizes:
        offs = np.arange(0, n_clips * T + 1, T, dtype=np.int64)
        N = int(offs[-1])
        torch.manual_seed(0)
        qpos = {r: _qpos(cm, N, i) for i, (r, cm) in enumerate(zip(ROBOTS, mr._cms))}
        batches = [(qpos[r], offs) for r in ROBOTS]
        a_dev = lambda: [_single_device(g, qpos[r], offs) for r, g in zip(ROBOTS, singles)]  # noqa: E731
        b_dev = lambda: mr.group.motion_epilogue(batches)  # noqa: E731
        a_host = lambda: [dataset.motions_from_qpos(g, qpos[r], offs, 30) for r, g in zip(ROBOTS, singles)]  # noqa: E731
        b_host = lambda: mr.motions_from_qpos(qpos, offs, 30)  # noqa: E731
        if trace_only:
            for f in (a_dev, b_dev):
                f()
            torch.cuda.synchronize()
            continue
        frames = len(ROBOTS) * N
        row = {"clips_per_robot": n_clips, "frames_per_clip": T, "robot_frames": frames}
        for name, f in (("a_device", a_dev), ("b_device", b_dev), ("a_to_host", a_host), ("b_to_host", b_host)):
            med, lo, hi = _time(f, repeats)
            row[name] = {"median_s": med, "min_s": lo, "max_s": hi, "frames_per_s": frames / med}
            print(f"{n_clips}x{T} {name}: {frames / med:.3e} frames/s (median {med * 1e3:.2f} ms, {lo * 1e3:.2f} .. {hi * 1e3:.2f})", flush=True)
        # pass 1 algorithmic traffic: qpos row in; root_rot, dof_pos, root_pos (f64) and local_body_pos (f32) out
        bpf = [8 * cm.robot.nq + 8 * (4 + cm.robot.nq - 7 + 3) + 12 * len(cm.robot.body_names) for cm in mr._cms]
        row["pass1_bytes_per_frame"] = dict(zip(ROBOTS, bpf))
        row["pass1_bytes_total"] = int(sum(b * N for b in bpf))
        rows.append(row)
        del qpos, batches
        torch.cuda.empty_cache()
    return rows


def from_stats(path, bytes_total):
    """Kernel totals of a --trace-only run's kernel-stats CSV; pass 1's HBM fraction from its algorithmic bytes."""
    out = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            out[r["Name"]] = {"calls": int(r["Calls"]), "total_ns": int(float(r["TotalDurationNs"]))}
    pick = lambda key: {k: v for k, v in out.items() if key in k}  # noqa: E731
    res = {"kernels": {k: v for k, v in out.items() if any(s in k for s in ("motion_", "fk_pos_kernel", "fk_kernel", "fk_minkey"))}}
    ep = sum(v["total_ns"] for v in pick("motion_epilogue_kernel").values())
    fin = sum(v["total_ns"] for v in pick("motion_finish_kernel").values())
    fk = sum(v["total_ns"] for v in pick("fk_pos_kernel").values()) + sum(v["total_ns"] for v in pick("fk_kernel<1>").values())
    res.update(epilogue_total_ns=ep + fin, fk_pos_plus_min_height_ns=fk)
    if ep and bytes_total:
        res["pass1_hbm_fraction"] = bytes_total / (ep * 1e-9) / HBM_PEAK
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", default="64x1000,1024x3000")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-only", action="store_true", help="both device paths once at the largest size (for a rocprofv3 run)")
    ap.add_argument("--from-stats", default=None, help="kernel-stats CSV of a --trace-only run")
    ap.add_argument("--pass1-bytes", type=int, default=0, help="with --from-stats: pass 1's algorithmic bytes of the traced size")
    args = ap.parse_args()
    if args.from_stats:
        rec = from_stats(args.from_stats, args.pass1_bytes)
    else:
        sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
        if args.trace_only:
            sizes = sizes[-1:]
        rec = {"robots": ROBOTS, "repeats": args.repeats, "rows": run(sizes, args.repeats, args.trace_only)}
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()

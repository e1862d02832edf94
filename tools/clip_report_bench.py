"""Time the clip report against what the library offered before it for the same answer: gmr_evaluate with task_err_out plus torch
reductions.  One process, the two alternated, CUDA-event times; prints one JSON line (and writes it to --out).

    python tools/clip_report_bench.py --clips 2048 --frames 300 --rounds 10 --out profiles/clip_report_bench.json

The two sides are not the same work, and the record says so (`notes`).  The torch side reduces what gmr_evaluate returns (stage errors,
|v| and |w| of the per-task 6-vectors), the solve counts, and computes the joint and root statistics with tensor ops; it has no
prepared targets, so its position figure is |v|, not the world distance the report gives, and it only counts non-finite frames
instead of keeping them and their steps out of every statistic.  `clip_report_ms` is Engine.clip_report as a user calls it: it
includes allocating and zeroing its 14 output tensors, the host planning and the upload; `clip_report_call_ms` is the native call
alone on outputs allocated once (planning and upload still inside).  `segments` repeats that call for other segment lengths.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--robot", default="unitree_g1")
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from gmr_amd import GeneralMotionRetargeting
    g = GeneralMotionRetargeting("smplx", args.robot, device=0)
    eng, dev = g._engine, g.device
    S, T = args.clips, args.frames
    N = S * T
    gen = torch.Generator(device=dev).manual_seed(1)
    names = list(g.ik_columns)
    cols = g._columns(names)
    pos = (torch.randn((N, len(names), 3), generator=gen, device=dev) * 0.5).to(torch.float32)
    quat = torch.nn.functional.normalize(torch.randn((N, len(names), 4), generator=gen, device=dev), dim=-1).to(torch.float32)
    offs = np.arange(S + 1, dtype=np.int64) * T
    r = g.model
    hb = sorted((int(b) for b in r.hinge_bodies()), key=lambda b: int(r.qpos_adr[b]))
    lo = torch.tensor([r.jnt_range[b][0] if r.jnt_limited[b] else -np.inf for b in hb], device=dev, dtype=torch.float64)
    hi = torch.tensor([r.jnt_range[b][1] if r.jnt_limited[b] else np.inf for b in hb], device=dev, dtype=torch.float64)
    # in-range qpos: hinges uniform within their limits (+-1 rad where unlimited), unit root quaternions
    qpos = torch.randn((N, eng.nq), generator=gen, device=dev, dtype=torch.float64) * 0.3
    qpos[:, 3:7] = torch.nn.functional.normalize(qpos[:, 3:7], dim=-1)
    u = torch.rand((N, len(hb)), generator=gen, device=dev, dtype=torch.float64)
    flo, fhi = torch.where(torch.isfinite(lo), lo, -torch.ones_like(lo)), torch.where(torch.isfinite(hi), hi, torch.ones_like(hi))
    qpos[:, 7:] = flo + u * (fhi - flo)
    iters = torch.randint(2, 12, (N,), generator=gen, device=dev, dtype=torch.int32)

    def report():
        return eng.clip_report(qpos, offs, pos, quat, cols, iters=iters)

    import ctypes as C
    from gmr_amd import _native
    from gmr_amd.engine import CLIP_REPORT_LIMIT_EPS, CLIP_REPORT_SEGMENT, _report_input
    ri, rep, keep = _report_input(eng, qpos, pos, quat, cols, offs, None, iters)

    def call(segment=0):
        prm = _native.ClipReportParams(CLIP_REPORT_LIMIT_EPS, segment, 0)
        eng._check(eng._lib.gmr_clip_report(eng._h, C.byref(ri), C.byref(prm), eng._stream()), "gmr_clip_report")

    def torch_path():
        err, _, _, terr = eng.evaluate(qpos, pos, quat, cols, want_task_errors=True)
        e = err.view(S, T, 2)
        v, w = terr[..., :3].norm(dim=-1).view(S, T, -1), terr[..., 3:].norm(dim=-1).view(S, T, -1)
        q = qpos.view(S, T, -1)
        th = q[..., 7:]
        d = (th[:, 1:] - th[:, :-1]).abs().amax(1)
        rs = (q[:, 1:, :3] - q[:, :-1, :3]).norm(dim=-1).amax(1)
        dot = (q[:, 1:, 3:7] * q[:, :-1, 3:7]).sum(-1).abs().clamp(max=1.0)
        it = (iters & 0x3FFFFFFF).view(S, T)
        bad = (~(torch.isfinite(qpos).all(1) & torch.isfinite(pos[:, cols.tolist()]).all(2).all(1)
                 & torch.isfinite(quat[:, cols.tolist()]).all(2).all(1))).view(S, T).sum(1)
        return (it.amax(1), it.sum(1, dtype=torch.int64), bad, e.amax(1), e.sum(1), v.amax(1), v.sum(1), w.amax(1), w.sum(1), (th - lo <= 1e-3).sum(1), (hi - th <= 1e-3).sum(1), d, rs,
                (2.0 * torch.acos(dot)).amax(1))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    sweep = [1, 4, 8, 16, CLIP_REPORT_SEGMENT, 64, 128, T]
    for _ in range(2):
        report(); torch_path(); call()
        for sg in sweep:
            call(sg)
    torch.cuda.synchronize()
    t_rep, t_ref, t_call, t_seg = [], [], [], {sg: [] for sg in sweep}
    for _ in range(args.rounds):
        t_rep.append(timed(report))
        t_ref.append(timed(torch_path))
        t_call.append(timed(call))
        for sg in sweep:  # (alternated with the rest, round by round)
            t_seg[sg].append(timed(lambda: call(sg)))
    nt, nh, B = eng.info.ntask[0] + eng.info.ntask[1], eng.nq - 7, len(names)
    read = N * (eng.nq * 8 + B * 7 * 4 + 4)
    seg = CLIP_REPORT_SEGMENT
    rows = S * -(-T // seg) * (9 + 4 * nt + 3 * nh) * 8
    res = {"robot": args.robot, "clips": S, "frames_per_clip": T, "frames": N, "rounds": args.rounds,
           "clip_report_ms_median": float(np.median(t_rep)), "clip_report_ms_min": float(np.min(t_rep)),
           "evaluate_plus_torch_ms_median": float(np.median(t_ref)), "evaluate_plus_torch_ms_min": float(np.min(t_ref)),
           "clip_report_frames_per_s": N / (float(np.median(t_rep)) * 1e-3),
           "clip_report_call_ms_median": float(np.median(t_call)), "clip_report_call_ms_min": float(np.min(t_call)),
           "segments": {str(sg): {"call_ms_median": float(np.median(v)), "call_ms_min": float(np.min(v))} for sg, v in t_seg.items()},
           "segment_frames_default": seg,
           "bytes_read_inputs": read, "clip_report_bytes_rows_written": rows, "clip_report_bytes_rows_written_and_reread": 2 * rows,
           "clip_report_row_bytes_per_frame_written": rows / N,
           "notes": "clip_report_ms includes allocating and zeroing the 14 output tensors, host planning and upload; clip_report_call_ms "
                    "is the native call on preallocated outputs; the evaluate path has no world-distance figure and only counts "
                    "non-finite frames",
           "evaluate_bytes_written_per_frame": (2 + 6 * nt) * 8, "evaluate_bytes_written": N * (2 + 6 * nt) * 8}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

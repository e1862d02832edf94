"""Tracking export: the fused call (Engine.motion_track) against the unfused composition on the same device.

    python tools/track_bench.py [--clips 8192] [--frames 3000] [--batch_clips 512] [--repeats 7] [--warmup 2] [--lowpass_hz HZ] [--out FILE]

Workload: unitree_g1, `clips` clips x `frames` frames at 30 fps, resampled to 50 fps and to 30 fps.  Both sides run the workload
as consecutive batches of `batch_clips` clips into result tensors allocated once (8192 x 3000 frames at 50 fps are 41 M output
frames x 2.1 KB); every batch reads the same smooth random qpos, which does not change what is timed.  The composition is
what a user of the package writes without the call: a torch lerp and slerp on index tensors, Engine.fk(want_rot=True) on the
float32 casts, and torch differences; its index tensors (i0, i1, a, km, kp, h) are built outside the timed region.  Timing: HIP
events around the whole workload, `warmup` untimed runs, the median of `repeats` runs (min and max alongside).  Prints one JSON line.

With --lowpass_hz the fused call is also timed with the low-pass on (`fused_lowpass`: one more kernel per batch, in front of the
export), and what a user does without it is timed once for one batch (`host_filtfilt_one_batch`): qpos to the host,
scipy.signal.filtfilt per clip (all columns at once; the root quaternion made sign-continuous first and normalised after), and
back to the device.  The filter kernel's own duration comes from a kernel trace of its own:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/track_bench.py --lowpass_hz 6 --trace_only
"""
from __future__ import annotations

import argparse
import datetime
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8e12  # the figure DESIGN uses for the MI355X roofline


def smooth_qpos(nq: int, clips: int, frames: int, device, seed: int = 0) -> torch.Tensor:
    g = torch.Generator(device=device).manual_seed(seed)
    u = lambda *sh: torch.rand(*sh, generator=g, device=device, dtype=torch.float64) * 2 - 1
    q = torch.empty((clips, frames, nq), dtype=torch.float64, device=device)
    q[..., :3] = u(clips, 1, 3) + torch.cumsum(u(clips, frames, 3) * 0.02, dim=1)
    w = u(clips, 1, 4) + torch.cumsum(u(clips, frames, 4) * 0.02, dim=1)
    q[..., 3:7] = w / w.norm(dim=-1, keepdim=True)
    q[..., 7:] = (u(clips, 1, nq - 7) * 0.5 + torch.cumsum(u(clips, frames, nq - 7) * 0.05, dim=1)).clamp(-1.5, 1.5)
    return q.reshape(clips * frames, nq)


def composition_plan(offs, out_offs, ratio, fps_out, device):
    """Index tensors of the unfused path (host loop over clips, outside the timed region)."""
    i0s, i1s, As, kms, kps = [], [], [], [], []
    for s in range(len(offs) - 1):
        T, M = int(offs[s + 1] - offs[s]), int(out_offs[s + 1] - out_offs[s])
        u = np.arange(M, dtype=np.float64) * ratio[s]
        i0 = np.minimum(np.floor(u).astype(np.int64), T - 1)
        i1 = np.minimum(i0 + 1, T - 1)
        k = np.arange(M)
        i0s.append(offs[s] + i0); i1s.append(offs[s] + i1); As.append(np.where(i1 > i0, u - i0, 0.0))
        kms.append(out_offs[s] + np.maximum(k - 1, 0)); kps.append(out_offs[s] + np.minimum(k + 1, M - 1))
    cat = lambda xs: torch.from_numpy(np.concatenate(xs)).to(device)
    km, kp = cat(kms), cat(kps)
    return cat(i0s), cat(i1s), cat(As), km, kp, (kp - km).to(torch.float64) / fps_out


def _rotvec(p, q):
    """rotvec(p (x) conj(q)) for xyzw tensors [..., 4] (float64)."""
    pv, pw, qv, qw = p[..., :3], p[..., 3:], q[..., :3], q[..., 3:]
    w = pw * qw + (pv * qv).sum(-1, keepdim=True)
    v = qw * pv - pw * qv - torch.linalg.cross(pv, qv)
    sgn = torch.where(w < 0, -1.0, 1.0)
    w, v = w * sgn, v * sgn
    n = v.norm(dim=-1, keepdim=True)
    return torch.where(n > 1e-12, v * (2.0 * torch.atan2(n, w) / n.clamp_min(1e-300)), 2.0 * v)


def composition(eng, q, plan, out_pos, out_rot):
    """The unfused path on one batch; returns the ten arrays."""
    i0, i1, a, km, kp, h = plan
    x0, x1 = q[i0], q[i1]
    a1 = a[:, None]
    lerp = x0 + a1 * (x1 - x0)
    root_pos, joint_pos = lerp[:, :3].contiguous(), lerp[:, 7:].contiguous()
    q0, q1 = x0[:, [4, 5, 6, 3]], x1[:, [4, 5, 6, 3]]
    d = (q0 * q1).sum(-1, keepdim=True)
    q1 = torch.where(d < 0, -q1, q1)
    # (the contract in include/gmr_amd.h also copies q0 when q0 == q1 in all four components; this composition returns q0 / |q0| there,
    #  an ulp beside it -- the smooth clips of this benchmark hold no identical neighbouring rows)
    om = torch.acos(d.abs().clamp_max(1.0))
    so = torch.sin(om)
    small = om < 1e-8
    w0 = torch.where(small, 1.0 - a1, torch.sin((1.0 - a1) * om) / so)
    w1 = torch.where(small, a1, torch.sin(a1 * om) / so)
    r = w0 * q0 + w1 * q1
    root_rot = torch.where(a1 == 0, q0, r / r.norm(dim=-1, keepdim=True))
    bp, br = eng.fk(root_pos.to(torch.float32), root_rot.to(torch.float32), joint_pos.to(torch.float32), want_rot=True,
                    out_pos=out_pos, out_rot=out_rot)
    hh = torch.where(h == 0, torch.inf, h)
    root_lin = (root_pos[kp] - root_pos[km]) / hh[:, None]
    joint_vel = (joint_pos[kp] - joint_pos[km]) / hh[:, None]
    root_ang = _rotvec(root_rot[kp], root_rot[km]) / hh[:, None]
    body_lin = ((bp[kp].to(torch.float64) - bp[km].to(torch.float64)) / hh[:, None, None]).to(torch.float32)
    body_ang = (_rotvec(br[kp].to(torch.float64), br[km].to(torch.float64)) / hh[:, None, None]).to(torch.float32)
    return root_pos, root_rot, joint_pos, root_lin, root_ang, joint_vel, bp, br, body_lin, body_ang


def host_filtfilt(q: torch.Tensor, offs, fs: float, fc: float) -> torch.Tensor:
    """The host route for one batch, copies included: the same filter through scipy, clip by clip."""
    from scipy import signal
    b, a = signal.butter(2, 2 * fc / fs)
    x = q.cpu().numpy()
    out = np.empty_like(x)
    for s in range(len(offs) - 1):
        c = x[offs[s]:offs[s + 1]].copy()
        w = c[:, 3:7]
        flip = np.cumprod(np.where(np.sum(w[1:] * w[:-1], axis=1) < 0, -1.0, 1.0))  # (the sign of each row against its corrected predecessor)
        w[1:] *= flip[:, None]
        c = signal.filtfilt(b, a, c, axis=0, padlen=min(9, c.shape[0] - 1))
        c[:, 3:7] /= np.linalg.norm(c[:, 3:7], axis=1, keepdims=True)
        out[offs[s]:offs[s + 1]] = c
    return torch.from_numpy(out).to(q.device)


def timed(fn, warmup: int, repeats: int):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--clips", type=int, default=8192)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--batch_clips", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--robot", default="unitree_g1")
    ap.add_argument("--lowpass_hz", type=float, default=None, help="also time the fused call with the low-pass at this cutoff, and the host route once")
    ap.add_argument("--trace_only", action="store_true", help="with --lowpass_hz: the filtered fused call over the workload three times at "
                    "30 -> 50 fps and nothing else (for a rocprofv3 --kernel-trace run)")
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args(argv)
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    if args.trace_only and args.lowpass_hz is None:
        ap.error("--trace_only needs --lowpass_hz")
    from gmr_amd import GeneralMotionRetargeting
    from gmr_amd.engine import TRACK_FIELDS
    from gmr_amd.schedule import track_plan
    g = GeneralMotionRetargeting("smplx", args.robot, device=0)
    eng = g._engine
    dev = eng.device
    bc = min(args.batch_clips, args.clips)
    n_batches = (args.clips + bc - 1) // bc
    offs = np.arange(bc + 1, dtype=np.int64) * args.frames
    q = smooth_qpos(eng.nq, bc, args.frames, dev)
    nd, nb = eng.nq - 7, eng.nbody
    res = {"workload": f"{args.robot}, {n_batches} x {bc} clips x {args.frames} frames at 30 fps", "date": datetime.date.today().isoformat(),
           "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "warmup": args.warmup, "cases": []}
    for fps_out in (50.0, 30.0):
        out_offs, ratio = track_plan(offs, 30.0, fps_out)
        M = int(out_offs[-1])
        frames_out = M * n_batches
        bytes_per_frame = float(ratio[0]) * eng.nq * 8 + (2 * (3 + nd) + 4 + 3) * 8 + nb * (3 + 4 + 3 + 3) * 4
        shapes = {"root_pos": (M, 3), "root_rot": (M, 4), "joint_pos": (M, nd), "root_lin_vel": (M, 3), "root_ang_vel": (M, 3), "joint_vel": (M, nd),
                  "body_pos_w": (M, nb, 3), "body_quat_w": (M, nb, 4), "body_lin_vel_w": (M, nb, 3), "body_ang_vel_w": (M, nb, 3)}
        out = {k: torch.empty(shapes[k], dtype=torch.float32 if k.startswith("body_") else torch.float64, device=dev) for k in TRACK_FIELDS}

        def fused():
            for _ in range(n_batches):
                eng.motion_track(q, offs, 30.0, fps_out, out=out)

        def fused_lowpass():
            for _ in range(n_batches):
                eng.motion_track(q, offs, 30.0, fps_out, out=out, lowpass_hz=args.lowpass_hz)
        if args.trace_only:
            for _ in range(3):
                fused_lowpass()
            torch.cuda.synchronize()
            return 0
        plan = composition_plan(offs, out_offs, ratio, fps_out, dev)
        bp, br = torch.empty_like(out["body_pos_w"]), torch.empty_like(out["body_quat_w"])

        def unfused():
            for _ in range(n_batches):
                composition(eng, q, plan, bp, br)
        # the two sides compute the same thing (the composition's torch slerp may differ in the last bits)
        fused()
        ref = composition(eng, q, plan, bp, br)
        worst = max(float((out[k].to(torch.float64) - r.to(torch.float64)).abs().max()) for k, r in zip(TRACK_FIELDS, ref))
        case = {"fps_in": 30.0, "fps_out": fps_out, "output_frames": frames_out, "algorithmic_bytes_per_output_frame": round(bytes_per_frame, 1),
                "max_abs_difference_fused_vs_composition": worst}
        sides = [("fused", fused), ("composition", unfused)]
        if args.lowpass_hz is not None:
            # the filtered call is the plain call on the filtered qpos, and the host route computes the same filtered qpos
            import time
            from gmr_amd import dataset
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            qh = host_filtfilt(q, offs, 30.0, args.lowpass_hz)
            torch.cuda.synchronize()
            host_s = time.perf_counter() - t0
            qs = dataset.smooth_qpos(g, q, offs, 30.0, args.lowpass_hz)
            case["lowpass_hz"] = args.lowpass_hz
            case["max_abs_difference_device_vs_host_filtfilt"] = float((qs - qh).abs().max())
            case["host_filtfilt_one_batch"] = {"s": round(host_s, 3), "clips": bc, "note": "device -> host, scipy.signal.filtfilt per clip, host -> device; once"}
            fused_lowpass()
            plain = eng.motion_track(qs, offs, 30.0, fps_out)
            case["filtered_call_equals_plain_call_on_filtered_qpos"] = all(bool(torch.equal(out[k], plain[k])) for k in TRACK_FIELDS)
            del qh, qs, plain
            sides.insert(1, ("fused_lowpass", fused_lowpass))
        for name, fn in sides:
            med, lo, hi = timed(fn, args.warmup, args.repeats)
            print(f"30 -> {fps_out:g} fps, {name}: {med:.2f} ms (median of {args.repeats})", file=sys.stderr, flush=True)
            fps = frames_out / (med * 1e-3)
            case[name] = {"ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3), "output_frames_per_s": round(fps, 1),
                          "fraction_of_8TBps_hbm": round(fps * bytes_per_frame / HBM_BYTES_PER_S, 4)}
        case["speedup_fused_over_composition"] = round(case["composition"]["ms_median"] / case["fused"]["ms_median"], 2)
        if args.lowpass_hz is not None:
            case["lowpass_ms_per_workload"] = round(case["fused_lowpass"]["ms_median"] - case["fused"]["ms_median"], 3)
        res["cases"].append(case)
        del out, bp, br, plan, ref
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

"""Motion library: the fused query (MotionLibrary.query -> gmr_motion_sample, one kernel) against the composition a user would
write without it, on the same device.

    python tools/motion_sample_bench.py [--clips 2048] [--frames 3000] [--repeats 21] [--warmup 5] [--out profiles/motion_sample_bench.json]

Workload: unitree_g1, a library of `clips` clips x `frames` frames at 30 fps kept as qpos; query sets E x K of {4096 x 1, 4096 x 5,
65536 x 1} (K future times per environment), random ids and times, with all bodies and with a 14-body subset; float32 times and
float32 outputs, as a trainer holds them.

A, the fused call, is measured two ways: as a user calls it -- MotionLibrary.query(out=..., check=False), time.perf_counter around
the call plus a synchronise (host to host) -- and on the device: HIP events around `--burst` back-to-back calls, divided by their
number (the kernel's time where it is longer than an enqueue -- it was at every size measured -- the enqueue rate otherwise).
B is the composition: the plan as torch ops on the ids and times (a trainer's times change every step), torch gathers, lerp and
slerp on those indices, the two stencils, Engine.fk(want_rot=True) on the float32 casts, and a torch loop over the bodies for
the twist -- the same ten fields, host to host the same way.  A and B alternate inside one run; every figure is the median of
`repeats` after `warmup`, with min and max.  Their agreement is checked once per case, outside the timed region.
Prints one JSON line and writes it to --out.  The kernel's own duration comes from a trace run of its own:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/motion_sample_bench.py --trace-only
(ten dispatches of motion_sample_kernel per case, in the order of the cases).
"""
from __future__ import annotations

import argparse
import datetime
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.track_bench import _rotvec, smooth_qpos  # noqa: E402

HBM_BYTES_PER_S = 8e12  # the figure DESIGN uses for the MI355X roofline
GEN = ("root_pos", "root_rot", "joint_pos", "root_lin_vel", "root_ang_vel", "joint_vel")
BODY = ("body_pos_w", "body_quat_w", "body_lin_vel_w", "body_ang_vel_w")


def _slerp(q0, q1, a1):
    d = (q0 * q1).sum(-1, keepdim=True)
    q1 = torch.where(d < 0, -q1, q1)
    om = torch.acos(d.abs().clamp_max(1.0))
    so = torch.sin(om)
    small = om < 1e-8
    w0 = torch.where(small, 1.0 - a1, torch.sin((1.0 - a1) * om) / so)
    w1 = torch.where(small, a1, torch.sin(a1 * om) / so)
    r = w0 * q0 + w1 * q1
    return torch.where(a1 == 0, q0, r / r.norm(dim=-1, keepdim=True))


def _rotate(q, v):
    """Rotation of v by the xyzw quaternion q (float32 tensors)."""
    qv, qw = q[..., :3], q[..., 3:]
    v = v.expand_as(qv)
    t = 2.0 * torch.linalg.cross(qv, v)
    return v + qw * t + torch.linalg.cross(qv, t)


class Composition:
    """What a user writes today: plan, gathers, lerp / slerp, stencils, Engine.fk, a loop over the bodies."""

    def __init__(self, gmr, lib, body_cols):
        rob = gmr.model
        self.eng, self.lib = gmr._engine, lib
        dev = self.eng.device
        self.parent = [int(p) for p in rob.parent]
        hinge = set(int(b) for b in rob.hinge_bodies())
        self.dof = [int(rob.qpos_adr[b]) - 7 if b in hinge else -1 for b in range(rob.nbody)]
        self.axis = torch.tensor(np.asarray(rob.jnt_axis), dtype=torch.float32, device=dev)
        self.cols = None if body_cols is None else torch.tensor(body_cols, dtype=torch.int64, device=dev)
        self.lens = lib._offs_dev[1:] - lib._offs_dev[:-1]

    def __call__(self, ids, times):
        lib, q = self.lib, self.lib.qpos
        if times.dim() == 2:
            ids = ids[:, None].expand(times.shape).reshape(-1)
        lead, t = tuple(times.shape), times.reshape(-1).to(torch.float64)
        sb, T, f = lib._offs_dev[ids], self.lens[ids], lib._fps_dev[ids]
        u = t * f
        i0 = torch.floor(u.clamp(min=0.0)).to(torch.int64).clamp(max=T - 1)
        i1 = (i0 + 1).clamp(max=T - 1)
        a = torch.where((i1 > i0) & (u > 0), u - i0, 0.0)[:, None]
        km0, kp1, km1 = (i0 - 1).clamp(min=0), (i1 + 1).clamp(max=T - 1), (i1 - 1).clamp(min=0)
        h0, h1 = ((i1 - km0) / f)[:, None], ((kp1 - km1) / f)[:, None]
        xm0, x0, x1, xp1, xm1 = q[sb + km0], q[sb + i0], q[sb + i1], q[sb + kp1], q[sb + km1]
        pose = x0 + a * (x1 - x0)
        v0, v1 = (x1 - xm0) / h0, (xp1 - xm1) / h1
        vel = v0 + a * (v1 - v0)
        xyzw = [4, 5, 6, 3]
        root_rot = _slerp(x0[:, xyzw], x1[:, xyzw], a)
        w0, w1 = _rotvec(x1[:, xyzw], xm0[:, xyzw]) / h0, _rotvec(xp1[:, xyzw], xm1[:, xyzw]) / h1
        root_ang = w0 + a * (w1 - w0)
        root_pos, joint_pos, root_lin, joint_vel = pose[:, :3], pose[:, 7:], vel[:, :3], vel[:, 7:]
        rp32, rr32, jp32 = root_pos.to(torch.float32), root_rot.to(torch.float32), joint_pos.to(torch.float32)
        X, R = self.eng.fk(rp32, rr32, jp32, want_rot=True)
        jv32 = joint_vel.to(torch.float32)
        V, W = [root_lin.to(torch.float32)], [root_ang.to(torch.float32)]
        for j in range(1, len(self.parent)):  # the loop over bodies
            p = self.parent[j]
            V.append(V[p] + torch.linalg.cross(W[p], X[:, j] - X[:, p]))
            W.append(W[p] if self.dof[j] < 0 else W[p] + _rotate(R[:, j], self.axis[j]) * jv32[:, self.dof[j], None])
        V, W = torch.stack(V, dim=1), torch.stack(W, dim=1)
        if self.cols is not None:
            X, R, V, W = X[:, self.cols], R[:, self.cols], V[:, self.cols], W[:, self.cols]
        out = {"root_pos": rp32, "root_rot": rr32, "joint_pos": jp32, "root_lin_vel": root_lin.to(torch.float32),
               "root_ang_vel": root_ang.to(torch.float32), "joint_vel": jv32, "body_pos_w": X, "body_quat_w": R, "body_lin_vel_w": V,
               "body_ang_vel_w": W}
        return {k: v.reshape(lead + tuple(v.shape[1:])) for k, v in out.items()}


def _host_to_host(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def _stats(us):
    us = sorted(us)
    return {"us_median": round(us[len(us) // 2], 2), "us_min": round(us[0], 2), "us_max": round(us[-1], 2)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--burst", type=int, default=50, help="back-to-back calls between the two HIP events of the device figure")
    ap.add_argument("--robot", default="unitree_g1")
    ap.add_argument("--trace-only", action="store_true", help="every case's fused call ten times and nothing else (for a rocprofv3 "
                    "--kernel-trace run of its own: the kernel's own duration per case, in launch order)")
    ap.add_argument("--out", default=os.path.join("profiles", "motion_sample_bench.json"))
    args = ap.parse_args(argv)
    if args.repeats < 20:
        ap.error("--repeats must be at least 20")
    from gmr_amd import GeneralMotionRetargeting, MotionLibrary
    g = GeneralMotionRetargeting("smplx", args.robot, device=0)
    eng = g._engine
    dev = eng.device
    offs = np.arange(args.clips + 1, dtype=np.int64) * args.frames
    lib = MotionLibrary(g, smooth_qpos(eng.nq, args.clips, args.frames, dev), offs, 30.0)
    names = list(g.model.body_names)
    subset = [names[i] for i in np.linspace(0, len(names) - 1, 14).round().astype(int)]
    nd = eng.nq - 7
    res = {"workload": f"{args.robot}, library {args.clips} clips x {args.frames} frames at 30 fps ({lib.qpos.numel() * 8 / 1e9:.2f} GB of qpos), "
                       "float32 times and outputs", "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "warmup": args.warmup, "burst": args.burst, "cases": []}
    gen = torch.Generator(device=dev).manual_seed(1)
    for E, K in ((4096, 1), (4096, 5), (65536, 1)):
        ids = lib.sample_ids(E, generator=gen)
        t0 = lib.sample_times(ids, generator=gen).to(torch.float32)
        future = None if K == 1 else torch.arange(K, dtype=torch.float32, device=dev) * 0.02
        times = t0 if K == 1 else t0[:, None] + future
        for label, bodies in (("all bodies", None), ("14 bodies", subset)):
            ncol = eng.nbody if bodies is None else len(bodies)
            out = {k: torch.empty_like(v) for k, v in lib.query(ids, t0, future=future, bodies=bodies, check=False).items()}
            fused = lambda: lib.query(ids, t0, future=future, bodies=bodies, out=out, check=False)  # noqa: E731
            comp = Composition(g, lib, None if bodies is None else [names.index(b) for b in bodies])
            unfused = lambda: comp(ids, times)  # noqa: E731
            if args.trace_only:
                for _ in range(10):
                    fused()
                torch.cuda.synchronize()
                continue
            fused()
            ref = unfused()
            agree = {k: float((out[k].to(torch.float64) - ref[k].to(torch.float64)).abs().max()) for k in GEN + BODY}
            for _ in range(args.warmup):
                fused(), unfused()
            a_us, b_us, d_us = [], [], []
            for _ in range(args.repeats):  # alternating
                a_us.append(_host_to_host(fused))
                b_us.append(_host_to_host(unfused))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.burst):
                    fused()
                e1.record()
                e1.synchronize()
                d_us.append(e0.elapsed_time(e1) * 1e3 / args.burst)
            Q = E * K
            bytes_q = 4 * eng.nq * 8 + 8.0 / K + 4 + (2 * (3 + nd) + 4 + 3) * 4 + ncol * (3 + 4 + 3 + 3) * 4
            A, B, D = _stats(a_us), _stats(b_us), _stats(d_us)
            case = {"E": E, "K": K, "bodies": label, "queries": Q, "algorithmic_bytes_per_query": round(bytes_q, 1),
                    "fused_host_to_host": A, "composition_host_to_host": B, "fused_device_events_per_call_in_a_burst": D,
                    "ratio_fused_over_composition": round(A["us_median"] / B["us_median"], 4),
                    "fused_queries_per_s_device": round(Q / (D["us_median"] * 1e-6), 1),
                    "fused_fraction_of_8TBps_hbm_device": round(Q * bytes_q / (D["us_median"] * 1e-6) / HBM_BYTES_PER_S, 5),
                    "max_abs_difference_fused_vs_composition": agree}
            print(f"E={E} K={K} {label}: fused {A['us_median']:.1f} us host-to-host, {D['us_median']:.1f} us per call in a burst; "
                  f"composition {B['us_median']:.1f} us", file=sys.stderr, flush=True)
            res["cases"].append(case)
            del out, ref
    if args.trace_only:
        return 0
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

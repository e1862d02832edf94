"""Clip composition: the time of one Engine.motion_compose call (two kernels) beside the mirror augmentation on as many rows and the
torch composition a user would write.

    python tools/motion_compose_bench.py [--clips 2048] [--frames 3000] [--segments 4] [--blend 8] [--repeats 21] [--warmup 5]
                                         [--out profiles/motion_compose_bench.json]

Workload: unitree_g1 (nq 36), a library of `clips` clips x `frames` frames of the random-walk qpos of tools/track_bench.py (the
figure is a time, not a result), random chains of `segments` segments and blend `blend` (gmr_amd.compose.random_sequences, seed 0),
as many of them as give at most the library's rows.  Three things alternate in one process, each timed between two HIP events on an
otherwise idle stream, caller-owned outputs, tables uploaded before the window; every figure is the median of `repeats` after
`warmup`, with min and max:

  compose  Engine.motion_compose: the plan kernel and the row kernel
  mirror   Engine.motion_mirror in "start" mode on the same number of rows with the composed clips' offsets: the same mapping and
           nearly the same bytes -- the yardstick
  torch    the composition written as torch ops: the placements by a loop over the position in the chain (vectorised over the
           chains), one gather of the rows, the maps, and lerp / slerp on the blended rows.  Its index tensors are built before the
           window, as the plan's tables are

The bytes are stated, not measured: every output row is written once and read once, a blended row read twice,
8 nq (2 rows + blended rows) bytes (tables, placements and anchor rows are not counted).  The roofline is the 8.0 TB/s HBM3E peak of
the MI355X.  Informational: nothing gates on it.  Prints one JSON line and writes it to --out."""
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


def _heading(r):
    r = r / r.norm(dim=-1, keepdim=True)
    w, x, y, z = r.unbind(-1)
    fx, fy = 1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y + w * z)
    h = torch.sqrt(fx * fx + fy * fy)
    flat = h * h < 1e-12
    return torch.where(flat, torch.ones_like(h), fx / h), torch.where(flat, torch.zeros_like(h), fy / h)


def _place(q, c, s, tx, ty, hw, hz):
    out = q.clone()
    out[:, 0] = c * q[:, 0] - s * q[:, 1] + tx
    out[:, 1] = s * q[:, 0] + c * q[:, 1] + ty
    w, x, y, z = q[:, 3], q[:, 4], q[:, 5], q[:, 6]
    out[:, 3], out[:, 4], out[:, 5], out[:, 6] = hw * w - hz * z, hw * x - hz * y, hw * y + hz * x, hw * z + hz * w
    return out


class TorchComposition:
    """The composition as torch ops, for chains of equal length (what random_sequences draws)."""

    def __init__(self, plan, segments, device):
        dev = lambda a: torch.from_numpy(np.array(a)).to(device)   # noqa: E731
        K = plan.n_seg
        self.n_chain, self.segments = K // segments, segments
        seg = np.repeat(np.arange(K), [int(n) for n in self._rows(plan)])
        j = np.concatenate([np.arange(int(n)) for n in self._rows(plan)])
        self.seg, self.src = dev(seg), dev(plan.seg_src[seg] + j)
        bl = j < plan.seg_blend[seg]
        self.blended = dev(np.flatnonzero(bl))
        sb, jb = seg[bl], j[bl]
        self.prev_seg = dev(sb - 1)
        self.prev_src = dev(plan.seg_src[sb - 1] + plan.seg_len[sb - 1] - plan.seg_blend[sb] + jb)
        u = (jb + 1.0) / (plan.seg_blend[sb] + 1.0)
        self.w = dev(u * u * (3.0 - 2.0 * u))
        a = plan.seg_blend // 2
        k = np.arange(K)
        self.anchor_b = dev(plan.seg_src + a)
        self.anchor_a = dev(np.where(plan.seg_blend > 0, plan.seg_src[k - 1] + plan.seg_len[k - 1] - plan.seg_blend + a, 0))

    @staticmethod
    def _rows(plan):
        nxt = np.concatenate([plan.seg_blend[1:], [0]])
        return plan.seg_len - nxt

    def __call__(self, q):
        C, S = self.n_chain, self.segments
        va, vb = q[self.anchor_a, :7].view(C, S, 7), q[self.anchor_b, :7].view(C, S, 7)
        ca, sa = _heading(va[..., 3:7])
        cb, sb = _heading(vb[..., 3:7])
        cd, sd = ca * cb + sa * sb, sa * cb - ca * sb
        tdx = va[..., 0] - (cd * vb[..., 0] - sd * vb[..., 1])
        tdy = va[..., 1] - (sd * vb[..., 0] + cd * vb[..., 1])
        T = torch.zeros((C, S, 6), dtype=q.dtype, device=q.device)
        T[:, 0, 0] = T[:, 0, 4] = 1.0
        for i in range(1, S):   # the chain, position by position
            c, s, tx, ty, hw, hz = T[:, i - 1].unbind(-1)
            c1, s1 = c * cd[:, i] - s * sd[:, i], s * cd[:, i] + c * sd[:, i]
            n = torch.sqrt(c1 * c1 + s1 * s1)
            c1, s1 = c1 / n, s1 / n
            half = torch.atan2(s1, c1) * 0.5
            h = torch.stack([torch.cos(half), torch.zeros_like(half), torch.zeros_like(half), torch.sin(half)], -1)
            qa = _place(va[:, i], c, s, tx, ty, hw, hz)[:, 3:7]
            qb = _place(vb[:, i], c1, s1, tx, ty, h[:, 0], h[:, 3])[:, 3:7]
            sign = torch.where((qa * qb).sum(-1) < 0, -1.0, 1.0)
            T[:, i] = torch.stack([c1, s1, (c * tdx[:, i] - s * tdy[:, i]) + tx, (s * tdx[:, i] + c * tdy[:, i]) + ty, sign * h[:, 0], sign * h[:, 3]], -1)
        T = T.view(-1, 6)
        out = _place(q[self.src], *T[self.seg].unbind(-1))
        x1 = out[self.blended]
        x0 = _place(q[self.prev_src], *T[self.prev_seg].unbind(-1))
        w = self.w[:, None]
        mix = x0 + w * (x1 - x0)
        q0, q1 = x0[:, 3:7], x1[:, 3:7]
        d = (q0 * q1).sum(-1, keepdim=True)
        q1 = torch.where(d < 0, -q1, q1)
        om = torch.acos(d.abs().clamp(max=1.0))
        so = torch.sin(om)
        small = om < 1e-8
        w0 = torch.where(small, 1.0 - w, torch.sin((1.0 - w) * om) / so)
        w1 = torch.where(small, w, torch.sin(w * om) / so)
        r = w0 * q0 + w1 * q1
        mix[:, 3:7] = r / r.norm(dim=-1, keepdim=True)
        out[self.blended] = mix
        return out, T


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--segments", type=int, default=4)
    ap.add_argument("--blend", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--robot", default="unitree_g1")
    ap.add_argument("--out", default=os.path.join("profiles", "motion_compose_bench.json"))
    args = ap.parse_args(argv)
    from gmr_amd import GeneralMotionRetargeting
    from gmr_amd.compose import ComposePlan, random_sequences
    g = GeneralMotionRetargeting("smplx", args.robot, device=0)
    eng = g._engine
    dev = eng.device
    offs = np.arange(args.clips + 1, dtype=np.int64) * args.frames
    qpos = smooth_qpos(eng.nq, args.clips, args.frames, dev)
    N = int(qpos.shape[0])
    seqs = random_sequences(offs, max(1, (2 * args.clips) // args.segments), args.segments, 2 * args.blend, args.blend, rng=0)
    plan = ComposePlan(offs, seqs, args.blend)
    while plan.n_out_frames > N:                 # the mirror runs on rows of the library: at most as many
        seqs = seqs[:max(1, int(len(seqs) * 0.95 * N / plan.n_out_frames))]
        plan = ComposePlan(offs, seqs, args.blend)
    M, n_blend = plan.n_out_frames, int(plan.seg_blend.sum())
    out, tr = torch.empty((M, eng.nq), dtype=torch.float64, device=dev), torch.empty((plan.n_seg, 6), dtype=torch.float64, device=dev)
    sym = eng.symmetry_plan()
    m_in, m_out, m_offs = qpos[:M], torch.empty((M, eng.nq), dtype=torch.float64, device=dev), torch.from_numpy(np.array(plan.out_offsets)).to(dev)
    user = TorchComposition(plan, args.segments, dev)
    runs = {"compose": lambda: eng.motion_compose(qpos, plan, out=out, transform_out=tr),
            "mirror": lambda: eng.motion_mirror(m_in, m_offs, plan=sym, about="start", out=m_out),
            "torch": lambda: user(qpos)}
    for _ in range(args.warmup):
        for fn in runs.values():
            fn()
    ms = {k: [] for k in runs}
    for _ in range(args.repeats):  # alternating
        for k, fn in runs.items():
            ms[k].append(_timed(fn))
    # what was timed is the composition: the torch version agrees with it to rounding
    t_out, t_T = user(qpos)
    torch.cuda.synchronize()
    agree = {"hinges_max_abs": float((t_out[:, 7:] - out[:, 7:]).abs().max()), "xy_max_abs": float((t_out[:, :2] - out[:, :2]).abs().max()),
             "quat_max_abs": float((t_out[:, 3:7] - out[:, 3:7]).abs().max()), "transform_max_abs": float((t_T - tr).abs().max())}
    st = {k: _stats(v) for k, v in ms.items()}
    moved = 8 * eng.nq * (2 * M + n_blend)
    sec = lambda k: st[k]["ms_median"] * 1e-3   # noqa: E731
    line = {"workload": f"{args.robot}, nq {eng.nq}, library {args.clips} clips x {args.frames} frames ({N} frames), {plan.n_out} chains of "
                        f"{args.segments} segments, blend {args.blend}: {plan.n_seg} segments, {M} output rows, {n_blend} of them blended",
            "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "warmup": args.warmup,
            "output_rows": M, "blended_rows": n_blend, "segments": plan.n_seg, "bytes_moved": moved,
            "compose_device_events": st["compose"], "mirror_start_device_events": st["mirror"], "torch_composition_device_events": st["torch"],
            "compose_rows_per_s": round(M / sec("compose"), 1), "mirror_rows_per_s": round(M / sec("mirror"), 1), "torch_rows_per_s": round(M / sec("torch"), 1),
            "compose_over_mirror_rows_per_s": round(sec("mirror") / sec("compose"), 4), "torch_over_compose_time": round(sec("torch") / sec("compose"), 2),
            "compose_bytes_per_s": round(moved / sec("compose"), 1), "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
            "compose_fraction_of_hbm_roofline": round(moved / sec("compose") / HBM_PEAK_BYTES_PER_S, 4),
            "mirror_fraction_of_hbm_roofline": round(2 * 8 * eng.nq * M / sec("mirror") / HBM_PEAK_BYTES_PER_S, 4),
            "torch_composition_agrees": agree}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

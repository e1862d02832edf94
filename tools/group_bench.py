#!/usr/bin/env python3
"""Multi-robot batch retargeting (EngineGroup) on one GPU: one JSON object on stdout.

    python tools/group_bench.py [--reps 3] [--many-clips 1024] [--out FILE]

* config4: BASELINE config 4 as stated, 5 robots x 64 clips x 1000 frames, bench.py's heterogeneous inputs, in three forms --
  the whole-clip group launch (bench.py's `heterogeneous` record), `EngineGroup.ik_solve_chunked(chunk="auto")`, and the five
  members' own `Engine.ik_solve_chunked` one after the other; frames/s, the chunk / burn-in chosen, the walks' re-solved frames,
  and the equality flags (group chunked == per-member chunked bitwise; chunked == whole clips to 1e-7, same solve counts).
* many_clips: the five robots x N distinct clips of different lengths (synth_clips_torch, any heading, 300..3000 frames), the
  group launch in array order against `launch_order="auto"` (probe and device sort included), and their bitwise equality.
Times: wall clock between device synchronisations, after one warm-up call, mean of --reps calls.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gmr_amd import params, synth  # noqa: E402
from gmr_amd.engine import EngineGroup  # noqa: E402
from gmr_amd.ik_config import load_ik_config  # noqa: E402
from gmr_amd.mjcf import load_robot  # noqa: E402
from gmr_amd.model import compile_model  # noqa: E402
from gmr_amd.schedule import make_items  # noqa: E402

ROBOTS = ["unitree_g1", "booster_t1", "stanford_toddy", "fourier_n1", "engineai_pm01"]
MASK = 0x3FFFFFFF


def timed(fn, reps):
    fn()  # warm-up
    torch.cuda.synchronize()
    ts, r = [], None
    for _ in range(reps):
        r = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.mean(ts)), r


def config4(grp, cms, dev, reps):
    offs = np.arange(65, dtype=np.int64) * 1000
    batches = []
    for cm in cms:  # bench.py heterogeneous_leg's inputs
        pos, quat, names, _, _ = synth.synth_clips(cm, 8, 1000, seed=41, hard=True, dtype=np.float32)
        batches.append((torch.from_numpy(pos).to(dev).repeat(8, 1, 1), torch.from_numpy(quat).to(dev).repeat(8, 1, 1), cm.slot_columns(names)))
    nfr = 5 * 64 * 1000
    t_whole, whole = timed(lambda: grp.ik_solve([b + (make_items(offs),) for b in batches]), reps)
    t_chunk, chunked = timed(lambda: grp.ik_solve_chunked([b + (offs,) for b in batches], "auto", 0), reps)
    chunk, burn_in = grp.last_chunk

    def members():
        return [e.ik_solve_chunked(b[0], b[1], b[2], offs, chunk, burn_in) for e, b in zip(grp.engines, batches)]
    t_mem, per = timed(members, reps)
    breakdown = chunked_breakdown(grp, batches, offs, chunk, burn_in, reps)
    bitwise = all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2] for a, b in zip(chunked, per))
    close = all(float((a[0] - w[0]).abs().max().item()) < 1e-7 and torch.equal(a[1] & MASK, w[1] & MASK) for a, w in zip(chunked, whole))
    return {
        "robots": ROBOTS, "frames": nfr,
        "whole_clip_group_frames_per_s": nfr / t_whole,
        "chunked_group_frames_per_s": nfr / t_chunk,
        "chunked_members_one_after_another_frames_per_s": nfr / t_mem,
        "chunk": chunk, "burn_in": burn_in,
        "chunks_per_robot": chunked[0][2]["chunks"],
        "resolved_frames": {r: c[2]["resolved_frames"] for r, c in zip(ROBOTS, chunked)},
        "resolved_frames_members": {r: p[2]["resolved_frames"] for r, p in zip(ROBOTS, per)},
        "chunked_breakdown": breakdown,
        "group_chunked_equals_member_chunked_bitwise": bool(bitwise),
        "chunked_equals_whole_clips_1e-7_same_solve_counts": bool(close),
    }


def chunked_breakdown(grp, batches, offs, chunk, burn_in, reps):
    """The two launches of the chunked group solve timed apart, and what bounds the second: the frames the slowest walk re-solves
    one after the other (a clip whose speculative chunks do not verify is re-solved by its walk, sequentially)."""
    from gmr_amd._native import IKParams
    from gmr_amd.schedule import plan_walks
    prm = IKParams(check_tol=1e-7)
    items = make_items(offs, chunk=chunk, burn_in=burn_in, track=True)
    walks = plan_walks(items, offs, chunk)
    dones = [torch.zeros(len(walks), dtype=torch.int32, device=b[0].device) for b in batches]
    t1, t2 = [], []
    for _ in range(reps + 1):  # (the walks overwrite the chunks' states they re-solve: every walk launch gets a fresh first launch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = grp.ik_solve([{"pos": b[0], "quat": b[1], "slot_col": b[2], "items": items, "n_final": 2 * len(items)} for b in batches], prm)
        torch.cuda.synchronize()
        t1.append(time.perf_counter() - t0)
        for d in dones:
            d.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        grp.ik_solve([{"pos": b[0], "quat": b[1], "slot_col": b[2], "items": walks, "qpos_init": q[2], "qpos_final": q[2], "out": q[0],
                       "iters": q[1], "frames_done": d} for b, q, d in zip(batches, r, dones)], prm)
        torch.cuda.synchronize()
        t2.append(time.perf_counter() - t0)
    t1, t2 = float(np.mean(t1[1:])), float(np.mean(t2[1:]))  # (the first round is the warm-up)
    worst = [int(d.max().item()) for d in dones]
    return {"launch1_chunks_ms": 1e3 * t1, "launch2_walks_ms": 1e3 * t2, "items_launch1": len(items) * len(batches),
            "walks_launch2": len(walks) * len(batches), "max_frames_resolved_by_one_walk": dict(zip(ROBOTS, worst)),
            "walks_resolving_any_frame": {r: int((d > 0).sum().item()) for r, d in zip(ROBOTS, dones)}}


def many_clips(grp, cms, dev, n_clips, reps):
    rng = np.random.default_rng(71)
    lengths = rng.integers(300, 3001, size=n_clips)
    g1 = cms[0]
    pos, quat, names, offs = synth.synth_clips_torch(g1, lengths, seed=72, device=dev, hard=rng.integers(2, size=n_clips).astype(bool))
    offs = np.asarray(offs, dtype=np.int64)
    items = make_items(offs)
    batches = [(pos, quat, cm.slot_columns(names), items) for cm in cms]
    nfr = 5 * int(offs[-1])
    pf = grp.engines[0]._probe_frames(np.concatenate([items] * len(cms)))
    t_arr, a = timed(lambda: grp.ik_solve(batches), reps)
    t_ord, o = timed(lambda: grp.ik_solve(batches, launch_order="auto"), reps)
    same = all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, o))
    return {"robots": ROBOTS, "clips_per_robot": n_clips, "lengths": [300, 3000], "frames": nfr, "probe_frames": pf,
            "array_order_frames_per_s": nfr / t_arr, "auto_order_frames_per_s": nfr / t_ord, "auto_order_gain": t_arr / t_ord - 1.0,
            "bitwise_equal": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--many-clips", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cms = [compile_model(load_robot(params.ROBOT_XML_DICT[r], name=r), load_ik_config(params.IK_CONFIG_DICT["smplx"][r])) for r in ROBOTS]
    grp = EngineGroup(cms, 0)
    res = {"device": torch.cuda.get_device_name(dev), "cus": torch.cuda.get_device_properties(dev).multi_processor_count,
           "config4": config4(grp, cms, dev, a.reps)}
    torch.cuda.empty_cache()
    res["many_clips"] = many_clips(grp, cms, dev, a.many_clips, a.reps)
    grp.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

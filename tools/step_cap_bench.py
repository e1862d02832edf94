#!/usr/bin/env python3
"""What a capped launch costs: bench.py's shaped workload (unitree_g1, 8192 clips x 3000 frames, 64 distinct clips tiled) solved by
three engines in turn, several rounds, alternating --

    uncapped   no step cap: the shaped kernel instance (the bench's headline path)
    inf_cap    a cap of +inf on every dof: the generic instance with the cap code, nothing binds, same solves per frame
               (the price of leaving the shaped instance)
    capped     use_velocity_limit=True: 3 pi rad/s on every limited hinge (the generic instance AND more solves per frame: the robot
               lags its targets, most frames run into max_iter)

One JSON line: per engine the step times (HIP events around Engine.ik_solve, launch_order="auto" as in the bench), frames/s from the
median, and the mean solves per frame.

    python tools/step_cap_bench.py [--clips 8192] [--frames 3000] [--rounds 3]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8192)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch

    from gmr_amd import params, synth
    from gmr_amd.engine import Engine
    from gmr_amd.ik_config import load_ik_config
    from gmr_amd.mjcf import load_robot
    from gmr_amd.model import compile_model, resolve_velocity_limits
    from gmr_amd.schedule import make_items
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device")
    dev = torch.device("cuda", 0)
    robot = load_robot(params.ROBOT_XML_DICT["unitree_g1"], name="unitree_g1")
    cfg = load_ik_config(params.IK_CONFIG_DICT["smplx"]["unitree_g1"])
    cm = compile_model(robot, cfg)
    cm_cap = compile_model(robot, cfg, velocity_limits=resolve_velocity_limits(robot, True))
    S, T, D = args.clips, args.frames, min(args.distinct, args.clips)
    pe, qe, names, _, _ = synth.synth_clips(cm, D // 2, T, seed=1000, hard=False, dtype=np.float32)  # bench.py's workload 1
    ph, qh, _, _, _ = synth.synth_clips(cm, D - D // 2, T, seed=2000, hard=True, dtype=np.float32)
    reps = (S + D - 1) // D
    pos = torch.from_numpy(np.concatenate([pe, ph])).to(dev).repeat(reps, 1, 1)[: S * T].contiguous()
    quat = torch.from_numpy(np.concatenate([qe, qh])).to(dev).repeat(reps, 1, 1)[: S * T].contiguous()
    items = make_items(np.arange(S + 1, dtype=np.int64) * T)
    sc = cm.slot_columns(names)
    out = torch.empty((S * T, robot.nq), dtype=torch.float64, device=dev)
    engines = {"uncapped": Engine(cm, 0), "inf_cap": Engine(cm, 0), "capped": Engine(cm_cap, 0)}
    engines["inf_cap"].set_step_cap(np.full(robot.nv, np.inf))
    res = {k: {"step_ms": []} for k in engines}

    def step(k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _, iters, _ = engines[k].ik_solve(pos, quat, sc, items, out=out)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), iters

    for k in engines:  # warm-up: code objects, pools
        step(k)
    for _ in range(args.rounds):
        for k in engines:
            ms, iters = step(k)
            res[k]["step_ms"].append(round(ms, 3))
            res[k]["solves_per_frame"] = round(float((iters & 0x3FFFFFFF).to(torch.float64).mean().item()), 3)
            res[k]["qp_iteration_caps"] = int(((iters >> 30) & 1).ne(0).sum().item())
    for k, r in res.items():
        r["frames_per_s"] = S * T / (float(np.median(r["step_ms"])) * 1e-3)
    print(json.dumps({"workload": f"unitree_g1, {S} clips x {T} frames, {D} distinct", "rounds": args.rounds, **res,
                      "inf_cap_over_uncapped_time": float(np.median(res["inf_cap"]["step_ms"]) / np.median(res["uncapped"]["step_ms"])),
                      "capped_over_uncapped_time": float(np.median(res["capped"]["step_ms"]) / np.median(res["uncapped"]["step_ms"]))}))


if __name__ == "__main__":
    main()

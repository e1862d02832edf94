"""Self-collision: the time of one Engine.motion_self_collision call, its two kernels apart, both homes of the pair table, and the
numpy reference on 16 threads beside it.

    python tools/self_collision_bench.py [--clips 2048] [--frames 3000] [--repeats 21] [--warmup 3] [--out profiles/self_collision_bench.json]

Workload: unitree_g1 with the default proxies (the skeleton's capsules of 0.03 m and their default pairs), `clips` clips x `frames`
frames of the random-walk qpos of tools/track_bench.py (the figure is a time, not a result).  Timed between two HIP events on an
otherwise idle stream, caller-owned outputs, cached tables and device-resident offsets (no allocation, no upload inside the window):
the whole call (two kernels), the call without statistics (kernel a alone), kernel b as their difference, and kernel a again with
the pair table in its other home (GMR_AMD_COLLISION_PAIRS), alternating.  Every figure is the median of `repeats` after `warmup`,
with min and max.

The flop count is stated, not measured: per pair 9 subtractions for d1, d2, r; 5 dot products of 5 flops; den 3; s 5 and t 3 with
their divisions counted as one flop each; w 15; the norm 5 and its root 1; the radii 2; compare, min and hit 3: 71 flops, plus per
capsule two rotations and additions (2 x 33) and per body the pose step (about 80).  The share is of the 78.6 TFLOP/s FP64 vector peak
of the MI355X.  The yardstick beside it is the numpy reference of tests/self_collision_reference.py on 16 threads over a sample of
the same rows (`--baseline_rows`), not the code under test.  Informational: nothing gates on it.  Prints one JSON line and writes it
to --out."""
from __future__ import annotations

import argparse
import concurrent.futures
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

FP64_VECTOR_FLOPS = 78.6e12
FLOPS_PER_PAIR, FLOPS_PER_CAPSULE, FLOPS_PER_BODY = 71, 66, 80


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--robot", default="unitree_g1")
    ap.add_argument("--baseline_rows", type=int, default=16 * 512)
    ap.add_argument("--out", default=os.path.join("profiles", "self_collision_bench.json"))
    args = ap.parse_args(argv)
    from gmr_amd import GeneralMotionRetargeting
    g = GeneralMotionRetargeting("smplx", args.robot, device=0)
    eng = g._engine
    dev = eng.device
    caps, pairs = eng.default_proxies()
    offs = np.arange(args.clips + 1, dtype=np.int64) * args.frames
    offs_dev = torch.from_numpy(offs).to(dev)
    qpos = smooth_qpos(eng.nq, args.clips, args.frames, dev)
    N = int(qpos.shape[0])
    res = eng.motion_self_collision(qpos, offs_dev, caps, pairs)
    out = {k: torch.empty_like(v) for k, v in res.items()}
    frame_out = {k: out[k] for k in ("clearance", "pair", "hits")}

    def call(home, stats):
        def fn():
            if home is None:
                os.environ.pop("GMR_AMD_COLLISION_PAIRS", None)
            else:
                os.environ["GMR_AMD_COLLISION_PAIRS"] = home
            eng.motion_self_collision(qpos, offs_dev, caps, pairs, out=out if stats else frame_out)
        return fn

    runs = {"call": call(None, True), "kernel_a": call(None, False), "kernel_a_pairs_lds": call("lds", False), "kernel_a_pairs_global": call("global", False)}
    for _ in range(args.warmup):
        for fn in runs.values():
            fn()
    ms = {k: [] for k in runs}
    for _ in range(args.repeats):  # alternating
        for k, fn in runs.items():
            ms[k].append(_timed(fn))
    os.environ.pop("GMR_AMD_COLLISION_PAIRS", None)
    runs["call"]()
    torch.cuda.synchronize()
    same = all(torch.equal(out[k].view(torch.uint8), res[k].view(torch.uint8)) for k in res)   # bit-reproducible, whichever home
    st = {k: _stats(v) for k, v in ms.items()}
    b_ms = [c - a for c, a in zip(ms["call"], ms["kernel_a"])]
    flops = N * (len(pairs) * FLOPS_PER_PAIR + len(caps) * FLOPS_PER_CAPSULE + eng.nbody * FLOPS_PER_BODY)

    # the yardstick: the numpy reference on 16 threads over a sample of the same rows
    from tests import self_collision_reference as SR
    rows = qpos[:args.baseline_rows].cpu().numpy()
    chunks = np.array_split(rows, 16)
    rob = eng.cm.robot
    work = lambda q: SR.frames(SR.pair_clearance(rob, caps, pairs, q))   # noqa: E731
    work(chunks[0][:8])
    t0 = time.perf_counter()
    with concurrent.futures.ThreadPoolExecutor(16) as pool:
        parts = list(pool.map(work, chunks))
    numpy_s = time.perf_counter() - t0
    ref_cl = np.concatenate([p["clearance"] for p in parts])
    worst = float(np.abs(res["clearance"][:args.baseline_rows].cpu().numpy() - ref_cl).max())

    a_s = st["kernel_a"]["ms_median"] * 1e-3
    line = {"workload": f"{args.robot}, {len(caps)} capsules, {len(pairs)} pairs, {args.clips} clips x {args.frames} frames ({N} frames)",
            "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "warmup": args.warmup,
            "frames": N, "call_device_events": st["call"], "kernel_a_device_events": st["kernel_a"], "kernel_b_by_difference": _stats(b_ms),
            "kernel_a_pairs_in_lds": st["kernel_a_pairs_lds"], "kernel_a_pairs_from_l2": st["kernel_a_pairs_global"],
            "frames_per_s": round(N / (st["call"]["ms_median"] * 1e-3), 1), "pair_tests_per_s": round(N * len(pairs) / a_s, 1),
            "flops_counted": flops, "flops_per_pair": FLOPS_PER_PAIR,
            "fraction_of_fp64_vector_peak": round(flops / a_s / FP64_VECTOR_FLOPS, 4),
            "numpy_16_threads": {"rows": int(rows.shape[0]), "seconds": round(numpy_s, 3), "frames_per_s": round(rows.shape[0] / numpy_s, 1)},
            "speedup_over_numpy_16_threads": round((N / (st["call"]["ms_median"] * 1e-3)) / (rows.shape[0] / numpy_s), 1),
            "worst_abs_difference_to_numpy_on_those_rows": worst,
            "colliding_frames": int(res["colliding_frames"].sum()), "clearance_min": float(res["clearance_min"].min()),
            "nonfinite_frames": int(res["nonfinite_frames"].sum()), "repeated_calls_identical": bool(same)}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

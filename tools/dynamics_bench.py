"""Inverse dynamics: the time of one Engine.motion_dynamics call next to the Engine.motion_track call on the same qpos.

    python tools/dynamics_bench.py [--clips 2048] [--frames 3000] [--repeats 21] [--warmup 5] [--out profiles/dynamics_bench.json]

Workload: that of tools/track_bench.py -- unitree_g1, `clips` clips x `frames` frames of its random-walk qpos at 30 fps, whose second
differences are large (torques far over the limits: the figure is a time, not a result) -- with velocities and accelerations
differenced by the kernel, all per-frame outputs but qvel / qacc, and all per-clip statistics.  The inertial table is
the robot's own MJCF file's (GMR_ROOT, or the copy under tests/golden).  The dynamics call alone and the export (30 fps -> 50 Hz)
alone are timed in the same process, alternating, each between two HIP events on an otherwise idle stream, caller-owned outputs and
device-resident offsets (no allocation, no upload inside the window).  Every figure is the median of `repeats` after `warmup`, with
min and max.  The bytes the call needs are counted from the shapes: qpos read once, tau, root_wrench, com and zmp written, tau and
root_wrench read again by the statistics kernel.  Informational: nothing gates on it.  Prints one JSON line and writes it to --out."""
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

from tools.contact_bench import HBM_BYTES_PER_S, _stats, _timed  # noqa: E402
from tools.track_bench import smooth_qpos  # noqa: E402


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--robot", default="unitree_g1")
    ap.add_argument("--out", default=os.path.join("profiles", "dynamics_bench.json"))
    args = ap.parse_args(argv)
    if args.repeats < 20:
        ap.error("--repeats must be at least 20")
    from gmr_amd import GeneralMotionRetargeting, params
    from gmr_amd.inertial import load_inertial
    g = GeneralMotionRetargeting("smplx", args.robot, device=0)
    eng = g._engine
    dev = eng.device
    table = None if g.model.xml_path else load_inertial(os.path.join(ROOT, "tests", "golden", "gmr_root", "assets", params._ROBOT_XML_REL[args.robot]))
    offs = np.arange(args.clips + 1, dtype=np.int64) * args.frames
    offs_dev = torch.from_numpy(offs).to(dev)
    qpos = smooth_qpos(eng.nq, args.clips, args.frames, dev)
    N, nh = int(qpos.shape[0]), eng.nq - 7
    names = [k for k in eng.motion_dynamics(qpos[:4], [0, 4], 30.0, table=table) if k not in ("qvel", "qacc")]
    first = eng.motion_dynamics(qpos, offs_dev, 30.0, table=table)
    res = {k: first[k] for k in names}
    del first
    out = {k: torch.empty_like(v) for k, v in res.items()}
    track = eng.motion_track(qpos, offs, 30.0, 50.0)
    dyn = lambda: eng.motion_dynamics(qpos, offs_dev, 30.0, table=table, out=out)  # noqa: E731
    export = lambda: eng.motion_track(qpos, offs, 30.0, 50.0, out=dict(track))  # noqa: E731
    for _ in range(args.warmup):
        dyn(), export()
    d_ms, t_ms = [], []
    for _ in range(args.repeats):  # alternating
        d_ms.append(_timed(dyn))
        t_ms.append(_timed(export))
    torch.cuda.synchronize()
    same = all(torch.equal(out[k].view(torch.uint8), res[k].view(torch.uint8)) for k in res)   # bit-reproducible
    bytes_needed = N * 8 * (eng.nq + (nh + 6 + 3 + 2) + (nh + 6))
    Ds, Ts = _stats(d_ms), _stats(t_ms)
    line = {"workload": f"{args.robot}, {args.clips} clips x {args.frames} frames ({N} frames) at 30 fps, differenced velocities and "
                        "accelerations, outputs tau, root_wrench, com, zmp and all statistics",
            "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "warmup": args.warmup,
            "frames": N, "motion_dynamics_device_events": Ds, "motion_track_device_events": Ts,
            "dynamics_over_track": round(Ds["ms_median"] / Ts["ms_median"], 4),
            "dynamics_frames_per_s": round(N / (Ds["ms_median"] * 1e-3), 1),
            "dynamics_algorithmic_bytes": bytes_needed,
            "dynamics_fraction_of_8TBps_hbm": round(bytes_needed / (Ds["ms_median"] * 1e-3) / HBM_BYTES_PER_S, 5),
            "tau_abs_max": float(res["tau_abs_max"].max()), "fz_ratio_max": float(res["fz_ratio_max"].max()),
            "frames_any_over_limit": int(res["frames_any_over_limit"].sum()), "unloaded_frames": int(res["unloaded_frames"].sum()),
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

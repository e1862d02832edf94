#!/usr/bin/env python3
"""Record the bits of the G1 / smplx solve for tests/golden/ik_g1_smplx_parent_bits.npz (tests/test_gpu_ik_target_blocks.py).

    python tools/record_ik_bits.py --commit <id of the commit whose library is loaded> [--out FILE]

Run it with the library of the commit the bits are to be pinned to (GMR_AMD_LIB may point at it): 3 easy + 3 hard synthetic clips of
40 frames (the generator and seeds of tests/test_gpu_ik_shapes.py), one whole-clip launch on the shaped instance, qpos and the solve
words as they come back.  The commit id is stored in the file; nothing else identifies the build.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gmr_amd import synth  # noqa: E402
from gmr_amd.engine import Engine  # noqa: E402
from gmr_amd.schedule import make_items  # noqa: E402
from tests.util import compiled  # noqa: E402

N_EACH, T, SEED_EASY, SEED_HARD = 3, 40, 21, 22


def clips(cm):
    pe, qe, names, _, _ = synth.synth_clips(cm, N_EACH, T, seed=SEED_EASY, hard=False, dtype=np.float32)
    ph, qh, names_h, _, _ = synth.synth_clips(cm, N_EACH, T, seed=SEED_HARD, hard=True, dtype=np.float32)
    assert names == names_h
    return np.concatenate([pe, ph]), np.concatenate([qe, qh]), cm.slot_columns(names), np.arange(2 * N_EACH + 1, dtype=np.int64) * T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="id of the commit the loaded library was built from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ik_g1_smplx_parent_bits.npz"))
    args = ap.parse_args()
    os.environ["GMR_AMD_BALANCE"] = "0"  # the whole-clip launch
    os.environ["GMR_AMD_GENERIC_SHAPE"] = "0"
    cm = compiled("smplx", "unitree_g1")
    pos, quat, sc, offs = clips(cm)
    dev = torch.device("cuda", 0)
    eng = Engine(cm, 0)
    q, it, _ = eng.ik_solve(torch.from_numpy(pos).to(dev), torch.from_numpy(quat).to(dev), sc, make_items(offs), launch_order=None)
    torch.cuda.synchronize()
    q, it = q.cpu().numpy(), it.cpu().numpy()
    eng.close()
    assert np.isfinite(q).all() and int((it & 0x3fffffff).max()) > 2
    np.savez_compressed(args.out, qpos=q, iters=it, commit=np.array(args.commit), n_each=N_EACH, frames=T, seeds=np.array([SEED_EASY, SEED_HARD]))
    print(f"{args.out}: qpos {q.shape} {q.dtype}, iters {it.shape} {it.dtype}, {os.path.getsize(args.out)} bytes, commit {args.commit}")


if __name__ == "__main__":
    main()

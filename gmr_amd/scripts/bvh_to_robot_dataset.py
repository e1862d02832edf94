"""scripts/bvh_to_robot_dataset.py on this engine: a folder of BVH files -> one pickle per clip, same flags, same file layout.

The reference converts file by file, frame by frame (:59-151).  Here the files of a batch are read ahead and parsed on the GPU, solved in one
launch (verified parallel-in-time chunks, one height estimate per file), post-processed and written by a thread pool while the next batch
is on the GPU.  Files that cannot be loaded are reported and skipped like the reference's ``except: print; continue`` (:75-80).
"""
from __future__ import annotations

import argparse

from ._walk import add_common_flags, convert, plan, resolve_robots, resolve_track


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--src_folder", required=True, type=str, help="Folder containing BVH motion files to load.")
    ap.add_argument("--tgt_folder", default="../../motion_data/LAFAN1_g1_gmr", help="Folder to save the retargeted motion files.")
    ap.add_argument("--robot", default=None, help="(default: unitree_g1)")
    ap.add_argument("--target_fps", default=30, type=int, help="(accepted like the reference, which stores 30 whatever it is given)")
    ap.add_argument("--batch_files", default=64, type=int, help="files per GPU batch (one skeleton per batch)")
    ap.add_argument("--threads", default=8, type=int, help="host threads reading files / writing pickles")
    add_common_flags(ap)
    args = ap.parse_args(argv)
    resolve_robots(ap, args)
    resolve_track(ap, args)
    srcs, tgts, skipped = plan(args, ".bvh", lambda n: n.endswith(".bvh"))
    print(f"{len(srcs)} files to retarget ({skipped} skipped: target exists)")

    def batches(todo, columns):
        from ..bvh import iter_lafan1_batches
        while todo:  # a batch holds one skeleton (its first readable file's); files of another one wait for the next pass
            again = []
            for batch in iter_lafan1_batches(todo, batch_files=args.batch_files, device=args.device, threads=args.threads, columns=columns, skip_errors=True):
                again += [f for f, why in batch.skipped if "skeleton differs" in why]
                batch.skipped = [(f, why) for f, why in batch.skipped if "skeleton differs" not in why]
                yield batch
            todo = again if len(again) < len(todo) else []
    return convert(args, list(zip(srcs, tgts)), "bvh", batches, lambda batch: dict(fps=30, height_adjust=False, root_origin_offset=False, chunk="auto"),  # :127-128
                   args.threads, "Done. saved to ")


if __name__ == "__main__":
    raise SystemExit(main())

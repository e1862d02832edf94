"""scripts/smplx_to_robot_dataset.py behind the body model: a folder of joint-array files -> one pickle per clip, same flags, same file layout.

The reference loads each AMASS file, runs the licensed SMPL-X body model, aligns the frame rate, retargets frame by frame and writes a pickle, in
``--num_cpus`` processes (:63-146, 241-242).  The body model stays on the reference side: its outputs are dumped once per clip with
``gmr_amd.smplx_adapter.save_joint_file``; this script does everything behind it on the GPU, batch by batch, with the same
folder walk, the same exclusions (``_stagei`` files, the hard-motion lists, the BMLrub / EKUT / crawl / _lie / stairs names, :193-227) and the
same targets.
"""
from __future__ import annotations

import argparse
import os

from ._walk import add_common_flags, convert, hard_motion_names, plan, resolve_robots, resolve_track

EXCLUDE_FILE_CONTENT = ["BMLrub", "EKUT", "crawl", "_lie", "upstairs", "downstairs"]  # smplx_to_robot_dataset.py:218


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--robot", default=None, help="(default: unitree_g1)")
    ap.add_argument("--src_folder", type=str, required=True, help="folder of joint-array .npz files (smplx_adapter.save_joint_file)")
    ap.add_argument("--tgt_folder", type=str, required=True)
    ap.add_argument("--num_cpus", default=4, type=int, help="host threads reading files / writing pickles (the reference's worker processes)")
    ap.add_argument("--hard_motions", nargs="*", default=None, help="lists of motions to leave out (default: $GMR_ROOT/assets/hard_motions/0.txt, 1.txt when present)")
    ap.add_argument("--batch_files", default=1024, type=int)
    ap.add_argument("--smplx_model_folder", default=None, type=str,
                    help="folder holding smplx/SMPLX_<GENDER>.npz|pkl: --src_folder then holds AMASS .npz files and the body model's joints are evaluated here")
    ap.add_argument("--num_betas", default=None, type=int, help="with --smplx_model_folder: shape coefficients used per clip (default: all the file and the model share)")
    add_common_flags(ap)
    args = ap.parse_args(argv)
    resolve_robots(ap, args)
    resolve_track(ap, args)
    srcs, tgts, skipped = plan(args, ".npz", lambda n: n.endswith(".npz") and not n.endswith("_stagei.npz"), natural=True)
    print("full args_list:", len(srcs))
    lists = args.hard_motions
    if lists is None:
        root = os.environ.get("GMR_ROOT", "")
        lists = [os.path.join(root, "assets", "hard_motions", n) for n in ("0.txt", "1.txt")] if root else []
    hard = set(hard_motion_names(lists))
    keep = []
    for s, t in zip(srcs, tgts):
        name = s.split("/")[-1].split(".")[0]
        if name in hard or any(c in name for c in EXCLUDE_FILE_CONTENT):
            continue
        keep.append((s, t))
    print("new args_list:", len(keep))
    print(f"Total number of files to process: {len(keep)}")

    def batches(files, columns):
        from ..smplx_adapter import iter_amass_batches, iter_joint_batches
        if args.smplx_model_folder is not None:
            return iter_amass_batches(files, args.smplx_model_folder, batch_files=args.batch_files, device=args.device, threads=max(1, args.num_cpus),
                                      columns=columns, skip_errors=True, num_betas=args.num_betas)
        return iter_joint_batches(files, batch_files=args.batch_files, device=args.device, threads=max(1, args.num_cpus), columns=columns, skip_errors=True)
    return convert(args, keep, "smplx", batches, lambda batch: dict(fps=batch.fps), args.num_cpus, "Done. Saved to ")  # :97-141


if __name__ == "__main__":
    raise SystemExit(main())

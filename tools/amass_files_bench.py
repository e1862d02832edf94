"""AMASS files straight to pickles against the joint-file path: the same synthetic clips as AMASS .npz files (body model evaluated
here, gmr_amd.smplx_body) and as joint-array files (the body model's outputs dumped beforehand) -> key-points -> qpos -> pickles.

    python tools/amass_files_bench.py [n_files] [frames_per_file] [threads] [batch_files] [reps]

Synthetic folder on tmpfs (page cache warm: the files were just written): random AMASS parameters at 30 fps on a random stand-in
model (synth.write_smplx_model), float64 as AMASS stores them; the joint files hold the body kernel's own outputs for the same
clips, float32 as a body model emits them (what tools/smplx_files_bench.py reads).  Also times the body kernel alone on a chip-filling
batch.  One JSON line; medians of `reps` timed passes after one warm-up pass.
"""
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def run(n_files=512, T=750, threads=16, batch_files=256, reps=5, device=0):
    from gmr_amd import GeneralMotionRetargeting as GMR, dataset, smplx_body, synth
    from gmr_amd import smplx_adapter as sa
    dev = torch.device("cuda", device)
    tmpd = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    res = {"files": n_files, "frames": n_files * T, "threads": threads, "batch_files": batch_files, "reps": reps, "page_cache": "warm (tmpfs)"}
    try:
        g = GMR(src_human="smplx", tgt_robot="unitree_g1")
        cols = g.ik_columns
        folder = synth.write_smplx_model_folder(os.path.join(tmpd, "models"), seed=1)
        models = smplx_body.BodyModelSet(folder)
        d_am, d_jf, d_out = (os.path.join(tmpd, n) for n in ("amass", "joint", "out"))
        files, arrays = synth.write_amass_files(d_am, [T] * n_files, seed=7, fps=30.0, genders=("neutral", "male", "female"))
        os.makedirs(d_jf)
        jfiles = []
        for k, a in enumerate(arrays):
            m = models.get(a["gender"])
            clip = dict(model=m, betas=m.clip_betas(a["betas"]), **{key: torch.as_tensor(a[key]).to(dev) for key in ("root_orient", "pose_body", "trans")})
            go, fp, jt, _ = smplx_body.evaluate_clips([clip])
            jf = os.path.join(d_jf, f"clip_{k:05d}.npz")
            sa.save_joint_file(jf, jt.float().cpu().numpy(), go.float().cpu().numpy(), fp.reshape(T, -1).float().cpu().numpy(), 30.0, a["betas"])
            jfiles.append(jf)
        res["amass_input_MB"] = sum(os.path.getsize(f) for f in files) / 1e6
        res["joint_input_MB"] = sum(os.path.getsize(f) for f in jfiles) / 1e6
        N = n_files * T
        paths = {"amass": lambda: sa.iter_amass_batches(files, models, batch_files=batch_files, threads=threads, columns=cols),
                 "joint": lambda: sa.iter_joint_batches(jfiles, batch_files=batch_files, threads=threads, columns=cols)}

        def timed(fn):
            ts = []
            for i in range(reps + 1):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if i:
                    ts.append(time.perf_counter() - t0)
            return float(np.median(ts))

        def to_qpos(it):
            for b in it():
                g.retarget_batch(b.pos, b.quat, b.body_names, seq_offsets=b.seq_offsets, human_heights=b.human_heights)

        def to_pickles(it):
            with dataset.MotionWriter(workers=max(2, min(16, threads)), override=True) as w:
                for b in it():
                    motions = dataset.retarget_clips(g, b.pos, b.quat, b.body_names, b.seq_offsets, fps=b.fps, human_heights=b.human_heights)
                    w.submit(motions, [os.path.join(d_out, os.path.basename(f)[:-4] + ".pkl") for f in b.files])
        for name, it in paths.items():  # the two paths alternate stage by stage inside one process
            res[f"{name}_files_to_keypoints_frames_per_s"] = N / timed(lambda: [len(b) for b in it()])
        for name, it in paths.items():
            res[f"{name}_files_to_qpos_frames_per_s"] = N / timed(lambda: to_qpos(it))
        for name, it in paths.items():
            res[f"{name}_files_to_pickles_frames_per_s"] = N / timed(lambda: to_pickles(it))

        # the body kernel alone: 4 M frames in 4096 clips, float64 inputs, all 55 joints and the IK columns
        nk, tk = 4096, 1024
        m = models.get("neutral")
        big = synth.amass_arrays(tk, 3)
        base = {key: torch.as_tensor(big[key]).to(dev) for key in ("root_orient", "pose_body", "trans")}
        clips = [dict(model=m, betas=big["betas"], **{key: base[key].clone() for key in base}) for _ in range(nk)]
        for label, c, live in (("all", None, 55), ("ik_columns", cols, None)):
            smplx_body.evaluate_clips(clips, columns=c)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ts = []
            for _ in range(reps):
                torch.cuda.synchronize(); ev[0].record()
                smplx_body.evaluate_clips(clips, columns=c)
                ev[1].record(); torch.cuda.synchronize()
                ts.append(ev[0].elapsed_time(ev[1]))
            ms = float(np.median(ts))
            if live is None:
                names = list(sa.SMPLX_JOINT_NAMES)
                s = set()
                for n in c:
                    j = names.index(n)
                    while j >= 0:
                        s.add(j); j = sa.SMPLX_PARENTS[j]
                live = len(s)
            posed = min(live, 22)
            byts = (3 + 3 * posed + 3) * 8 + (3 + 2 * 3 * live) * 8  # in: trans, root + body rotations of live joints; out: global_orient, full_pose + joints rows
            res[f"body_kernel_{label}"] = {"frames": nk * tk, "ms_incl_launch_and_table": ms, "live_joints": live, "algorithmic_bytes_per_frame": byts,
                                           "fraction_of_8TBps": nk * tk * byts / (ms * 1e-3) / 8e12}
    finally:
        shutil.rmtree(tmpd, ignore_errors=True)
    return res


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:6]]
    a = a + [512, 750, 16, 256, 5][len(a):]
    print(json.dumps(run(a[0], a[1], a[2], batch_files=a[3], reps=a[4])))

"""SMPL-X key-point adapter on the fast path.

``get_smplx_data_offline_fast`` of the reference (general_motion_retargeting/utils/smpl.py:109-198) minus the Python:
the SMPL-X body model itself (licensed assets, smpl.py:12-34) stays with the caller and hands over
``global_orient [T,3]``, ``full_pose [T,J*3]`` (axis-angle), ``joints [T,>=J,3]`` and ``parents [J]``; this module
aligns them to the target frame rate (slerp per joint, lerp per coordinate) and chains the orientations down the
kinematic tree on the GPU (``gmr_smplx_keypoints``), returning the ``[T', J, 3]`` / ``[T', J, 4]`` tensors
``retarget_batch`` consumes, with the SMPL-X joint names as columns.

The reference module cannot be imported here (it needs the ``smplx`` package), so this row is "parity unpinned";
tests pin it against a scipy restatement of the cited lines.
"""
from __future__ import annotations

import ast
import ctypes as C
import os
import struct
import zlib
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native
from ._filebatch import ClipBatch, Staged, pinned, read_ahead, read_files, read_planned

# smplx.joint_names.JOINT_NAMES[:55] (body, jaw, eyes, hands) -- the names the smplx_to_*.json configs refer to
SMPLX_JOINT_NAMES: List[str] = [
    "pelvis", "left_hip", "right_hip", "spine1", "left_knee", "right_knee", "spine2", "left_ankle", "right_ankle", "spine3",
    "left_foot", "right_foot", "neck", "left_collar", "right_collar", "head", "left_shoulder", "right_shoulder", "left_elbow",
    "right_elbow", "left_wrist", "right_wrist", "jaw", "left_eye_smplhf", "right_eye_smplhf",
    "left_index1", "left_index2", "left_index3", "left_middle1", "left_middle2", "left_middle3", "left_pinky1", "left_pinky2",
    "left_pinky3", "left_ring1", "left_ring2", "left_ring3", "left_thumb1", "left_thumb2", "left_thumb3",
    "right_index1", "right_index2", "right_index3", "right_middle1", "right_middle2", "right_middle3", "right_pinky1", "right_pinky2",
    "right_pinky3", "right_ring1", "right_ring2", "right_ring3", "right_thumb1", "right_thumb2", "right_thumb3",
]
# kinematic tree of the SMPL-X model (body_model.parents)
SMPLX_PARENTS: List[int] = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 15, 15, 15,
                            20, 25, 26, 20, 28, 29, 20, 31, 32, 20, 34, 35, 20, 37, 38,
                            21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50, 21, 52, 53]


def get_smplx_data_offline_fast(global_orient, full_pose, joints, parents: Sequence[int] = SMPLX_PARENTS, src_fps: float = 30.0,
                                tgt_fps: float = 30.0, joint_names: Sequence[str] = SMPLX_JOINT_NAMES,
                                device: int = 0, columns: Optional[Sequence[str]] = None, out=None) -> Tuple[torch.Tensor, torch.Tensor, List[str], float]:
    """-> (pos [T',J,3], quat [T',J,4] wxyz, joint names, aligned_fps); float64 CUDA tensors.
    ``columns``: emit only these joints, in this order (e.g. ``ik_columns(config)``: the 14 an smplx_to_*.json config reads) --
    their ancestors are chained inside the kernel, the rest of the 55 is neither read nor written.
    ``out``: (pos, quat) contiguous float64 tensors of exactly the result's shapes to write into (rows of a batch)."""
    lib = _native.load()
    dev = torch.device("cuda", device)
    # float32 arrays (a body model's output) go to the kernel as they are; anything else is made float64
    f32 = all((a.dtype == torch.float32) if isinstance(a, torch.Tensor) else (np.asarray(a).dtype == np.float32) for a in (global_orient, full_pose, joints))
    dt = torch.float32 if f32 else torch.float64
    as_t = lambda a: (a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))).detach().to(dev, dt)
    parents = np.ascontiguousarray(parents, dtype=np.int32)
    J = len(parents)
    go = as_t(global_orient).reshape(-1, 3).contiguous()
    T = int(go.shape[0])
    fp = as_t(full_pose).reshape(T, -1, 3)
    if fp.shape[1] < J:
        raise ValueError("full_pose has fewer joints than parents")
    fp = fp[:, :J].contiguous()
    jt = as_t(joints).reshape(T, -1, 3).contiguous()
    if jt.shape[1] < J or len(joint_names) < J:
        raise ValueError("joints / joint_names shorter than parents")
    frame_skip = int(src_fps / tgt_fps)  # smpl.py:119
    if tgt_fps < src_fps:
        T_out = T // frame_skip          # :127
        resample = 1
        aligned_fps = T_out / T * src_fps if T else tgt_fps  # :172
    else:
        T_out, resample, aligned_fps = T, 0, tgt_fps
    names = list(joint_names[:J])
    cols = None
    if columns is not None:
        sel = [str(c) for c in columns]
        missing = [c for c in sel if c not in names]
        if missing:
            raise KeyError(missing[0])
        cols = np.asarray([names.index(c) for c in sel], dtype=np.int32)
        names = sel
    B = len(names)
    if out is None:
        pos = torch.empty((T_out, B, 3), dtype=torch.float64, device=dev)
        quat = torch.empty((T_out, B, 4), dtype=torch.float64, device=dev)
    else:
        pos, quat = out
        for t, k in ((pos, 3), (quat, 4)):
            if tuple(t.shape) != (T_out, B, k) or t.dtype != torch.float64 or t.device != dev or not t.is_contiguous():
                raise ValueError(f"out tensors must be contiguous float64 [{T_out}, {B}, 3 / 4] on {dev}")
    vp = C.c_void_p
    if T_out > 0:
        with torch.cuda.device(dev):
            rc = lib.gmr_smplx_keypoints_in(parents.ctypes.data_as(vp), J, int(jt.shape[1]), vp(go.data_ptr()), vp(fp.data_ptr()), vp(jt.data_ptr()),
                                            _native.GMR_DTYPE_F32 if f32 else _native.GMR_DTYPE_F64, T, T_out, resample,
                                            cols.ctypes.data_as(vp) if cols is not None else None, B,
                                            vp(pos.data_ptr()), vp(quat.data_ptr()), vp(torch.cuda.current_stream(dev).cuda_stream))
        if rc != 0:
            raise RuntimeError(f"gmr_smplx_keypoints_in failed with status {rc}")
    return pos, quat, names, float(aligned_fps)


# ---------------------------------------------------------------------------------------------------------------- joint-array files
# The file side of this row.  scripts/smplx_to_robot_dataset.py:63-87 goes AMASS .npz -> smplx body model (licensed assets, stays with
# the caller) -> get_smplx_data_offline_fast -> retarget, per file.  A caller that owns the body model dumps its outputs ONCE
# (`save_joint_file`) and the whole rest of the script -- frame-rate alignment, orientation chaining, IK, FK,
# post-processing, pickles -- runs here over folders of such files, batched like the BVH folder path (gmr_amd.bvh.iter_lafan1_batches).
JOINT_FILE_KEYS = ("joints", "global_orient", "full_pose", "mocap_frame_rate", "betas")


def human_height_from_betas(betas) -> float:
    """load_smplx_file's height estimate (utils/smpl.py:37-40): 1.66 + 0.1 * betas[0] (betas [16] or [1, 16])."""
    b = np.asarray(betas, dtype=np.float64)
    return float(1.66 + 0.1 * (b[0] if b.ndim == 1 else b[0, 0]))


def save_joint_file(path, joints, global_orient, full_pose, mocap_frame_rate, betas, n_joints: int = len(SMPLX_PARENTS)) -> None:
    """One clip's body-model outputs as an uncompressed .npz: ``joints [T, >= n_joints, 3]`` (only the first ``n_joints`` are kept: the
    model emits 127, the adapter reads 55), ``global_orient [T, 3]``, ``full_pose [T, >= 3 n_joints]`` (axis-angle), the AMASS file's
    ``mocap_frame_rate`` and ``betas``.  Arrays keep their dtype (the model's float32 halves the file)."""
    j = np.asarray(joints)
    T = j.shape[0]
    fp = np.asarray(full_pose).reshape(T, -1)
    np.savez(path, joints=np.ascontiguousarray(j.reshape(T, -1, 3)[:, :n_joints]), global_orient=np.asarray(global_orient).reshape(T, 3),
             full_pose=np.ascontiguousarray(fp[:, :3 * n_joints]), mocap_frame_rate=np.asarray(mocap_frame_rate), betas=np.asarray(betas))


class SmplxBatch(ClipBatch):
    """A ``ClipBatch`` of SMPL-X clips at the target frame rate, heights from their betas; ``fps``: each clip's aligned frame rate
    (what the reference stores in the pickle) -- the arguments of ``retarget_batch`` / ``dataset.retarget_clips``."""

    def __init__(self, pos, quat, names, seq_offsets, heights, fps, files, skipped=None):
        super().__init__(pos, quat, names, seq_offsets, heights, files, skipped)
        self.fps = fps


def _zip_directory(view: memoryview, path: str):
    """{name: (dtype, shape, byte offset of the data in `view`)} of an UNCOMPRESSED .npz (np.savez): the end-of-central-directory
    record, the central directory and the .npy headers are parsed in place; the arrays themselves are not touched.  (np.load walks every
    byte through zipfile's CRC loop under the GIL: 0.3 GB/s, slower with threads; a plain read of the same file runs at 5 GB/s.)"""
    n = len(view)
    tail = bytes(view[max(0, n - 65557):])
    k = tail.rfind(b"PK\x05\x06")
    if k < 0:
        raise ValueError(f"{path}: not a zip archive")
    total, cd_size, cd_off = struct.unpack_from("<HII", tail, k + 10)
    if cd_off == 0xFFFFFFFF or total == 0xFFFF:
        raise ValueError(f"{path}: zip64 directory")
    out, p = {}, cd_off
    for _ in range(total):
        sig, method, csize, usize, nlen, xlen, clen, lho = struct.unpack_from("<4s6xH8xIIHHH8xI", view, p)
        if sig != b"PK\x01\x02":
            raise ValueError(f"{path}: bad central directory")
        name = bytes(view[p + 46:p + 46 + nlen]).decode()
        p += 46 + nlen + xlen + clen
        if method != 0:
            raise ValueError(f"{path}: member {name} is compressed (write joint files with np.savez / save_joint_file)")
        if usize == 0xFFFFFFFF or lho == 0xFFFFFFFF:
            raise ValueError(f"{path}: zip64 member")
        sig2, nlen2, xlen2 = struct.unpack_from("<4s22xHH", view, lho)
        if sig2 != b"PK\x03\x04":
            raise ValueError(f"{path}: bad local header")
        d0 = lho + 30 + nlen2 + xlen2
        head = bytes(view[d0:d0 + min(usize, 4096)])
        if head[:6] != b"\x93NUMPY":
            raise ValueError(f"{path}: member {name} is not a .npy array")
        major = head[6]
        hlen, hoff = (struct.unpack_from("<H", head, 8)[0], 10) if major == 1 else (struct.unpack_from("<I", head, 8)[0], 12)
        try:
            d = ast.literal_eval(head[hoff:hoff + hlen].decode("latin1"))
            dt, shape, plain = np.dtype(d["descr"]), tuple(int(x) for x in d["shape"]), not d["fortran_order"]
        except (SyntaxError, ValueError, TypeError, KeyError) as ex:  # (a header that is not np.save's dict of descr / shape / order)
            raise ValueError(f"{path}: member {name} has a malformed .npy header ({ex})") from None
        if not plain or dt.hasobject:
            raise ValueError(f"{path}: member {name} is not a plain C-ordered array")
        out[name[:-4] if name.endswith(".npy") else name] = (dt, shape, d0 + hoff + hlen)
    return out


def _joint_meta(view, path: str, n_joints: int) -> dict:
    """``parse_one`` of the joint files: where a file's arrays lie (offsets in the file), its frame count, frame rate and height.
    A malformed archive is a ValueError like any other file this loader does not understand."""
    view = memoryview(view)
    n = len(view)
    try:
        mem = _zip_directory(view, path)
    except (struct.error, IndexError, UnicodeDecodeError) as ex:  # (offsets or names in the directory that do not fit the file)
        raise ValueError(f"{path}: malformed zip archive ({ex})") from None
    missing = [key for key in JOINT_FILE_KEYS if key not in mem]
    if missing:
        raise ValueError(f"{path}: no '{missing[0]}' array (a joint file holds {', '.join(JOINT_FILE_KEYS)})")
    (jd, js, jo), (gd, gs, go_), (fd, fs, fo) = mem["joints"], mem["global_orient"], mem["full_pose"]
    T = js[0] if len(js) == 3 else -1
    if len(js) != 3 or js[1] < n_joints or js[2] != 3 or gs != (T, 3) or len(fs) != 2 or fs[0] != T or fs[1] < 3 * n_joints:
        raise ValueError(f"{path}: array shapes do not describe {n_joints} joints over {T} frames")
    for dt in (jd, gd, fd):
        if dt not in (np.dtype("<f4"), np.dtype("<f8")):
            raise ValueError(f"{path}: arrays must be float32 or float64")
    small = {}
    for key in ("mocap_frame_rate", "betas"):
        dt, shp, off = mem[key]
        cnt = int(np.prod(shp)) if shp else 1
        small[key] = np.frombuffer(view, dtype=dt, count=cnt, offset=off).reshape(shp).copy()
    fps = float(np.asarray(small["mocap_frame_rate"]).reshape(-1)[0])
    if not (fps > 0):
        raise ValueError(f"{path}: mocap_frame_rate must be positive")
    for (dt, shp, off) in (mem["joints"], mem["global_orient"], mem["full_pose"]):
        if off + int(np.prod(shp)) * dt.itemsize > n:
            raise ValueError(f"{path}: truncated")
    return {"T": T, "fps": fps, "height": human_height_from_betas(small["betas"]), "arrays": {key: mem[key] for key in ("joints", "global_orient", "full_pose")}}


def _stage(files, dev: torch.device, threads: int, n_joints: int, skip_errors: bool, slot: int) -> Staged:
    """The files in the joint-file loader's pinned ``slot``, each on a 256-byte boundary, with where their arrays lie."""
    with torch.cuda.device(dev):
        return read_files(files, pinned("smplx", slot), 256, lambda view, path: _joint_meta(view, path, n_joints), threads, skip_errors)


def _joint_batch(st: Staged, dev, tgt_fps, columns, parents, joint_names) -> SmplxBatch:
    if not st.files:
        return SmplxBatch.empty(dev, st.skipped)
    J = len(parents)
    names = list(joint_names[:J]) if columns is None else [str(c) for c in columns]
    t_out = [m["T"] // int(m["fps"] / tgt_fps) if tgt_fps < m["fps"] else m["T"] for m in st.parsed]  # smpl.py:119,127
    offs = np.concatenate([[0], np.cumsum(t_out)]).astype(np.int64)
    B = len(names)
    with torch.cuda.device(dev):
        pos = torch.empty((int(offs[-1]), B, 3), dtype=torch.float64, device=dev)
        quat = torch.empty((int(offs[-1]), B, 4), dtype=torch.float64, device=dev)
        raw = st.buf[: st.total].to(dev, non_blocking=True)  # ONE copy of the files as they are; the kernel reads float32 or float64

        def arr(meta, base):
            dt, shp, off = meta
            off += base
            nbytes = int(np.prod(shp)) * dt.itemsize
            t = raw[off:off + nbytes]
            if off % dt.itemsize:
                t = t.clone()  # (np.savez happens to align its members; a foreign writer may not)
            return t.view(torch.float32 if dt.itemsize == 4 else torch.float64).reshape(shp)
        out_fps = []
        for k, m in enumerate(st.parsed):
            a, base = m["arrays"], int(st.starts[k])
            _, _, _, afps = get_smplx_data_offline_fast(arr(a["global_orient"], base), arr(a["full_pose"], base), arr(a["joints"], base), parents, src_fps=m["fps"],
                                                        tgt_fps=tgt_fps, joint_names=joint_names, device=dev.index or 0, columns=columns,
                                                        out=(pos[offs[k]:offs[k + 1]], quat[offs[k]:offs[k + 1]]))
            out_fps.append(afps)
        torch.cuda.current_stream(dev).synchronize()  # the pinned buffer is reused by the batch after next
    return SmplxBatch(pos, quat, names, offs, [m["height"] for m in st.parsed], out_fps, list(st.files), list(st.skipped))


def load_joint_files(files, device: int = 0, tgt_fps: float = 30.0, columns: Optional[Sequence[str]] = None, threads: int = 8, skip_errors: bool = False,
                     parents: Sequence[int] = SMPLX_PARENTS, joint_names: Sequence[str] = SMPLX_JOINT_NAMES) -> SmplxBatch:
    """A folder's worth of joint-array files (``save_joint_file``) -> one ``SmplxBatch`` on the GPU: files read on ``threads`` host
    threads, every clip aligned to ``tgt_fps`` and chained by the adapter kernel straight into its rows of the batch tensors."""
    dev = torch.device("cuda", device)
    return _joint_batch(_stage([str(f) for f in files], dev, threads, len(parents), skip_errors, 0), dev, tgt_fps, columns, parents, joint_names)


def iter_joint_batches(files, batch_files: int = 256, device: int = 0, tgt_fps: float = 30.0, columns: Optional[Sequence[str]] = None, threads: int = 8,
                       skip_errors: bool = False, parents: Sequence[int] = SMPLX_PARENTS, joint_names: Sequence[str] = SMPLX_JOINT_NAMES):
    """The folder in batches of ``batch_files`` files, read ahead: while the caller solves and writes batch k, a background thread reads
    batch k + 1's files.  A batch without a good file is yielded empty (``len(batch) == 0``) with its ``skipped`` list."""
    files = [str(f) for f in files]
    dev = torch.device("cuda", device)
    groups = [files[i:i + batch_files] for i in range(0, len(files), max(1, batch_files))]
    yield from read_ahead(groups, lambda group, slot: _stage(group, dev, threads, len(parents), skip_errors, slot),
                          lambda st: _joint_batch(st, dev, tgt_fps, columns, parents, joint_names))


# --------------------------------------------------------------------------------------------------------------------- AMASS files
# The whole of scripts/smplx_to_robot_dataset.py:63-146 from the user's own folder: AMASS / OMOMO .npz files plus the SMPL-X model
# files.  The body model's joints come from gmr_amd.smplx_body (one launch per batch), the rest is the joint-file path above.
# Of a file only root_orient, pose_body, trans (69 numbers per frame) and the small betas / gender / mocap_frame_rate are read --
# an AMASS archive also carries poses, pose_hand, dmpls, markers ... (several times as much), which stay on the disk.
AMASS_ARRAYS = (("root_orient", 3), ("pose_body", 63), ("trans", 3))
AMASS_SMALL = ("betas", "gender", "mocap_frame_rate")
_MEMBER_ALIGN = 64


def _npy_header(head: bytes, path: str, name: str):
    """(dtype, shape, header length) of a .npy member from its first bytes."""
    if head[:6] != b"\x93NUMPY" or len(head) < 12:
        raise ValueError(f"{path}: member {name} is not a .npy array")
    hlen, hoff = (struct.unpack_from("<H", head, 8)[0], 10) if head[6] == 1 else (struct.unpack_from("<I", head, 8)[0], 12)
    if hoff + hlen > len(head):
        raise ValueError(f"{path}: member {name} has a malformed .npy header")
    try:
        d = ast.literal_eval(head[hoff:hoff + hlen].decode("latin1"))
        dt, shape, plain = np.dtype(d["descr"]), tuple(int(x) for x in d["shape"]), not d["fortran_order"]
    except (SyntaxError, ValueError, TypeError, KeyError) as ex:
        raise ValueError(f"{path}: member {name} has a malformed .npy header ({ex})") from None
    if dt.hasobject or not (plain or len(shape) < 2):
        raise ValueError(f"{path}: member {name} is not a plain C-ordered array")
    return dt, shape, hoff + hlen


def _pread(fh, n: int, at: int, path: str) -> bytes:
    b = os.pread(fh.fileno(), n, at) if n > 0 else b""
    if len(b) != n:
        raise ValueError(f"{path}: truncated")
    return b


def _amass_plan(path: str):
    """``plan_one`` of the AMASS loader: the archive's directory, the small members' values and where the three per-frame arrays lie --
    ``(meta, bytes needed)``.  Only the members named above are looked at: an object array or a member of another kind elsewhere in the
    archive does not matter.  Members may be stored (np.savez) or deflated (np.savez_compressed)."""
    size = os.path.getsize(path)
    with open(path, "rb", buffering=0) as fh:
        try:
            tail_at = max(0, size - 65557)
            tail = _pread(fh, size - tail_at, tail_at, path)
            k = tail.rfind(b"PK\x05\x06")
            if k < 0 or k + 22 > len(tail):
                raise ValueError(f"{path}: not a zip archive")
            total, cd_size, cd_off = struct.unpack_from("<HII", tail, k + 10)
            if cd_off == 0xFFFFFFFF or total == 0xFFFF:
                raise ValueError(f"{path}: zip64 directory")
            if cd_off + cd_size > size:
                raise ValueError(f"{path}: truncated")
            cd = _pread(fh, cd_size, cd_off, path)
            want = {a for a, _ in AMASS_ARRAYS} | set(AMASS_SMALL)
            mem, p = {}, 0
            for _ in range(total):
                sig, method, csize, usize, nlen, xlen, clen, lho = struct.unpack_from("<4s6xH8xIIHHH8xI", cd, p)
                if sig != b"PK\x01\x02":
                    raise ValueError(f"{path}: bad central directory")
                name = cd[p + 46:p + 46 + nlen].decode("utf-8", "replace")
                p += 46 + nlen + xlen + clen
                key = name[:-4] if name.endswith(".npy") else name
                if key not in want:
                    continue
                if method not in (0, 8):
                    raise ValueError(f"{path}: member {name} uses compression method {method}")
                if usize == 0xFFFFFFFF or csize == 0xFFFFFFFF or lho == 0xFFFFFFFF:
                    raise ValueError(f"{path}: zip64 member")
                sig2, nlen2, xlen2 = struct.unpack_from("<4s22xHH", _pread(fh, 30, lho, path), 0)
                if sig2 != b"PK\x03\x04":
                    raise ValueError(f"{path}: bad local header")
                d0 = lho + 30 + nlen2 + xlen2
                if d0 + csize > size:
                    raise ValueError(f"{path}: truncated")
                mem[key] = (method, d0, csize, usize)
        except (struct.error, IndexError) as ex:
            raise ValueError(f"{path}: malformed zip archive ({ex})") from None
        for key in [a for a, _ in AMASS_ARRAYS] + list(AMASS_SMALL):
            if key not in mem:
                raise ValueError(f"{path}: no '{key}' array (an AMASS file holds {', '.join(a for a, _ in AMASS_ARRAYS)}, {', '.join(AMASS_SMALL)})")
        small = {}
        for key in AMASS_SMALL:
            method, d0, csize, usize = mem[key]
            raw = _pread(fh, csize, d0, path)
            raw = _inflate(raw, usize, path, key) if method == 8 else raw
            dt, shape, hl = _npy_header(raw[:4096], path, key)
            cnt = int(np.prod(shape)) if shape else 1
            if hl + cnt * dt.itemsize > len(raw):
                raise ValueError(f"{path}: truncated")
            small[key] = np.frombuffer(raw, dtype=dt, count=cnt, offset=hl).reshape(shape).copy()
        arrays, need, T = {}, 0, None
        for key, width in AMASS_ARRAYS:
            method, d0, csize, usize = mem[key]
            if method == 8:  # (the header sits inside the deflate stream: shape and dtype are checked when the member is inflated)
                dt, shape, hl = None, None, None
            else:
                dt, shape, hl = _npy_header(_pread(fh, min(usize, 4096), d0, path), path, key)
                _check_amass_array(path, key, width, dt, shape, hl, usize)
                if T is not None and shape[0] != T:
                    raise ValueError(f"{path}: {key} has {shape[0]} frames, root_orient {T}")
                T = shape[0] if T is None else T
            arrays[key] = dict(method=method, at=d0, csize=csize, usize=usize, dtype=dt, shape=shape, hl=hl, off=need)
            room = usize if method == 8 else shape[0] * width * dt.itemsize  # (a deflated member's .npy header is at most that much too much)
            need += (room + _MEMBER_ALIGN - 1) // _MEMBER_ALIGN * _MEMBER_ALIGN
    g = small["gender"]
    if g.size != 1 or g.dtype.kind not in "US":
        raise ValueError(f"{path}: gender must be one string")
    g = g.reshape(-1)[0]
    gender = (g.decode("utf-8", "replace") if isinstance(g, bytes) else str(g)).strip().lower()
    if small["mocap_frame_rate"].size < 1 or small["mocap_frame_rate"].dtype.kind not in "fiu":
        raise ValueError(f"{path}: mocap_frame_rate must be a number")
    fps = float(small["mocap_frame_rate"].reshape(-1)[0])
    if not (fps > 0):
        raise ValueError(f"{path}: mocap_frame_rate must be positive")
    if small["betas"].dtype.kind != "f" or small["betas"].size < 1:
        raise ValueError(f"{path}: betas must be floating point")
    betas = small["betas"].astype(np.float64).reshape(-1)
    return dict(T=T, fps=fps, gender=gender, betas=betas, height=human_height_from_betas(betas), arrays=arrays), need


def _check_amass_array(path, key, width, dt, shape, hl, usize):
    if dt not in (np.dtype("<f4"), np.dtype("<f8")):
        raise ValueError(f"{path}: {key} must be float32 or float64")
    if len(shape) != 2 or shape[1] != width:
        raise ValueError(f"{path}: {key} has shape {shape}, expected [T, {width}]")
    if hl + shape[0] * width * dt.itemsize > usize:
        raise ValueError(f"{path}: truncated")


def _inflate(raw: bytes, usize: int, path: str, key: str) -> bytes:
    try:
        out = zlib.decompressobj(-15).decompress(raw, usize + 1)
    except zlib.error as ex:
        raise ValueError(f"{path}: member {key} does not inflate ({ex})") from None
    if len(out) != usize:
        raise ValueError(f"{path}: member {key} inflates to {len(out)} bytes, the directory says {usize}")
    return out


def _amass_fill(path: str, meta: dict, view: np.ndarray) -> None:
    """``fill_one``: the three arrays' numbers into the file's region of the pinned buffer, each on a 64-byte boundary.  A stored
    member is read from the disk straight to its place (one copy); a deflated one is inflated on this thread and copied there."""
    T = meta["T"]
    with open(path, "rb", buffering=0) as fh:
        for key, width in AMASS_ARRAYS:
            a = meta["arrays"][key]
            if a["method"] == 8:
                raw = _inflate(_pread(fh, a["csize"], a["at"], path), a["usize"], path, key)
                a["dtype"], a["shape"], a["hl"] = _npy_header(raw[:4096], path, key)
                _check_amass_array(path, key, width, a["dtype"], a["shape"], a["hl"], a["usize"])
                n = a["shape"][0] * width * a["dtype"].itemsize
                view[a["off"]:a["off"] + n] = np.frombuffer(raw, dtype=np.uint8, count=n, offset=a["hl"])
            else:
                n = a["shape"][0] * width * a["dtype"].itemsize
                dst, got = memoryview(view)[a["off"]:a["off"] + n], 0
                while got < n:
                    r = os.preadv(fh.fileno(), [dst[got:]], a["at"] + a["hl"] + got)
                    if not r:
                        raise ValueError(f"{path}: truncated")
                    got += r
            if T is not None and a["shape"][0] != T:
                raise ValueError(f"{path}: {key} has {a['shape'][0]} frames, another array {T}")
            T = a["shape"][0]
    meta["T"] = T


def read_amass_members(files, alloc, threads: int = 8, skip_errors: bool = False) -> Staged:
    """The files' per-frame arrays in one byte buffer from ``alloc(nbytes)`` (each file's region on a 256-byte boundary), their
    directories' findings in ``.parsed``: the host half of the AMASS loader, usable without a device."""
    return read_planned([str(f) for f in files], alloc, 256, _amass_plan, _amass_fill, threads, skip_errors)


def read_amass_file(path) -> dict:
    """One AMASS file's ``root_orient``, ``pose_body``, ``trans`` (as stored), ``betas`` (float64), ``gender``, ``mocap_frame_rate``
    through the loader's own parser (numpy arrays on the host)."""
    st = read_amass_members([path], lambda n: torch.empty(n, dtype=torch.uint8), 1, False)
    m, host = st.parsed[0], st.buf.numpy()
    out = dict(betas=m["betas"], gender=m["gender"], mocap_frame_rate=m["fps"])
    for key, width in AMASS_ARRAYS:
        a = m["arrays"][key]
        out[key] = np.frombuffer(host, dtype=a["dtype"], count=m["T"] * width, offset=int(st.starts[0]) + a["off"]).reshape(m["T"], width).copy()
    return out


def _amass_stage(files, dev: torch.device, threads: int, skip_errors: bool, slot: int) -> Staged:
    with torch.cuda.device(dev):
        return read_amass_members(files, pinned("amass", slot), threads, skip_errors)


def _amass_batch(st: Staged, dev, models, tgt_fps, columns, num_betas, skip_errors) -> SmplxBatch:
    """Staged AMASS members -> body model (all clips, one launch) -> the adapter, clip by clip as ``_joint_batch`` runs it."""
    from . import smplx_body
    # clips whose gender has no model (or whose betas do not fit num_betas) leave the batch here: skippable like a parse error
    good, clip_models, clip_betas, skipped = [], [], [], list(st.skipped)
    for k, m in enumerate(st.parsed):
        try:
            model = models.get(m["gender"])
            clip_betas.append(model.clip_betas(m["betas"], num_betas))
            clip_models.append(model)
            good.append(k)
        except ValueError as ex:
            if not skip_errors:
                raise ValueError(f"{st.files[k]}: {ex}") from None
            skipped.append((st.files[k], str(ex)))
    if not good:
        return SmplxBatch.empty(dev, skipped)
    names = list(SMPLX_JOINT_NAMES) if columns is None else [str(c) for c in columns]
    metas = [st.parsed[k] for k in good]
    t_out = [m["T"] // int(m["fps"] / tgt_fps) if tgt_fps < m["fps"] else m["T"] for m in metas]  # smpl.py:119,127
    offs = np.concatenate([[0], np.cumsum(t_out)]).astype(np.int64)
    B = len(names)
    with torch.cuda.device(dev):
        pos = torch.empty((int(offs[-1]), B, 3), dtype=torch.float64, device=dev)
        quat = torch.empty((int(offs[-1]), B, 4), dtype=torch.float64, device=dev)
        raw = st.buf[: st.total].to(dev, non_blocking=True)  # ONE copy of the members as they lie in the files
        clips = []
        for i, k in enumerate(good):
            m, base = metas[i], int(st.starts[k])
            c = dict(model=clip_models[i], betas=clip_betas[i])
            for key, width in AMASS_ARRAYS:
                a = m["arrays"][key]
                n = m["T"] * width * a["dtype"].itemsize
                c[key] = raw[base + a["off"]:base + a["off"] + n].view(torch.float32 if a["dtype"].itemsize == 4 else torch.float64).reshape(m["T"], width)
            clips.append(c)
        go, fp, jt, src = smplx_body.evaluate_clips(clips, device=dev.index or 0, columns=columns)
        out_fps = []
        for i, m in enumerate(metas):
            a, e = int(src[i]), int(src[i + 1])
            _, _, _, afps = get_smplx_data_offline_fast(go[a:e], fp[a:e], jt[a:e], SMPLX_PARENTS, src_fps=m["fps"], tgt_fps=tgt_fps, device=dev.index or 0,
                                                        columns=columns, out=(pos[offs[i]:offs[i + 1]], quat[offs[i]:offs[i + 1]]))
            out_fps.append(afps)
        torch.cuda.current_stream(dev).synchronize()  # the pinned buffer is reused by the batch after next
    return SmplxBatch(pos, quat, names, offs, [m["height"] for m in metas], out_fps, [st.files[k] for k in good], skipped)


def _model_set(body_models):
    from .smplx_body import BodyModelSet
    return body_models if isinstance(body_models, BodyModelSet) else BodyModelSet(body_models)


def load_amass_files(files, body_models, device: int = 0, tgt_fps: float = 30.0, columns: Optional[Sequence[str]] = None, threads: int = 8,
                     skip_errors: bool = False, num_betas: Optional[int] = None) -> SmplxBatch:
    """AMASS ``.npz`` files -> one ``SmplxBatch`` on the GPU, the body model included.  ``body_models``: the folder holding
    ``smplx/SMPLX_<GENDER>.npz|pkl`` (a gender's model is loaded when first needed) or a ``{gender: SmplxBodyModel}`` dict.
    ``num_betas``: shape coefficients used per clip (``None``: as many as the file and the model share)."""
    dev = torch.device("cuda", device)
    return _amass_batch(_amass_stage([str(f) for f in files], dev, threads, skip_errors, 0), dev, _model_set(body_models), tgt_fps, columns,
                        num_betas, skip_errors)


def iter_amass_batches(files, body_models, batch_files: int = 256, device: int = 0, tgt_fps: float = 30.0, columns: Optional[Sequence[str]] = None,
                       threads: int = 8, skip_errors: bool = False, num_betas: Optional[int] = None):
    """``load_amass_files`` over a folder in batches of ``batch_files`` files, read ahead like ``iter_joint_batches``.  A batch without a
    good file is yielded empty with its ``skipped`` list."""
    files = [str(f) for f in files]
    dev = torch.device("cuda", device)
    models = _model_set(body_models)
    groups = [files[i:i + batch_files] for i in range(0, len(files), max(1, batch_files))]
    yield from read_ahead(groups, lambda group, slot: _amass_stage(group, dev, threads, skip_errors, slot),
                          lambda st: _amass_batch(st, dev, models, tgt_fps, columns, num_betas, skip_errors))

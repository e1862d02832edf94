"""The SMPL-X body model's joints without the `smplx` package: the first arrow of scripts/smplx_to_robot_dataset.py:63-146.

``load_smplx_file`` (reference utils/smpl.py:12-41) evaluates the whole body model -- 10 475 skinned vertices per frame -- and the
retargeter reads 55 joints of it.  Those do not depend on vertices: the rest joints are ``J_regressor @ (v_template + shapedirs betas)``,
linear in ``betas``, and the posed joints are a rigid chain over them.  ``SmplxBodyModel`` folds the vertices away once per model file
(float64, on the host); ``evaluate_clips`` runs the chain for every clip of a batch in one launch (``gmr_smplx_body``), producing the
``global_orient`` / ``full_pose`` / ``joints`` arrays ``smplx_adapter.get_smplx_data_offline_fast`` takes.

The model file is the user's own (``SMPLX_{NEUTRAL,MALE,FEMALE}.npz|pkl``); nothing of it is stored by this package.  Pose-corrective
blend shapes and expression coefficients move vertices only and are not read.  Parity with the `smplx` package is unpinned (the
package cannot be installed next to this repository): DESIGN 4.8 lists the two documented deviations.
"""
from __future__ import annotations

import ctypes as C
import os
import pickle
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MODEL_KEYS = ("v_template", "shapedirs", "J_regressor", "kintree_table", "hands_meanl", "hands_meanr")
N_JOINTS = 55
GENDERS = ("neutral", "male", "female")


class SmplxBodyModel:
    """What the joint chain needs of one SMPL-X model file: ``J_template [J,3]``, ``J_dirs [J,3,nb]``, ``parents [J]``,
    ``hand_mean [90]`` (hands_meanl, hands_meanr), all float64 / int32 on the host; device copies are made on first use."""

    def __init__(self, J_template, J_dirs, parents, hand_mean, path: str = ""):
        self.J_template = np.ascontiguousarray(J_template, dtype=np.float64)
        self.J_dirs = np.ascontiguousarray(J_dirs, dtype=np.float64)
        self.parents = np.ascontiguousarray(parents, dtype=np.int32)
        self.hand_mean = np.ascontiguousarray(hand_mean, dtype=np.float64).reshape(-1)
        self.path = path
        self._dev: Dict[int, tuple] = {}

    @property
    def num_betas(self) -> int:
        return int(self.J_dirs.shape[2])

    @classmethod
    def from_file(cls, path, num_betas: Optional[int] = None) -> "SmplxBodyModel":
        """``.npz`` through numpy, ``.pkl`` through ``pickle.load(..., encoding="latin1")``; only ``MODEL_KEYS`` are read.
        ``num_betas``: shape columns kept (``None``: all the file has)."""
        from .smplx_adapter import SMPLX_PARENTS
        path = str(path)
        if path.endswith(".pkl"):
            with open(path, "rb") as f:
                data = pickle.load(f, encoding="latin1")
        else:
            data = np.load(path, allow_pickle=True)
        have = set(data.keys()) if hasattr(data, "keys") else set()
        for key in MODEL_KEYS:
            if key not in have:
                raise ValueError(f"{path}: no '{key}' in the model file (needed: {', '.join(MODEL_KEYS)})")

        def dense(a):
            a = a.toarray() if hasattr(a, "toarray") else a
            if isinstance(a, np.ndarray) and a.dtype == object and a.shape == ():
                a = a.item()
                a = a.toarray() if hasattr(a, "toarray") else a
            return np.asarray(a, dtype=np.float64)
        v_template, shapedirs, reg = dense(data["v_template"]), dense(data["shapedirs"]), dense(data["J_regressor"])
        kin = np.asarray(data["kintree_table"]).astype(np.int64)
        V = v_template.shape[0]
        if v_template.shape != (V, 3) or shapedirs.ndim != 3 or shapedirs.shape[:2] != (V, 3) or reg.ndim != 2 or reg.shape[1] != V:
            raise ValueError(f"{path}: v_template {v_template.shape}, shapedirs {shapedirs.shape}, J_regressor {reg.shape} do not fit each other")
        J = reg.shape[0]
        if kin.ndim != 2 or kin.shape[0] != 2 or kin.shape[1] != J:
            raise ValueError(f"{path}: kintree_table {kin.shape} does not describe {J} joints")
        nb = shapedirs.shape[2] if num_betas is None else int(num_betas)
        if nb < 0 or nb > shapedirs.shape[2]:
            raise ValueError(f"{path}: num_betas={num_betas}, the model has {shapedirs.shape[2]} shape columns")
        parents = kin[0].copy()
        parents[0] = -1
        if J != N_JOINTS or parents.tolist() != list(SMPLX_PARENTS):
            raise ValueError(f"{path}: not the SMPL-X kinematic tree ({J} joints; smplx_adapter.SMPLX_PARENTS has {len(SMPLX_PARENTS)})")
        hands = [dense(data[k]).reshape(-1) for k in ("hands_meanl", "hands_meanr")]
        if any(h.shape != (45,) for h in hands):
            raise ValueError(f"{path}: hands_meanl / hands_meanr must hold 45 numbers each")
        J_template = reg @ v_template
        J_dirs = np.einsum("jv,vcl->jcl", reg, shapedirs[:, :, :nb])
        return cls(J_template, J_dirs, parents, np.concatenate(hands), path)

    @classmethod
    def from_folder(cls, folder, gender: str, num_betas: Optional[int] = None) -> "SmplxBodyModel":
        """``<folder>/smplx/SMPLX_<GENDER>.npz``, then ``.pkl`` (the layout of the reference README:125-131)."""
        g = str(gender).lower()
        if g not in GENDERS:
            raise ValueError(f"unknown gender '{gender}' (one of {', '.join(GENDERS)})")
        for ext in (".npz", ".pkl"):
            p = os.path.join(str(folder), "smplx", f"SMPLX_{g.upper()}{ext}")
            if os.path.exists(p):
                return cls.from_file(p, num_betas)
        raise ValueError(f"no SMPLX_{g.upper()}.npz / .pkl under {os.path.join(str(folder), 'smplx')}")

    def clip_betas(self, betas, num_betas: Optional[int] = None) -> np.ndarray:
        """The betas a clip is evaluated with: the first ``num_betas`` of the file's (``None``: as many as the file and the model share)."""
        b = np.asarray(betas, dtype=np.float64).reshape(-1)
        nb = min(len(b), self.num_betas) if num_betas is None else int(num_betas)
        if nb > len(b) or nb > self.num_betas or nb < 0:
            raise ValueError(f"num_betas={nb}: the file has {len(b)} betas, the model {self.num_betas} shape columns")
        return np.ascontiguousarray(b[:nb])

    def rest_joints(self, betas) -> np.ndarray:
        """``J_template + J_dirs @ betas[:nb]`` -> [J, 3] (nb = what ``betas`` and the model share)."""
        b = self.clip_betas(betas)
        return self.J_template + self.J_dirs[:, :, :len(b)] @ b

    def on_device(self, device: int):
        """(J_template, J_dirs, hand_mean) as float64 tensors on the device, made once."""
        import torch
        t = self._dev.get(device)
        if t is None:
            dev = torch.device("cuda", device)
            t = tuple(torch.as_tensor(a).to(dev) for a in (self.J_template, self.J_dirs, self.hand_mean))
            self._dev[device] = t
        return t


class BodyModelSet:
    """``body_models`` of the loaders: a folder (a gender's model is loaded when its first clip arrives) or a {gender: model} dict."""

    def __init__(self, body_models):
        self.folder = None if isinstance(body_models, dict) else str(body_models)
        self.models: Dict[str, SmplxBodyModel] = {str(k).lower(): v for k, v in body_models.items()} if isinstance(body_models, dict) else {}

    def get(self, gender: str) -> SmplxBodyModel:
        g = str(gender).lower()
        m = self.models.get(g)
        if m is None:
            if self.folder is None or g not in GENDERS:
                raise ValueError(f"no body model for gender '{gender}'")
            m = self.models[g] = SmplxBodyModel.from_folder(self.folder, g)
        return m


def evaluate_clips(clips: Sequence[dict], device: int = 0, columns: Optional[Sequence[str]] = None, return_rest: bool = False):
    """All clips in one launch.  A clip is ``dict(model=SmplxBodyModel, betas=[nb] float64, root_orient=[T,3], pose_body=[T,63],
    trans=[T,3])`` with float32 or float64 CUDA tensors (contiguous, as they lie in the file).  -> ``(global_orient [N,3],
    full_pose [N,55,3], joints [N,55,3], offsets [n+1])`` float64 on the device, clip c at rows ``offsets[c]:offsets[c+1]``.
    ``columns``: only these joints and their ancestors are evaluated and written (the rows the adapter reads with the same ``columns``);
    the other joints' entries are uninitialised.  ``return_rest``: also the clips' rest joints ``[n,55,3]``."""
    import torch
    from . import _native
    from .smplx_adapter import SMPLX_JOINT_NAMES, SMPLX_PARENTS
    lib = _native.load()
    dev = torch.device("cuda", device)
    n = len(clips)
    lens = [int(c["root_orient"].shape[0]) for c in clips]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N = int(offs[-1])
    cols = None
    if columns is not None:
        names = list(SMPLX_JOINT_NAMES)
        missing = [c for c in columns if c not in names]
        if missing:
            raise KeyError(missing[0])
        cols = np.asarray([names.index(str(c)) for c in columns], dtype=np.int32)
    vp = C.c_void_p
    table = (_native.SmplxBodyClip * max(n, 1))()
    keep = []  # what the table points at, alive until the call has returned
    for k, c in enumerate(clips):
        m: SmplxBodyModel = c["model"]
        jt, jd, hm = m.on_device(device)
        b = np.ascontiguousarray(c["betas"], dtype=np.float64).reshape(-1)
        if len(b) > m.num_betas:
            raise ValueError(f"clip {k}: {len(b)} betas for a model of {m.num_betas} shape columns")
        e = table[k]
        for i, (key, width) in enumerate((("root_orient", 3), ("pose_body", 63), ("trans", 3))):
            t = c[key]
            if t.device != dev or not t.is_contiguous() or tuple(t.shape) != (lens[k], width) or t.dtype not in (torch.float32, torch.float64):
                raise ValueError(f"clip {k}: {key} must be a contiguous float32 / float64 [{lens[k]}, {width}] tensor on {dev}")
            setattr(e, key, t.data_ptr() or None)
            e.in_dtype[i] = _native.GMR_DTYPE_F32 if t.dtype == torch.float32 else _native.GMR_DTYPE_F64
        e.j_template, e.j_dirs, e.hand_mean = jt.data_ptr(), jd.data_ptr() or None, hm.data_ptr()
        e.betas = b.ctypes.data if len(b) else None
        e.n_frames, e.n_betas, e.dirs_stride = lens[k], len(b), m.num_betas
        keep.append((b, jt, jd, hm))
    with torch.cuda.device(dev):
        go = torch.empty((N, 3), dtype=torch.float64, device=dev)
        fp = torch.empty((N, N_JOINTS, 3), dtype=torch.float64, device=dev)
        jo = torch.empty((N, N_JOINTS, 3), dtype=torch.float64, device=dev)
        rest = torch.empty((n, N_JOINTS, 3), dtype=torch.float64, device=dev) if return_rest else None
        if n:
            parents = np.ascontiguousarray(SMPLX_PARENTS, dtype=np.int32)
            rc = lib.gmr_smplx_body(parents.ctypes.data_as(vp), N_JOINTS, table, n, cols.ctypes.data_as(vp) if cols is not None else None,
                                    len(cols) if cols is not None else 0, vp(go.data_ptr()), vp(fp.data_ptr()), vp(jo.data_ptr()),
                                    vp(rest.data_ptr()) if rest is not None and n else None, vp(torch.cuda.current_stream(dev).cuda_stream))
            if rc != 0:
                raise RuntimeError(f"gmr_smplx_body failed with status {rc}")
    del keep
    return (go, fp, jo, offs, rest) if return_rest else (go, fp, jo, offs)


class BodyOutput:
    """The three fields of the `smplx` package's output object that ``get_smplx_data_offline_fast`` reads, as float32 torch tensors."""

    def __init__(self, global_orient, full_pose, joints):
        self.global_orient, self.full_pose, self.joints = global_orient, full_pose, joints

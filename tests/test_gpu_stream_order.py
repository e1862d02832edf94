"""Every exported function with a ``void *stream`` parameter, on a busy stream (tests/stream_order.py has the schedules).

CASES maps each entry to the builder of its case; tests/test_stream_order_host.py checks that its keys are exactly the
stream-taking prototypes of include/gmr_amd.h, so a new entry point cannot be added without a case here.  The calls go through
ctypes with the handles of ``Engine`` / ``EngineGroup``: the harness has to own every device buffer (to late-produce it) and
every host array and struct the call receives (to overwrite it the moment the call returns), and the wrapper methods allocate
and convert those themselves.  Every decoy is a complete valid input: whatever order the library reads things in, it computes a
wrong answer and never an address out of range.

SYNCHRONISES lists the entries that the header says synchronise the stream before they return; every other entry must return
while its producer is still spinning.  Measured on one MI355X (ROCm 7): profiles/stream_order.json, DESIGN.md "Stream order".

Run as a module from the repository root (``python -m tests.test_gpu_stream_order OUT.json``) it writes that profile."""
import ctypes as C
import functools
import sys
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gmr_amd import _native  # noqa: E402
from tests import stream_order as so  # noqa: E402
from tests.util import compiled  # noqa: E402

vp = C.c_void_p
F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
SYNCHRONISES = {"gmr_bvh_parse_motion_device"}  # (the header: "Runs on `stream` and synchronises it before returning")
IK_LENS = [24, 1, 40]
KIN_OFFS = np.array([0, 70, 71, 200], np.int64)          # clips of 70, 1 and 129 frames
KIN_OFFS_DECOY = np.array([0, 60, 129, 200], np.int64)
N_KIN = 200


def DEV():
    return torch.device("cuda", 0)


def P(t):
    return vp(t.data_ptr()) if t is not None and t.numel() else None


def H(a):
    return a.ctypes.data_as(vp)


@functools.lru_cache(maxsize=None)
def _engine():
    from gmr_amd.engine import Engine
    return Engine(compiled("smplx", "unitree_g1"), 0)


@functools.lru_cache(maxsize=None)
def _group():
    from gmr_amd.engine import EngineGroup
    return EngineGroup([compiled("smplx", "unitree_g1"), compiled("smplx", "booster_t1")], 0)


def _lib():
    return _native.load()


def _gen(seed):
    return torch.Generator(device=DEV()).manual_seed(int(seed))


def _randn(g, shape, dtype=F64, scale=1.0):
    return (torch.randn(shape, generator=g, dtype=F64, device=DEV()) * scale).to(dtype)


def _unit(g, shape, dtype=F64):
    q = torch.randn(shape, generator=g, dtype=F64, device=DEV())
    return (q / q.norm(dim=-1, keepdim=True)).to(dtype).contiguous()


def _qpos(cm, n, seed):
    """Hinges uniform within the joint ranges, unit root quaternions (wxyz), root positions around a standing height."""
    r = cm.robot
    rng = np.random.default_rng(seed)
    hb = sorted(r.hinge_bodies(), key=lambda b: r.qpos_adr[b])
    lim = np.array(r.jnt_range, dtype=np.float64)[hb]
    lo = np.where(lim[:, 0] < lim[:, 1], lim[:, 0], -1.0)
    hi = np.where(lim[:, 0] < lim[:, 1], lim[:, 1], 1.0)
    q = np.empty((n, r.nq))
    q[:, :3] = rng.normal(size=(n, 3)) * [2.0, 2.0, 0.2] + [0.0, 0.0, 0.8]
    w = rng.normal(size=(n, 4))
    q[:, 3:7] = w / np.linalg.norm(w, axis=1, keepdims=True)
    q[:, 7:] = rng.uniform(lo, hi, size=(n, len(hb)))
    return torch.from_numpy(q).to(DEV())


def _keypoints(cm, n, seed, dtype=F64):
    """Random key-points: one column nothing consumes, then one per slot."""
    g = _gen(seed)
    pos = (_randn(g, (n, cm.nslot + 1, 3), scale=0.5) + torch.tensor([0.0, 0.0, 0.9], dtype=F64, device=DEV())).to(dtype).contiguous()
    return pos, _unit(g, (n, cm.nslot + 1, 4), dtype)


def _slot_cols(cm):
    """(true, decoy): slot s reads column s + 1; the decoy is another assignment of the same columns."""
    a = np.arange(cm.nslot, dtype=np.int32)
    return a + 1, np.roll(a, 1).astype(np.int32) + 1


def _random_tree(rng, J):
    par = np.full(J, -1, dtype=np.int32)
    for j in range(1, J):
        par[j] = j - 1 if rng.random() < 0.6 else rng.integers(0, j)
    return par


# ------------------------------------------------------------------ cases without structs
class Plain(so.Case):
    def __init__(self, entry, call, launches, h2d):
        super().__init__()
        self.entry, self._call, self.launches, self.h2d = entry, call, launches, h2d

    def invoke(self, b, st, stream):
        return self._call(b, stream)


def _fk_inputs(cm, v, n=N_KIN):
    out = {}
    for k, seed in ((0, 100 + 10 * v), (1, 105 + 10 * v)):
        g = _gen(seed)
        out[k] = (_randn(g, (n, 3), F32), _unit(g, (n, 4), F32), _randn(g, (n, cm.robot.nq - 7), F32, 0.5))
    return {"root_pos": (out[0][0], out[1][0]), "root_rot": (out[0][1], out[1][1]), "dof": (out[0][2], out[1][2])}


def case_fk(v, shape=False, min_height=False, offsets=None, n=N_KIN, eng=None, want_rot=True):
    """n, eng, want_rot: the guard-band tests' other lengths, another model's handle and the call with body_rot = NULL."""
    eng, lib = eng or _engine(), _lib()
    cm, nb = eng.cm, eng.nbody
    rot = (lambda b: P(b.out["body_rot"])) if want_rot else (lambda b: None)
    if min_height:
        offs = (KIN_OFFS, KIN_OFFS_DECOY) if offsets is None else offsets
        n_seq = len(offs[0]) - 1
        c = Plain("gmr_fk_min_height", lambda b, s: lib.gmr_fk_min_height(eng._h, P(b.dev["root_pos"]), P(b.dev["root_rot"]), P(b.dev["dof"]),
                                                                          H(b.host["seq_offsets"]), n_seq, P(b.out["min_z"]), s), 3, 1)
        c.host_in = {"seq_offsets": offs}
        c.out_spec = {"min_z": ((n_seq,), F32)}
        c.dev_in = _fk_inputs(cm, v, int(offs[0][-1]))
        return c
    elif shape:
        c = Plain("gmr_fk_shape", lambda b, s: lib.gmr_fk_shape(eng._h, P(b.dev["root_pos"]), P(b.dev["root_rot"]), P(b.dev["dof"]), P(b.dev["shape"]), 3,
                                                                n, P(b.out["body_pos"]), rot(b), s), 2, 0)
    else:
        c = Plain("gmr_fk", lambda b, s: lib.gmr_fk(eng._h, P(b.dev["root_pos"]), P(b.dev["root_rot"]), P(b.dev["dof"]), n, P(b.out["body_pos"]),
                                                    rot(b), s), 1, 0)
    c.dev_in = _fk_inputs(cm, v, n)
    if shape:
        g = _gen(120 + v)
        c.dev_in["shape"] = tuple((1.0 + 0.2 * torch.rand((nb, 3), generator=g, dtype=F64, device=DEV())).to(F32) for _ in range(2))
    if not min_height:
        c.out_spec = {"body_pos": ((n, nb, 3), F32)}
        if want_rot:
            c.out_spec["body_rot"] = ((n, nb, 4), F32)
    return c


def case_kin(v, name, n=N_KIN):
    eng, lib = _engine(), _lib()
    nb, nd = eng.nbody, eng.nq - 7
    shapes = {"gmr_dof_to_rot": ((n, nd), (n, nb - 1, 4)), "gmr_rot_to_dof": ((n, nb - 1, 4), (n, nd)),
              "gmr_local_rot_to_global": ((n, nb, 4), (n, nb, 4))}[name]
    fn = getattr(lib, name)
    c = Plain(name, lambda b, s: fn(eng._h, P(b.dev["x"]), n, P(b.out["y"]), s), 1, 0)
    make = (lambda g: _randn(g, shapes[0], F32, 0.5)) if name == "gmr_dof_to_rot" else (lambda g: _unit(g, shapes[0], F32))
    c.dev_in = {"x": (make(_gen(130 + 10 * v)), make(_gen(135 + 10 * v)))}
    c.out_spec = {"y": (shapes[1], F32)}
    return c


def case_evaluate(v, n=N_KIN, omit=()):
    """omit: the outputs passed as NULL (the guard-band tests leave each out in turn)."""
    eng, lib = _engine(), _lib()
    cm = eng.cm
    nt = eng.info.ntask[0] + eng.info.ntask[1]
    pt, qt = _keypoints(cm, n, 140 + 10 * v)
    pd, qd = _keypoints(cm, n, 145 + 10 * v)
    O = lambda b, k: P(b.out.get(k))  # noqa: E731
    c = Plain("gmr_evaluate", lambda b, s: lib.gmr_evaluate(eng._h, P(b.dev["qpos"]), n, P(b.dev["pos"]), P(b.dev["quat"]), _native.GMR_DTYPE_F64,
                                                            cm.nslot + 1, H(b.host["slot_col"]), 0, None, O(b, "err"), O(b, "task_err"),
                                                            O(b, "xpos"), O(b, "xquat"), s), 1, 1)
    c.dev_in = {"qpos": (_qpos(cm, n, 141 + 10 * v), _qpos(cm, n, 146 + 10 * v)), "pos": (pt, pd), "quat": (qt, qd)}
    c.host_in = {"slot_col": _slot_cols(cm)}
    c.out_spec = {"err": ((n, 2), F64), "task_err": ((n, nt, 6), F64), "xpos": ((n, eng.nbody, 3), F64), "xquat": ((n, eng.nbody, 4), F64)}
    for k in omit:
        del c.out_spec[k]
    return c


SMPLX_T, SMPLX_TOUT, SMPLX_STRIDE = 130, 65, 60


def case_smplx(v, name, T=SMPLX_T, T_out=SMPLX_TOUT):
    from gmr_amd import synth
    from gmr_amd.smplx_adapter import SMPLX_JOINT_NAMES, SMPLX_PARENTS
    lib = _lib()
    J = 55
    f32 = name == "gmr_smplx_keypoints_in"
    arrs = [synth.smplx_arrays_torch(T, DEV(), J, SMPLX_STRIDE, seed=150 + 10 * v + k) for k in (0, 5)]
    if f32:
        arrs = [tuple(a.to(F32) for a in t) for t in arrs]
    rng = np.random.default_rng(150 + v)
    par = (np.asarray(SMPLX_PARENTS, np.int32), _random_tree(rng, J))
    cols = [np.asarray([SMPLX_JOINT_NAMES.index(n) for n in _engine().cm.slot_names], np.int32)]
    n_out = len(cols[0])
    cols.append(rng.permutation(J)[:n_out].astype(np.int32))
    if name == "gmr_smplx_keypoints":
        B = J
        call = lambda b, s: lib.gmr_smplx_keypoints(H(b.host["parents"]), J, SMPLX_STRIDE, P(b.dev["go"]), P(b.dev["fp"]), P(b.dev["jt"]), T,  # noqa: E731
                                                    T_out, 1, P(b.out["pos"]), P(b.out["quat"]), s)
    elif name == "gmr_smplx_keypoints_cols":
        B = n_out
        call = lambda b, s: lib.gmr_smplx_keypoints_cols(H(b.host["parents"]), J, SMPLX_STRIDE, P(b.dev["go"]), P(b.dev["fp"]), P(b.dev["jt"]), T,  # noqa: E731
                                                         T_out, 1, H(b.host["out_cols"]), n_out, P(b.out["pos"]), P(b.out["quat"]), s)
    else:
        B = n_out
        call = lambda b, s: lib.gmr_smplx_keypoints_in(H(b.host["parents"]), J, SMPLX_STRIDE, P(b.dev["go"]), P(b.dev["fp"]), P(b.dev["jt"]),  # noqa: E731
                                                       _native.GMR_DTYPE_F32, T, T_out, 1, H(b.host["out_cols"]), n_out, P(b.out["pos"]),
                                                       P(b.out["quat"]), s)
    c = Plain(name, call, 1, 0)
    c.dev_in = {k: (arrs[0][i], arrs[1][i]) for i, k in enumerate(("go", "fp", "jt"))}
    c.host_in = {"parents": par}
    if B != J:
        c.host_in["out_cols"] = tuple(cols)
    c.out_spec = {"pos": ((T_out, B, 3), F64), "quat": ((T_out, B, 4), F64)}
    return c


BVH_T = 130


def case_bvh_fk(v, rows, n=BVH_T):
    from gmr_amd import synth
    lib = _lib()
    data = [synth.lafan_rows_torch(n, DEV(), seed=160 + 10 * v + k) for k in (0, 5)]
    parents, offsets = data[0][1], data[0][2]
    J = len(parents)
    rng = np.random.default_rng(160 + v)
    host = {"parents": (parents, _random_tree(rng, J)), "order": (np.array([2, 1, 0], np.int32), np.array([0, 2, 1], np.int32)),
            "extra_pos": (np.array([3, 7], np.int32), np.array([5, 2], np.int32)), "extra_rot": (np.array([4, 8], np.int32), np.array([1, 9], np.int32))}
    if rows:
        n_out = 14
        host["out_cols"] = (rng.permutation(J + 2)[:n_out].astype(np.int32), rng.permutation(J + 2)[:n_out].astype(np.int32))
        c = Plain("gmr_bvh_fk_rows", lambda b, s: lib.gmr_bvh_fk_rows(H(b.host["parents"]), J, H(b.host["order"]), H(b.host["extra_pos"]), H(b.host["extra_rot"]), 2, 3,
                                                                      P(b.dev["offsets"]), P(b.dev["rows"]), 3 + 3 * J, n, 0.01, H(b.host["out_cols"]), n_out,
                                                                      P(b.out["pos"]), P(b.out["quat"]), s), 1, 0)
        off = torch.from_numpy(offsets).to(DEV())
        c.dev_in = {"rows": (data[0][0], data[1][0]), "offsets": (off, off * 1.1)}
    else:
        n_out = J + 2
        c = Plain("gmr_bvh_fk", lambda b, s: lib.gmr_bvh_fk(H(b.host["parents"]), J, H(b.host["order"]), H(b.host["extra_pos"]), H(b.host["extra_rot"]), 2,
                                                            P(b.dev["lpos"]), P(b.dev["eul"]), n, 0.01, P(b.out["pos"]), P(b.out["quat"]), s), 1, 0)
        g = _gen(165 + v)
        c.dev_in = {"lpos": (_randn(g, (n, J, 3), scale=20.0), _randn(g, (n, J, 3), scale=20.0)),
                    "eul": (_randn(g, (n, J, 3)), _randn(g, (n, J, 3)))}
    c.host_in = host
    c.out_spec = {"pos": ((n, n_out, 3), F64), "quat": ((n, n_out, 4), F64)}
    return c


class BvhParse(so.Case):
    """Two files of 11 rows x 69 numbers (about 6 KB each) in one blob, one number of 25 digits (off the device's fast path) in each.
    The decoy text has the same bytes but for the digits; the decoy tables read the files in the other order, ten rows each."""
    entry, synchronises, launches, h2d = "gmr_bvh_parse_motion_device", True, 3, 1
    sort_rows = ("slow",)
    LINES, COLS, MAX_SLOW = 11, 69, 8

    def __init__(self, v):
        super().__init__()
        texts, ends = [], None
        for seed in (170 + 10 * v, 175 + 10 * v):
            rng = np.random.default_rng(seed)
            files = []
            for f in range(2):
                vals = rng.uniform(-999.0, 999.0, (self.LINES, self.COLS))
                toks = [["%+09.4f" % x for x in row] for row in vals]
                toks[3 + f][7] = "%+d." % rng.integers(1, 9) + "".join(str(d) for d in rng.integers(0, 10, 24))   # 25 digits
                files.append(("\n".join(" ".join(r) for r in toks) + "\n").encode())
            texts.append(b"".join(files))
            ends = [len(files[0]), len(files[0]) + len(files[1])]
        assert len(texts[0]) == len(texts[1])
        self.n_bytes = len(texts[0])
        self.dev_in = {"text": tuple(torch.from_numpy(np.frombuffer(t, np.uint8).copy()).to(DEV()) for t in texts)}
        i64 = lambda *a: np.array(a, np.int64)  # noqa: E731
        self.host_in = {"seg_begin": (i64(0, ends[0]), i64(ends[0], 0)), "seg_end": (i64(ends[0], ends[1]), i64(ends[1], ends[0])),
                        "n_lines": (i64(self.LINES, self.LINES), i64(self.LINES - 1, self.LINES - 1)), "row_begin": (i64(0, self.LINES), i64(self.LINES, 0))}
        self.out_spec = {"rows": ((2 * self.LINES, self.COLS), F64)}
        self.host_out_spec = {"status": ((2,), np.int32), "n_tokens": ((2,), np.int64), "slow": ((self.MAX_SLOW, 3), np.int64), "n_slow": ((1,), np.int64)}

    def sort_rows_count(self, b, a):
        return int(min(max(int(b.host_out["n_slow"][0]), 0), self.MAX_SLOW))

    def written(self, b, name):
        """Leading rows of an output the call writes (None: all): the rows of ``slow`` behind n_slow are left alone."""
        return self.sort_rows_count(b, None) if name == "host:slow" else None

    def invoke(self, b, st, stream):
        h, o = b.host, b.host_out
        return _lib().gmr_bvh_parse_motion_device(P(b.dev["text"]), self.n_bytes, 2, H(h["seg_begin"]), H(h["seg_end"]), H(h["n_lines"]), self.COLS, H(h["row_begin"]),
                                                  P(b.out["rows"]), H(o["status"]), H(o["n_tokens"]), H(o["slow"]), self.MAX_SLOW, H(o["n_slow"]), stream)


# ------------------------------------------------------------------ the batched IK calls
def _items(spans):
    it = np.zeros(len(spans), dtype=_native.WORK_ITEM_DTYPE)
    it["frame_begin"], it["n_out"] = [a for a, _ in spans], [n for _, n in spans]
    it["init_row"], it["final_row"], it["burn_row"], it["height_scale"] = -1, -1, -1, 1.0
    return it


# the clips of 24, 1 and 40 frames as nine work items; the decoy covers the same frames, split at other rows
IK_SPANS = [(0, 8), (8, 8), (16, 8), (24, 1), (25, 8), (33, 8), (41, 8), (49, 8), (57, 8)]
IK_SPANS_DECOY = [(0, 12), (12, 8), (20, 4), (24, 1), (25, 5), (30, 10), (40, 8), (48, 8), (56, 9)]
IK_FRAMES, IK_ITEMS, IK_PROBE = 65, 9, 4


class IKCase(so.Case):
    """mode: 'solve' | 'plan' | 'ordered'; group: the gmr_group_* form on unitree_g1 + booster_t1."""

    struct_values = True

    def __init__(self, v, mode, group, dtype=F32):
        super().__init__()
        from gmr_amd import synth
        self.mode, self.group = mode, group
        self.in_dtype = _native.GMR_DTYPE_F32 if dtype == F32 else _native.GMR_DTYPE_F64
        self.entry = {("solve", False): "gmr_ik_solve", ("plan", False): "gmr_ik_plan_order", ("ordered", False): "gmr_ik_solve_ordered",
                      ("solve", True): "gmr_group_ik_solve", ("plan", True): "gmr_group_plan_order", ("ordered", True): "gmr_group_ik_solve_ordered"}[mode, group]
        self.engines = _group().engines if group else [_engine()]
        n = len(self.engines)
        self.launches = 2 if mode == "plan" else 1
        self.h2d = 3 * n + (2 if group else 0) + (1 if mode == "plan" else 0)
        self.prm = (_native.IKParams(), _native.IKParams(damping=0.7))
        for i, eng in enumerate(self.engines):
            cm = eng.cm
            kp = []
            for seed, hard in ((200 + 10 * v + i, False), (205 + 10 * v + i, True)):
                pos, quat, _, _ = synth.synth_clips_torch(cm, IK_LENS, seed, DEV(), hard=hard, yaw0=1.0, dtype=dtype)
                pad_p = torch.zeros((IK_FRAMES, 1, 3), dtype=dtype, device=DEV())
                pad_q = torch.zeros((IK_FRAMES, 1, 4), dtype=dtype, device=DEV())
                pad_q[..., 0] = 1.0
                kp.append((torch.cat([pad_p, pos], 1).contiguous(), torch.cat([pad_q, quat], 1).contiguous()))
            self.dev_in[f"pos{i}"], self.dev_in[f"quat{i}"] = (kp[0][0], kp[1][0]), (kp[0][1], kp[1][1])
            self.host_in[f"slot_col{i}"] = _slot_cols(cm)
            self.host_in[f"items{i}"] = (_items(IK_SPANS), _items(IK_SPANS_DECOY))
            if mode != "plan":
                self.out_spec[f"qpos{i}"], self.out_spec[f"iters{i}"] = ((IK_FRAMES, eng.nq), F64), ((IK_FRAMES,), I32)
        tot = IK_ITEMS * n
        if mode == "plan":
            self.out_spec["order"] = ((tot,), I32)
        if mode == "ordered":
            rng = np.random.default_rng(210 + v)
            self.dev_in["launch_order"] = tuple(torch.from_numpy(rng.permutation(tot).astype(np.int32)).to(DEV()) for _ in range(2))

    def new_struct(self):
        return {"inp": (_native.GroupInput * len(self.engines))(), "prm": _native.IKParams()}

    def fill(self, st, b, decoy):
        C.memmove(C.byref(st["prm"]), C.byref(self.prm[1 if decoy else 0]), C.sizeof(_native.IKParams))
        for i, eng in enumerate(self.engines):
            e = st["inp"][i]
            e.human_pos, e.human_quat = b.dev[f"pos{i}"].data_ptr(), b.dev[f"quat{i}"].data_ptr()
            e.in_dtype, e.n_cols, e.n_frames, e.n_items = self.in_dtype, eng.cm.nslot + 1, IK_FRAMES, IK_ITEMS
            e.slot_col, e.items = b.host[f"slot_col{i}"].ctypes.data, b.host[f"items{i}"].ctypes.data
            if self.mode != "plan":
                e.qpos_out, e.iters_out = b.out[f"qpos{i}"].data_ptr(), b.out[f"iters{i}"].data_ptr()

    def invoke(self, b, st, stream):
        lib, prm = _lib(), C.byref(st["prm"])
        if self.group:
            g = _group()._g
            if self.mode == "solve":
                return lib.gmr_group_ik_solve(g, st["inp"], prm, stream)
            if self.mode == "plan":
                return lib.gmr_group_plan_order(g, st["inp"], prm, IK_PROBE, P(b.out["order"]), stream)
            return lib.gmr_group_ik_solve_ordered(g, st["inp"], prm, P(b.dev["launch_order"]), stream)
        eng = self.engines[0]
        batch = (eng._h, P(b.dev["pos0"]), P(b.dev["quat0"]), self.in_dtype, eng.cm.nslot + 1, H(b.host["slot_col0"]), IK_FRAMES, H(b.host["items0"]),
                 IK_ITEMS, prm, None)
        if self.mode == "plan":
            return lib.gmr_ik_plan_order(*batch, IK_PROBE, P(b.out["order"]), stream)
        solve = batch + (None, P(b.out["qpos0"]), P(b.out["iters0"]), None, None)
        if self.mode == "solve":
            return lib.gmr_ik_solve(*solve, stream)
        return lib.gmr_ik_solve_ordered(*solve, P(b.dev["launch_order"]), stream)


# ------------------------------------------------------------------ the post-solve kernels that take a struct per model
TRACK_FPS_OUT = 50.0


class MotionCase(so.Case):
    """kind: 'epilogue' | 'track' | 'report'; group: the gmr_group_* form.  Struct field names are the keys of the working sets."""

    struct_values = True
    epilogue_flags = _native.MOTION_HEIGHT_ADJUST | _native.MOTION_ROOT_ORIGIN

    def __init__(self, v, kind, group, offs=None):
        """offs: (true, decoy) tables of three clips other than KIN_OFFS (the guard-band tests' other lengths; not for 'track')."""
        super().__init__()
        from gmr_amd.schedule import track_plan
        assert offs is None or kind != "track"
        self.kind, self.group = kind, group
        self.offs = (KIN_OFFS, KIN_OFFS_DECOY) if offs is None else offs
        n = self.n_frames = int(self.offs[0][-1])
        base = {"epilogue": "motion_epilogue", "track": "motion_track", "report": "clip_report"}[kind]
        self.entry = ("gmr_group_" if group else "gmr_") + base
        self.engines = _group().engines if group else [_engine()]
        self.launches, self.h2d = {"epilogue": 3, "track": 1, "report": 2}[kind], 1
        self.stype = {"epilogue": _native.MotionInput, "track": _native.TrackInput, "report": _native.ClipReportInput}[kind]
        self.dev_names, self.host_names, self.out_names = [], [], []
        if kind == "track":
            self.out_offs, ratio = track_plan(KIN_OFFS, 30.0, TRACK_FPS_OUT)   # an unequal rate: 200 frames -> 331
            M = int(self.out_offs[-1])
            decoy_out = np.array([0, 100, 117, M], np.int64)
            assert M > 117
        for i, eng in enumerate(self.engines):
            cm, nq, nb, nd = eng.cm, eng.nq, eng.nbody, eng.nq - 7
            nt = eng.info.ntask[0] + eng.info.ntask[1]
            dev = {"qpos": (_qpos(cm, n, 300 + 10 * v + i), _qpos(cm, n, 305 + 10 * v + i))}
            host = {"seq_offsets": self.offs}
            if kind == "epilogue":
                out = {"root_pos_out": ((n, 3), F64), "root_rot_out": ((n, 4), F64), "dof_pos_out": ((n, nd), F64),
                       "local_body_pos_out": ((n, nb, 3), F32), "min_z_out": ((3,), F32)}
            elif kind == "track":
                host["out_offsets"] = (self.out_offs, decoy_out)
                host["ratio"] = (ratio, np.array([0.5, 0.7, 0.61]))
                tail = {"root_pos": (3,), "root_rot": (4,), "joint_pos": (nd,), "root_lin_vel": (3,), "root_ang_vel": (3,), "joint_vel": (nd,),
                        "body_pos_w": (nb, 3), "body_quat_w": (nb, 4), "body_lin_vel_w": (nb, 3), "body_ang_vel_w": (nb, 3)}
                out = {k + "_out": ((M,) + t, F32 if k.startswith("body_") else F64) for k, t in tail.items()}
            else:
                pt, qt = _keypoints(cm, n, 310 + 10 * v + i)
                pd, qd = _keypoints(cm, n, 315 + 10 * v + i)
                g = _gen(320 + 10 * v + i)
                its = tuple(torch.randint(1, 20, (n,), generator=g, device=DEV(), dtype=I64).to(I32) for _ in range(2))
                dev.update(human_pos=(pt, pd), human_quat=(qt, qd), iters=its)
                host["slot_col"] = _slot_cols(cm)
                S = 3
                out = {"err_max_out": ((S, 2), F64), "err_sum_out": ((S, 2), F64), "task_pos_max_out": ((S, nt), F64), "task_pos_sum_out": ((S, nt), F64),
                       "task_rot_max_out": ((S, nt), F64), "task_rot_sum_out": ((S, nt), F64), "near_lo_out": ((S, nd), I32), "near_hi_out": ((S, nd), I32),
                       "dof_step_max_out": ((S, nd), F64), "root_step_max_out": ((S,), F64), "root_turn_max_out": ((S,), F64),
                       "solves_max_out": ((S,), I32), "solves_sum_out": ((S,), I64), "nonfinite_frames_out": ((S,), I32)}
            if i == 0:
                self.dev_names, self.host_names, self.out_names = list(dev), list(host), list(out)
            self.dev_in.update({f"{k}{i}": p for k, p in dev.items()})
            self.host_in.update({f"{k}{i}": p for k, p in host.items()})
            self.out_spec.update({f"{k}{i}": p for k, p in out.items()})
        self.rprm = (_native.ClipReportParams(segment_frames=16), _native.ClipReportParams(limit_eps=2e-3, segment_frames=16))

    def new_struct(self):
        return {"inp": (self.stype * len(self.engines))(), "prm": _native.ClipReportParams()}

    def fill(self, st, b, decoy):
        C.memmove(C.byref(st["prm"]), C.byref(self.rprm[1 if decoy else 0]), C.sizeof(_native.ClipReportParams))
        for i, eng in enumerate(self.engines):
            e = st["inp"][i]
            for k in self.dev_names:
                setattr(e, k, b.dev[f"{k}{i}"].data_ptr())
            for k in self.host_names:
                setattr(e, k, b.host[f"{k}{i}"].ctypes.data)
            for k in self.out_names:
                setattr(e, k, b.out[f"{k}{i}"].data_ptr())
            e.n_frames, e.n_seq = self.n_frames, 3
            if self.kind == "epilogue":
                e.flags, e.ground_offset = self.epilogue_flags, 0.05 if decoy else 0.02
            elif self.kind == "track":
                e.fps_out = TRACK_FPS_OUT
            else:
                e.in_dtype, e.n_cols = _native.GMR_DTYPE_F64, eng.cm.nslot + 1

    def invoke(self, b, st, stream):
        lib = _lib()
        h = _group()._g if self.group else self.engines[0]._h
        fn = getattr(lib, self.entry)
        if self.kind == "report":
            return fn(h, st["inp"], C.byref(st["prm"]), stream)
        return fn(h, st["inp"], stream)


class SampleCase(so.Case):
    """130 queries, two per id (K = 2), five selected bodies; every array is a device array, the struct travels as the kernel's argument."""
    entry, launches, h2d = "gmr_motion_sample", 1, 0
    Q, K, NSEL = 130, 2, 5

    def __init__(self, v):
        super().__init__()
        eng = _engine()
        cm, nb, nd = eng.cm, eng.nbody, eng.nq - 7
        rng = np.random.default_rng(400 + v)
        T = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV())  # noqa: E731

        def queries(offs):
            ids = rng.integers(0, 3, self.Q // self.K)
            dur = (np.diff(offs)[ids] - 1) / 30.0
            return T(ids, I64), T(np.repeat(dur, self.K) * rng.uniform(-0.1, 1.1, self.Q), F64)
        it, tt = queries(KIN_OFFS)
        idd, td = queries(KIN_OFFS_DECOY)
        self.dev_in = {"qpos": (_qpos(cm, N_KIN, 401 + 10 * v), _qpos(cm, N_KIN, 406 + 10 * v)), "seq_offsets": (T(KIN_OFFS, I64), T(KIN_OFFS_DECOY, I64)),
                       "fps": (T([30.0, 30.0, 30.0], F64), T([24.0, 60.0, 50.0], F64)), "ids": (it, idd), "times": (tt, td),
                       "body_ids": (T(rng.permutation(nb)[:self.NSEL], I32), T(rng.permutation(nb)[:self.NSEL], I32))}
        tail = {"root_pos": (3,), "root_rot": (4,), "joint_pos": (nd,), "root_lin_vel": (3,), "root_ang_vel": (3,), "joint_vel": (nd,),
                "body_pos_w": (self.NSEL, 3), "body_quat_w": (self.NSEL, 4), "body_lin_vel_w": (self.NSEL, 3), "body_ang_vel_w": (self.NSEL, 3)}
        self.out_spec = {k + "_out": ((self.Q,) + t, F32 if k.startswith("body_") else F64) for k, t in tail.items()}

    def new_struct(self):
        return _native.SampleInput()

    def fill(self, st, b, decoy):
        for k, t in b.dev.items():
            setattr(st, k, t.data_ptr())
        for k, t in b.out.items():
            setattr(st, k, t.data_ptr())
        st.n_frames, st.n_seq, st.k_per_id, st.n_queries, st.n_sel = N_KIN, 3, self.K, self.Q, self.NSEL
        st.time_dtype = st.out_dtype = _native.GMR_DTYPE_F64

    def invoke(self, b, st, stream):
        return _lib().gmr_motion_sample(_engine()._h, C.byref(st), stream)


_MODEL_DIR = []


class SmplxBodyCase(so.Case):
    """Three clips (33, 0 and 70 frames; 16, 10 and 0 betas) on the synthetic model folder; the decoy is another gender's model,
    other motion, other betas, another tree and another column selection."""
    entry, launches, h2d = "gmr_smplx_body", 2, 1
    LENS, NBETA = (33, 0, 70), (16, 10, 0)

    def __init__(self, v):
        super().__init__()
        from gmr_amd import synth
        from gmr_amd.smplx_adapter import SMPLX_JOINT_NAMES, SMPLX_PARENTS
        from gmr_amd.smplx_body import BodyModelSet
        if not _MODEL_DIR:
            _MODEL_DIR.append(tempfile.TemporaryDirectory())
            synth.write_smplx_model_folder(_MODEL_DIR[0].name, seed=3)
        models = BodyModelSet(_MODEL_DIR[0].name)
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV())  # noqa: E731
        ms = [models.get("neutral"), models.get("male")]
        self.dirs_stride = ms[0].num_betas
        assert ms[1].num_betas == self.dirs_stride
        self.dev_in = {"j_template": tuple(T(m.J_template) for m in ms), "j_dirs": tuple(T(m.J_dirs) for m in ms), "hand_mean": tuple(T(m.hand_mean) for m in ms)}
        for k, n in enumerate(self.LENS):
            a = [synth.amass_arrays(max(n, 1), 500 + 10 * v + 5 * d + k, np.float32 if k == 2 else np.float64, big=True) for d in (0, 1)]
            if n:
                for key in ("root_orient", "pose_body", "trans"):
                    self.dev_in[f"{key}{k}"] = tuple(T(x[key][:n]) for x in a)
            if self.NBETA[k]:
                self.host_in[f"betas{k}"] = tuple(np.ascontiguousarray(x["betas"][:self.NBETA[k]], dtype=np.float64) for x in a)
        rng = np.random.default_rng(500 + v)
        cols = np.asarray([SMPLX_JOINT_NAMES.index(n) for n in _engine().cm.slot_names], np.int32)
        self.n_out = len(cols)
        self.host_in["parents"] = (np.asarray(SMPLX_PARENTS, np.int32), _random_tree(rng, 55))
        self.host_in["out_cols"] = (cols, rng.permutation(55)[:self.n_out].astype(np.int32))
        N = sum(self.LENS)
        self.out_spec = {"global_orient": ((N, 3), F64), "full_pose": ((N, 55, 3), F64), "joints": ((N, 55, 3), F64), "rest": ((3, 55, 3), F64)}

    def written(self, b, name):
        """Mask of the elements the call writes (None: all): of full_pose and joints only the named joints and their ancestors
        (the header: "the other joints' entries of full_pose / joints are left as they are")."""
        if name not in ("full_pose", "joints"):
            return None
        par, live = self.host_in["parents"][0], np.zeros(55, bool)
        for j in self.host_in["out_cols"][0]:
            while j >= 0 and not live[j]:
                live[j], j = True, par[j]
        return live[:, None]

    def new_struct(self):
        return (_native.SmplxBodyClip * 3)()

    def fill(self, st, b, decoy):
        for k, n in enumerate(self.LENS):
            e = st[k]
            for i, key in enumerate(("root_orient", "pose_body", "trans")):
                t = b.dev.get(f"{key}{k}")
                setattr(e, key, t.data_ptr() if t is not None else None)
                e.in_dtype[i] = _native.GMR_DTYPE_F32 if t is not None and t.dtype == F32 else _native.GMR_DTYPE_F64
            e.j_template, e.j_dirs, e.hand_mean = b.dev["j_template"].data_ptr(), b.dev["j_dirs"].data_ptr(), b.dev["hand_mean"].data_ptr()
            e.betas = b.host[f"betas{k}"].ctypes.data if self.NBETA[k] else None
            e.n_frames, e.n_betas, e.dirs_stride = n, self.NBETA[k], self.dirs_stride

    def invoke(self, b, st, stream):
        return _lib().gmr_smplx_body(H(b.host["parents"]), 55, st, 3, H(b.host["out_cols"]), self.n_out, P(b.out["global_orient"]), P(b.out["full_pose"]),
                                     P(b.out["joints"]), P(b.out["rest"]), stream)


CASES = {
    "gmr_ik_solve": lambda v: IKCase(v, "solve", False),
    "gmr_ik_plan_order": lambda v: IKCase(v, "plan", False),
    "gmr_ik_solve_ordered": lambda v: IKCase(v, "ordered", False),
    "gmr_group_ik_solve": lambda v: IKCase(v, "solve", True),
    "gmr_group_plan_order": lambda v: IKCase(v, "plan", True),
    "gmr_group_ik_solve_ordered": lambda v: IKCase(v, "ordered", True),
    "gmr_evaluate": case_evaluate,
    "gmr_fk": case_fk,
    "gmr_fk_shape": lambda v: case_fk(v, shape=True),
    "gmr_fk_min_height": lambda v: case_fk(v, min_height=True),
    "gmr_dof_to_rot": lambda v: case_kin(v, "gmr_dof_to_rot"),
    "gmr_rot_to_dof": lambda v: case_kin(v, "gmr_rot_to_dof"),
    "gmr_local_rot_to_global": lambda v: case_kin(v, "gmr_local_rot_to_global"),
    "gmr_motion_epilogue": lambda v: MotionCase(v, "epilogue", False),
    "gmr_group_motion_epilogue": lambda v: MotionCase(v, "epilogue", True),
    "gmr_motion_track": lambda v: MotionCase(v, "track", False),
    "gmr_group_motion_track": lambda v: MotionCase(v, "track", True),
    "gmr_motion_sample": SampleCase,
    "gmr_clip_report": lambda v: MotionCase(v, "report", False),
    "gmr_group_clip_report": lambda v: MotionCase(v, "report", True),
    "gmr_smplx_keypoints": lambda v: case_smplx(v, "gmr_smplx_keypoints"),
    "gmr_smplx_keypoints_cols": lambda v: case_smplx(v, "gmr_smplx_keypoints_cols"),
    "gmr_smplx_keypoints_in": lambda v: case_smplx(v, "gmr_smplx_keypoints_in"),
    "gmr_smplx_body": SmplxBodyCase,
    "gmr_bvh_fk": lambda v: case_bvh_fk(v, rows=False),
    "gmr_bvh_fk_rows": lambda v: case_bvh_fk(v, rows=True),
    "gmr_bvh_parse_motion_device": BvhParse,
}
ENTRIES = sorted(CASES)


def _large_table_case(v, n_seq=131072):
    """gmr_fk_min_height with 131072 clips of 0, 1, 2 and 1 frames: a pageable host table of 1 MiB, far beyond the few hundred bytes
    of the cases above, in case the runtime treats a large pageable copy differently (staging in pieces, pinning, blocking)."""
    true = np.concatenate([[0], np.cumsum(np.tile([0, 1, 2, 1], n_seq // 4))]).astype(np.int64)
    decoy = np.concatenate([[0], np.cumsum(np.tile([1, 2, 1, 0], n_seq // 4))]).astype(np.int64)
    return case_fk(v, min_height=True, offsets=(true, decoy))


CASES_LARGE = {"gmr_fk_min_height/1MiB_table": _large_table_case}


# ------------------------------------------------------------------ shared, computed once
@functools.lru_cache(maxsize=None)
def _calibration():
    return so.calibrate_spin()


@functools.lru_cache(maxsize=None)
def _prepared(entry, v):
    """(case, serial answers, spin in cycles, spin in ms) of variant v of an entry; the serial answers are checked here, once."""
    case = (CASES.get(entry) or CASES_LARGE[entry])(v)
    assert case.entry == entry.split("/")[0]
    ser = so.serial_answers(case, DEV())
    spin_ms = so.spin_ms_for(ser["ms"])
    return case, ser, int(spin_ms / _calibration()["ms_per_cycle"]), spin_ms


def _checked(entry, v):
    case, ser, cycles, spin_ms = _prepared(entry, v)
    assert ser["deterministic"], f"{entry}: two runs on the same inputs differ in {so.differing(ser['true'], ser['true2'])}"
    for k in ("dev_decoy", "host_decoy"):
        if k in ser:
            assert not so.same(ser[k], ser["true"]), f"{entry}: the {k} answer equals the true one: this case could not tell an ordering error"
    return case, ser, cycles, spin_ms


@pytest.mark.parametrize("entry", ENTRIES)
def test_late_producer(entry):
    """Issued behind a producer that is still running, with its host arrays overwritten on return, the call computes the serial
    true answer byte for byte; it returns before the producer finishes unless the header says it synchronises."""
    case, ser, cycles, spin_ms = _checked(entry, 0)
    r = so.run_late(case, DEV(), cycles)
    print(f"{entry}: serial {ser['ms']:.3f} ms, spin {spin_ms:.1f} ms, issue took {r['issue_ms']:.3f} ms, returned before producer: {r['returned_before_producer']}")
    assert not r["vacuous"], "the producer had finished before the call was issued: the run proves nothing"
    assert so.same(r["answer"], ser["true"]), f"differs from the serial answer in {so.differing(r['answer'], ser['true'])}"
    assert r["returned_before_producer"] == (entry not in SYNCHRONISES)


@pytest.mark.parametrize("entry", sorted(CASES_LARGE))
def test_late_producer_large_host_table(entry):
    """The same with a host table of 1 MiB: still read completely before the call returns.  The runtime does not stage a pageable
    copy of this size, though: the call waits until the earlier work on the stream has finished, which is what the header says of
    tables beyond the runtime's staging size (the sizes in between: profiles/stream_order.json)."""
    case, ser, cycles, spin_ms = _checked(entry, 0)
    r = so.run_late(case, DEV(), cycles)
    print(f"{entry}: serial {ser['ms']:.3f} ms, spin {spin_ms:.1f} ms, issue took {r['issue_ms']:.3f} ms, returned before producer: {r['returned_before_producer']}")
    assert not r["vacuous"], "the producer had finished before the call was issued: the run proves nothing"
    assert so.same(r["answer"], ser["true"]), f"differs from the serial answer in {so.differing(r['answer'], ser['true'])}"
    assert not r["returned_before_producer"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_off_stream_control(entry):
    """The harness can fail: issued on a stream that does not wait for the producer, the call sees the decoy device inputs."""
    case, ser, cycles, _ = _checked(entry, 0)
    r = so.run_late(case, DEV(), cycles, control=True)
    assert not r["vacuous"] and r["overtook_producer"], "the producer had finished before the control call did: the run shows nothing"
    assert so.same(r["answer"], ser["dev_decoy"]), f"differs from the decoy answer in {so.differing(r['answer'], ser['dev_decoy'])}"


@pytest.mark.parametrize("entry", ENTRIES)
def test_two_streams(entry):
    """Two cases of one handle on two streams, each behind its own late producer, issued A, B, A, B: each result is its own serial answer."""
    ca, sa, cyc_a, _ = _checked(entry, 0)
    cb, sb, cyc_b, _ = _checked(entry, 1)
    assert not so.same(sa["true"], sb["true"])
    cyc = 2 * max(cyc_a, cyc_b)   # four calls are issued behind the spins
    ans_a, ans_b, vacuous = so.run_two_streams(ca, cb, DEV(), cyc, cyc)
    assert not vacuous
    for r in range(2):
        assert so.same(ans_a[r], sa["true"]), f"A, call {r}: differs in {so.differing(ans_a[r], sa['true'])}"
        assert so.same(ans_b[r], sb["true"]), f"B, call {r}: differs in {so.differing(ans_b[r], sb['true'])}"


def main(path):
    entries, large = {}, {}
    for entry in ENTRIES + sorted(CASES_LARGE):
        case, ser, cycles, spin_ms = _prepared(entry, 0)
        rec = {"serial_ms": round(ser["ms"], 4), "spin_ms": round(spin_ms, 2), "launches": case.launches, "host_table_copies": case.h2d,
               "deterministic": bool(ser["deterministic"])}
        if ser["deterministic"]:
            r = so.run_late(case, DEV(), cycles)
            rec.update(returned_before_producer=bool(r["returned_before_producer"]), issue_ms=round(r["issue_ms"], 4), vacuous=bool(r["vacuous"]),
                       equals_serial=bool(so.same(r["answer"], ser["true"])),
                       decoys_differ=all(not so.same(ser[k], ser["true"]) for k in ("dev_decoy", "host_decoy") if k in ser))
        if ser["deterministic"] and entry in CASES:
            ctl = so.run_late(case, DEV(), cycles, control=True)
            rec["control_sees_decoy"] = bool(so.same(ctl["answer"], ser["dev_decoy"])) and not ctl["vacuous"] and bool(ctl["overtook_producer"])
            cb, sb, cyc_b, _ = _prepared(entry, 1)
            if sb["deterministic"]:
                cyc = 2 * max(cycles, cyc_b)
                ans_a, ans_b, vac = so.run_two_streams(case, cb, DEV(), cyc, cyc)
                rec["two_streams_equal_serial"] = all(so.same(a, ser["true"]) for a in ans_a) and all(so.same(b, sb["true"]) for b in ans_b) and not vac
        (large if entry in CASES_LARGE else entries)[entry] = rec
        print(entry, rec, flush=True)
    sweep = []   # where the runtime's treatment of a pageable copy changes: the same call with tables of 2 KiB .. 512 KiB
    for n_seq in (256, 1024, 2048, 4096, 8192, 16384, 32768, 65536):
        case = _large_table_case(0, n_seq)
        ser = so.serial_answers(case, DEV())
        r = so.run_late(case, DEV(), int(so.spin_ms_for(ser["ms"]) / _calibration()["ms_per_cycle"]))
        sweep.append({"table_bytes": 8 * (n_seq + 1), "returned_before_producer": bool(r["returned_before_producer"]), "issue_ms": round(r["issue_ms"], 4),
                      "equals_serial": bool(so.same(r["answer"], ser["true"])), "vacuous": bool(r["vacuous"])})
        print(sweep[-1], flush=True)
    so.write_profile(path, _calibration(), entries, large, sweep)


if __name__ == "__main__":
    main(sys.argv[1])

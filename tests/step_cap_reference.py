"""Reference for the per-solve step cap (``gmr_model_set_step_cap``): a helper, not a test.

The frame loop of the reference's ``retarget`` (motion_retarget.py:139-185) written out in Python on the pieces the CPU oracle
exports -- ``prepare_targets``, ``stage_error``, ``build_qp``, ``box_qp``, ``integrate`` -- with the one addition the feature
defines: between ``build_qp`` and ``box_qp`` the box is intersected with the cap, ``lo = max(lo, -cap)``, ``hi = min(hi, cap)``.
With a cap of ``+inf`` everywhere it is the oracle's own ``retarget_frame`` / ``ik_solve`` (tests/test_step_cap_host.py checks that
first); mink's ``VelocityLimit`` itself is not available to compare with, so the capped result is pinned by this definition.
"""
import dataclasses
from typing import List

import numpy as np

from oracle.oracle import IKParams, Oracle, box_qp


@dataclasses.dataclass
class CapResult:
    qpos: np.ndarray          # [N, nq]
    solves: np.ndarray        # [N] int32
    active: List[List[bool]]  # per frame, per solve: some dof ended on +-cap
    margins: np.ndarray       # |curr - next - tol| of every stopping decision that the error decrease (not max_iter) made

    def cap_active_solves(self) -> int:
        return sum(sum(f) for f in self.active)


def retarget_clips(cm, pos, quat, slot_col, seq_offsets, cap=None, params: IKParams = None, orc: Oracle = None) -> CapResult:
    """Every clip of ``seq_offsets`` from ``qpos0``, warm-started frame to frame.  ``pos [N, B, 3]`` / ``quat [N, B, 4]`` (float32 or
    float64: converted to float64 exactly as the kernel and the oracle do), ``cap [nv]`` or ``None`` (= no cap)."""
    orc = orc or Oracle(cm.blob)
    prm = params or IKParams()
    nv = orc.nv
    cap = np.full(nv, np.inf) if cap is None else np.asarray(cap, dtype=np.float64)
    assert cap.shape == (nv,)
    tables = [t for t, use in enumerate((cm.config.use_ik_match_table1, cm.config.use_ik_match_table2)) if use]
    ntask = [len(t) for t in cm.tasks]
    N = pos.shape[0]
    qout = np.full((N, orc.nq), np.nan)
    solves = np.zeros(N, dtype=np.int32)
    active: List[List[bool]] = [[] for _ in range(N)]
    margins = []
    slot_col = np.asarray(slot_col)
    for s in range(len(seq_offsets) - 1):
        q = np.array(cm.robot.qpos0, dtype=np.float64)
        for f in range(int(seq_offsets[s]), int(seq_offsets[s + 1])):
            tp, tq = orc.prepare_targets(pos[f][slot_col].astype(np.float64), quat[f][slot_col].astype(np.float64), prm.offset_to_ground)
            for tab in tables:
                curr, _ = orc.stage_error(tab, q, tp, tq, ntask[tab])
                num_iter, first = 0, True
                while True:
                    H, c, lo, hi = orc.build_qp(tab, q, tp, tq, prm)
                    lo, hi = np.maximum(lo, -cap), np.minimum(hi, cap)
                    dq, _ = box_qp(H, c, lo, hi)
                    active[f].append(bool(np.any(np.isfinite(cap) & (np.abs(dq) == cap))))
                    q = orc.integrate(q, dq)
                    solves[f] += 1
                    nxt, _ = orc.stage_error(tab, q, tp, tq, ntask[tab])
                    if not first:
                        num_iter += 1
                    first = False
                    if num_iter < prm.max_iter:
                        margins.append(abs(curr - nxt - prm.tol))
                    if not (curr - nxt > prm.tol and num_iter < prm.max_iter):
                        break
                    curr = nxt
            qout[f] = q
    return CapResult(qout, solves, active, np.asarray(margins))

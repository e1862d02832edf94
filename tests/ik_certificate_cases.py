"""The cases the IK certificate is applied to, shared by the host tests (solver = the CPU oracle) and the GPU tests (solver =
the HIP kernel): inputs, solver constants, the certified quantities and the deliberately wrong models of the negative controls.
Nothing here calls a solver."""
import dataclasses
import os

import numpy as np

from gmr_amd import params, synth
from gmr_amd.ik_config import IKConfig, IKTask, load_ik_config
from gmr_amd.mjcf import load_mjcf, load_robot
from gmr_amd.model import compile_model
from tests.ik_certificate import IKCertificate
from tests.util import CONFIG_ROBOTS

REACHABLE_ROBOTS = CONFIG_ROBOTS + ["kuavo_s45", "hightorque_hi", "booster_k1", "galaxea_r1pro"]

# tol: the solver stops a stage when the unweighted error falls by less than tol; a large negative value makes every stage run
# exactly 1 + max_iter solves, so the last stage of a frame is one long iteration on its own table alone.
RUN_ALL = -1e30


@dataclasses.dataclass
class Case:
    name: str
    robot: object          # gmr_amd.mjcf.RobotModel
    config: IKConfig
    height: object         # actual human height or None
    cm: object             # compile_model(robot, config, height): what a solver is given -- the certificate never sees it
    names: list            # human body names of the input columns
    pos: np.ndarray        # [n_clips, B, 3] one held frame per clip
    quat: np.ndarray       # [n_clips, B, 4]
    hold: int              # frames each clip holds its frame for
    solver: dict           # constants of the solve (max_iter, tol)
    tables: list           # tables certified at the final qpos

    def cert(self):
        return IKCertificate(self.robot, self.config, self.height)

    def held_input(self):
        """(pos [n_clips * hold, B, 3], quat, seq_offsets): every clip its one frame, repeated."""
        n = self.pos.shape[0]
        return np.repeat(self.pos, self.hold, axis=0), np.repeat(self.quat, self.hold, axis=0), np.arange(n + 1, dtype=np.int64) * self.hold

    def final_rows(self):
        return (np.arange(self.pos.shape[0]) + 1) * self.hold - 1


def _registry(src, robot):
    return load_robot(params.ROBOT_XML_DICT[robot], name=robot), load_ik_config(params.IK_CONFIG_DICT[src][robot])


# Seeds 4 and 14 of the easy generator: the first two (of 1..40) from which the oracle reaches the global minimum on all ten
# robots; from some others a robot settles in a local minimum of the reachable problem (stationary, cost ratio 1e-5 .. 1e-1),
# which is a property of the iteration the reference runs, not what case (a) is about.
REACHABLE_SEEDS = (4, 14)


def reachable_case(robot_name, hold=40, solver=None):
    """(a): the targets are the FK of an in-limit qpos (synth.synth_clips(hard=False), float32 key-points: reachable to the
    rounding of the inputs), so every table's cost has its minimum, ~0, at the same qpos.  The last frame of two 12-frame clips,
    each held from qpos0."""
    robot, config = _registry("smplx", robot_name)
    cm = compile_model(robot, config)
    P, Q = [], []
    for seed in REACHABLE_SEEDS:
        pos, quat, names, _, _ = synth.synth_clips(cm, 1, 12, seed=seed, hard=False, dtype=np.float32)
        P.append(pos[-1])
        Q.append(quat[-1])
    tables = [k for k, on in enumerate((config.use_ik_match_table1, config.use_ik_match_table2)) if on]
    return Case(f"reachable-{robot_name}", robot, config, None, cm, names, np.stack(P), np.stack(Q), hold,
                solver or dict(max_iter=50, tol=RUN_ALL), tables)


PAIR_ROBOTS = ("unitree_g1", "unitree_g1_with_hands")


def pair_case(robot_name):
    """(a) for the two robots MultiRobotRetargeting.retarget_batch is certified with: unitree_g1's reachable clips (the robot with
    hands reads unitree_g1's config: the same tasks on the same bodies, the hand hinges without any), the caller's constants."""
    case = reachable_case("unitree_g1", hold=PAIR_HOLD, solver=dict(max_iter=10, tol=1e-3))
    if robot_name != "unitree_g1":
        robot, config = _registry("smplx", robot_name)
        case = dataclasses.replace(case, name=f"reachable-{robot_name}", robot=robot, config=config, cm=compile_model(robot, config))
    return dataclasses.replace(case, name=case.name + "-default-constants")


PAIR_HOLD = 200


def held_reference_frame_case(golden_dir):
    """(b) 1: fbx_to_g1 at 1.75 m on the one IK input frame the reference holds (tests/test_oracle.py::_dumped_frame): far,
    unreachable targets, joint limits active.  Its two tables map the same frames to the same human bodies in the same order
    but do NOT carry the same weights (table 1: 0 / 10 on eleven tasks where table 2 has 10 / 5), so the alternation of the
    stages is not one continued iteration; what is stationary is the last stage's table at the end of a stage that ran long
    enough by itself -- hence few frames and a very large max_iter."""
    import json
    robot, config = _registry("fbx", "unitree_g1")
    cm = compile_model(robot, config, 1.75)
    with open(os.path.join(golden_dir, "ref_fixtures", "first_frame_debug.json")) as f:
        d = json.load(f)
    names = list(cm.slot_names)
    pos = np.array([[d[s]["pos"] for s in names]], dtype=np.float64)
    quat = np.array([[d[s]["quat_wxyz"] for s in names]], dtype=np.float64)
    return Case("held-reference-frame", robot, config, 1.75, cm, names, pos, quat, HELD_FRAME_HOLD, dict(max_iter=HELD_FRAME_MAX_ITER, tol=RUN_ALL), [1])


HELD_FRAME_HOLD, HELD_FRAME_MAX_ITER = 3, 3000


def synthetic_limits_case(tmp_path):
    """(b) 2: the synthetic robot of tests/test_gpu_parity.py::_synthetic_robot (a floating base, four chains of 5 / 5 / 4 / 4
    hinges about alternating axes, a task on every second link) with a narrow joint range and two IDENTICAL tables, so that
    the alternating stages are one continued iteration; the rotation weights differ from task to task.  Targets: the hard
    generator's (noise and over-reach: unreachable), one frame held."""
    limbs, every, jrange = [5, 5, 4, 4], 2, "-0.25 0.3"
    axes = ["1 0 0", "0 1 0", "0 0 1"]
    xml = ['<mujoco model="synth"><compiler angle="radian"/><worldbody><body name="base" pos="0 0 1"><freejoint/>']
    tasks = [("base", "h_base")]
    for li, n in enumerate(limbs):
        ang = 2 * np.pi * li / len(limbs)
        for k in range(n):
            pos = f"{0.15 * np.cos(ang):.4f} {0.15 * np.sin(ang):.4f} 0" if k == 0 else "0.02 0.01 -0.12"
            xml.append(f'<body name="l{li}_{k}" pos="{pos}"><joint name="j{li}_{k}" axis="{axes[(k + li) % 3]}" range="{jrange}"/>')
            if (k + 1) % every == 0 or k == n - 1:
                tasks.append((f"l{li}_{k}", f"h{li}_{k}"))
        xml.append("</body>" * n)
    xml.append("</body></worldbody></mujoco>")
    p = tmp_path / "synth_limits.xml"
    p.write_text("".join(xml))
    robot = load_mjcf(str(p))
    t1 = [IKTask(f, h, 0.0 if i % 3 else 50.0, (10.0, 6.0, 8.0)[i % 3], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]) for i, (f, h) in enumerate(tasks)]
    config = IKConfig("base", "h_base", 0.0, 1.8, True, True, {h: 1.0 for _, h in tasks}, t1, [dataclasses.replace(t) for t in t1], source="synthetic")
    cm = compile_model(robot, config)
    # the generator draws a trajectory inside the narrow range; the targets it derives are asked of a robot that cannot follow
    # them: amp 0.6 puts the trajectory at the range's edge, the hard variant's noise and over-reach beyond it
    pos, quat, names, _, _ = synth.synth_clips(cm, 1, 12, seed=SYNTHETIC_SEED, hard=True, dtype=np.float64, amp=0.6)
    return Case("synthetic-limits", robot, config, None, cm, names, pos[-1:], quat[-1:], SYNTHETIC_HOLD, dict(max_iter=SYNTHETIC_MAX_ITER, tol=RUN_ALL), [1])


SYNTHETIC_SEED, SYNTHETIC_HOLD, SYNTHETIC_MAX_ITER = 9, 3, 3000


# ------------------------------------------------------------------ what is certified
def certify(case, q_final, cert=None):
    """-> dict per certified table k: 'stat[k]' = worst over the clips of |projected gradient(q_final)|_inf / |gradient(qpos0)|_inf,
    'cost[k]' = worst cost(q_final) / cost(qpos0); plus 'active' = joint limits active over the clips' final qpos."""
    cert = cert or case.cert()
    q0 = case.robot.qpos0
    out = {"active": 0}
    for c in range(case.pos.shape[0]):
        targets = cert.prepare_targets(case.pos[c], case.quat[c], case.names)
        for k in case.tables:
            out[f"stat{k}"] = max(out.get(f"stat{k}", 0.0), cert.stationarity(k, q_final[c], q0, targets))
            out[f"cost{k}"] = max(out.get(f"cost{k}", 0.0), float(cert.cost(k, q_final[c], targets) / cert.cost(k, q0, targets)))
        state, feasible = cert.bound_state(q_final[c])
        out["active"] += int(np.count_nonzero(state)) if feasible else 0
    return out


# ------------------------------------------------------------------ negative controls: the certificate of a model that is wrong on purpose
def _tasked_hinge(case, q_final):
    """The hinge on the path from a task of the certified table to the root that is turned furthest at q_final."""
    r, cert = case.robot, case.cert()
    on_path = set()
    for b, _, _, _ in cert.tables[case.tables[-1]]:
        while b > 0:
            on_path.add(b)
            b = int(r.parent[b])
    hinges = [b for b in sorted(on_path) if r.jnt_type[b] == 1]
    return max(hinges, key=lambda b: abs(q_final[int(r.qpos_adr[b])]))


def wrong_axis(case, q_final):
    """One hinge axis negated."""
    b = _tasked_hinge(case, q_final)
    axis = case.robot.jnt_axis.copy()
    axis[b] = -axis[b]
    return IKCertificate(dataclasses.replace(case.robot, jnt_axis=axis), case.config, case.height)


def wrong_offset(case, q_final):
    """The position offset of one task (the last of the certified table that weighs position) shifted by 2 cm."""
    k = case.tables[-1]
    tab = (case.config.table1, case.config.table2)[k]
    human = [t.human for t in tab if t.pos_weight != 0][-1]
    t1 = [dataclasses.replace(t, pos_offset=[t.pos_offset[0] + 0.02, t.pos_offset[1], t.pos_offset[2]]) if t.human == human else t
          for t in case.config.table1]
    return IKCertificate(case.robot, dataclasses.replace(case.config, table1=t1), case.height)


def wrong_weight(case, q_final):
    """One task's w_r taken from the other table's neighbouring task (the first task for which that is another number)."""
    k = case.tables[-1]
    tabs = [list(case.config.table1), list(case.config.table2)]
    for i in range(len(tabs[k]) - 1):
        other = tabs[1 - k][i + 1].rot_weight
        if other != tabs[k][i].rot_weight and other != 0 and tabs[k][i].rot_weight != 0:
            tabs[k][i] = dataclasses.replace(tabs[k][i], rot_weight=other)
            return IKCertificate(case.robot, dataclasses.replace(case.config, table1=tabs[0], table2=tabs[1]), case.height)
    raise AssertionError("no task whose neighbour in the other table has another w_r")


def wrong_range(case, q_final):
    """One joint range shrunk so that it excludes q_final."""
    r = case.robot
    b = _tasked_hinge(case, q_final)
    q = float(q_final[int(r.qpos_adr[b])])
    rng, limited = r.jnt_range.copy(), r.jnt_limited.copy()
    rng[b] = (q + 0.01, max(q + 0.02, rng[b, 1])) if q <= 0 else (min(q - 0.02, rng[b, 0]), q - 0.01)
    limited[b] = True
    return IKCertificate(dataclasses.replace(r, jnt_range=rng, jnt_limited=limited), case.config, case.height)

// dev_model.h -- what the host's model planning (model_plan.h) and the kernels share: the compiled model as the IK kernels see it
// (DevModel, LdsLayout), the shapes a kernel instance can have compiled in, the FK / kin-ops table structs and the constants that
// size any of them.
//
// Declarations only, no HIP runtime call: it compiles under hipcc and under a plain host compiler (with -D__HIP_PLATFORM_AMD__ and
// the ROCm include directory, for the uint2 / uint4 of <hip/hip_vector_types.h>).  The kernels that read these structs live in
// ik_kernel.hip.h, fk_kernel.hip.h and kin_ops_kernel.hip.h.
#pragma once

#include <hip/hip_vector_types.h>
#include <stdint.h>

#include "../../include/gmr_amd.h"

namespace gmr {

typedef unsigned long long u64;

#ifndef GMR_IK_STAGE_TREE
#define GMR_IK_STAGE_TREE 1  // joint tree staged in LDS per wavefront; 0 = re-read from L2 (saves 3.3 KB LDS for G1)
#endif

// Doubles per task / composite block: LL(6) LA(9) AA(6) g(6) = 27 used, the block sums move 28 (14 lanes x 16 bytes), and the
// stride is 30 = 15 sixteen-byte slots, odd, so that the blocks of different composites start on different LDS slots: the F
// phase (every dof lane reads element c of ITS composite) then has no bank conflicts (stride 28 = 14 slots: 91 extra LDS
// cycles per solve on G1).  Stored "by column": element 3k + s, s = 0..2,
// (Round 2's mixed-precision variant -- this assembly in float32: -0.5 % time, 5.4e-5 rad -- lives in the history up to commit d74eaa7,
// profiles/experiment_log_r01_r02.md, round-2 item 7.)
constexpr int kBT = 30, kBTLanes = 14;
constexpr int kHPlanRegsSQ = 6;  // rounds of the H pair plan held in registers (even); structured back end only -- the generic one has no registers to spare
constexpr int kCompRegsSQ = 3;   // passes of the composite plan whose addresses stay in registers for a whole stage (ditto)
constexpr int kMaxCompPass = 32;  // passes of the composite plan (two composites per pass, children before parents)
constexpr int kBodyC = 11;  // doubles per body in the LDS-staged joint tree: pos(3) quat(4) axis(3) {fkanc(6 bytes), jtype, qadr}

// A compiled model as the kernels see it: ONE struct of fixed-capacity arrays in device memory (filled by model_plan.h), reached
// through a single kernel-argument pointer.  Every table is base + compile-time offset, so the model costs two SGPRs instead
// of two per table (with ~45 tables passed by value the kernel spilled hundreds of SGPRs into VGPR lanes).
constexpr int kMaxPairsPadded = (GMR_MAX_BODIES * (GMR_MAX_BODIES - 1) / 2 + 127) / 128 * 128;
struct DevModel {
  // root_tslot: slot whose prepared target the root body tracks (-1 = none); same_tasks: both tables used, same (body, slot) per task
  int nbody, nq, nv, nslot, root_slot, n_act, root_tslot, same_tasks;
  int ntask[2], use_table[2], ncomp[2], ncpass[2];  // ncpass: composite passes per table
  int npairp, fkrounds, sq_ok, sq_nlimb;              // npairp: entries of hplan (a multiple of 128)
  int root_planar, pad_[3];                           // 1: planar base (gmr_blob.h root_dof_mask 0x23): rows 2-4 of the QP are null dofs (akind 7)
  // per active dof [64]
  int abody[64], akind[64], aqadr[64], alimited[64];  // akind: 0..2 root translation, 3..5 root rotation, 6 hinge, 7 null (a root
                                                      // dof the model lacks: takes the hinge path with the root's zero axis)
  double arange[128];                                 // [64][2]
  int acomp[2 * 64];                                  // composite node of the dof per table
  // per task, table-major [2][GMR_MAX_TASKS]
  int tbody[2 * GMR_MAX_TASKS], tslot[2 * GMR_MAX_TASKS];
  double twp[2 * GMR_MAX_TASKS], twr[2 * GMR_MAX_TASKS];
  // per body [nbody]
  int jtype[GMR_MAX_BODIES], qadr[GMR_MAX_BODIES];
  double bpos[3 * GMR_MAX_BODIES], bquat[4 * GMR_MAX_BODIES], axis[3 * GMR_MAX_BODIES];  // bquat: unit wxyz
  u64 fkanc[GMR_MAX_BODIES];                          // byte r = ancestor folded in FK round r (0xff: none)
  double qpos0[GMR_MAX_BODIES + 8];                   // [nq]
  // per slot [nslot]
  double sscale[GMR_MAX_SLOTS], spoff[3 * GMR_MAX_SLOTS], sroff[4 * GMR_MAX_SLOTS];
  int sfoot[GMR_MAX_SLOTS];
  // structured QP (box_qp_struct): 4 groups of 16 lanes, each = one bin of limb dofs + a copy of the core dofs
  signed char sq_gdof[64], sq_owner[64];              // dof of a structured lane (-1 padding); 1 if the lane owns that dof
  int sq_lane_of_dof[64], sq_diag[64];                // per dof: its owner lane; LDS index of its diagonal entry
  // H assembly plan, one entry per structurally non-zero off-diagonal pair (dof j strictly above dof i), padded to a multiple
  // of 64 with entries that land in the dummy slots: LDS byte offsets {S_j | F_i << 16, H[i][j] | H[j][i] << 16}
  uint2 hplan[kMaxPairsPadded];
  // composite plan per table, pass and quarter-wave: LDS byte offsets of four source blocks and the destination block
  // {s0|s1<<16, s2|s3<<16, dst, -}; absent sources point at the zero block, an idle quarter at a scratch block
  uint4 comp_plan[2 * kMaxCompPass * 4];
};

struct LdsLayout {
  // offsets in doubles.  zero: block of zeros; hplan / cplan: the staged H-pair and composite plans; Lb (generic QP broadcast
  // rows) aliases S; Bc aliases the poses; H aliases [B | poses / Bc] (all dead during the QP)
  int zero, hplan, cplan, q, tp, tq, S, F, Lb, bodyc, xpos, xquat, B, Bc, H, total_doubles;
  // tring: the ring of kTargetBlockFrames target images [tp | tq] of a model that matches a plain shape (target_blocks.h), else -1
  int tring;
};

// The shape of a (model, call): everything ik_body reads from DevModel / IkLaunch / the work item that is wave-uniform and never
// changes for a given model and calling mode.  A shape is a struct of static constexpr ints, one per field below, -1 = "read it at
// run time"; IkShapeAny (all -1) is the generic instance that serves every model, the group kernels and the session kernel.  A
// shaped instance is only ever launched for a model and a launch the host has matched field by field (model_plan.h, ik_shape_of): the
// kernel does not re-check.  X(field, the value in a host DevModel d).
#define GMR_IK_SHAPE_FIELDS(X)                                                                                                   \
  X(nlimb, d.sq_nlimb) X(ntask0, d.ntask[0]) X(ntask1, d.ntask[1]) X(use0, d.use_table[0]) X(use1, d.use_table[1])              \
  X(same_tasks, d.same_tasks) X(ncpass0, d.ncpass[0]) X(ncpass1, d.ncpass[1]) X(npairp, d.npairp) X(nbody, d.nbody)              \
  X(fkrounds, d.fkrounds) X(n_act, d.n_act) X(nslot, d.nslot) X(nq, d.nq) X(root_slot, d.root_slot)
// plain (a property of the launch, not of the model): 1 = float32 key-points, no offset_to_ground, no item with a verification walk
// (check_stride) or a speculative chunk start (GMR_INIT_ROOT_TARGET), no step cap (IkLaunch::step_cap)
struct IkShapeAny {
#define GMR_X(f, e) static constexpr int f = -1;
  GMR_IK_SHAPE_FIELDS(GMR_X)
#undef GMR_X
  static constexpr int plain = -1;
  static constexpr int stage_shared = -1;
};
// unitree_g1 with the smplx config (and whatever else packs to the same counts) in the plain batched call
struct IkShapeG1Smplx {
  static constexpr int nlimb = 7, ntask0 = 14, ntask1 = 14, use0 = 1, use1 = 1, same_tasks = 1, ncpass0 = 3, ncpass1 = 3, npairp = 384,
                       nbody = 32, fkrounds = 4, n_act = 35, nslot = 14, nq = 36, root_slot = 0;
  // plain is compiled in: the host only sends plain launches here (api.hip, ik_launch_shape), and the target preparation -- the one
  // block whose contraction used to depend on the float64 / offset_to_ground / walk paths around it -- is pinned (target_prep_slot)
  static constexpr int plain = 1;
  // the two task tables differ in their weights only (model_plan.h, stage_tables_shared): a property of the model beside the fields
  // above, matched by ik_shape_matches.  The instance then reads the tables once per work item instead of once per stage.
  static constexpr int stage_shared = 1;
};

// ---- forward kinematics in the KinematicsModel convention (fk_kernel.hip.h) ----
constexpr int kFkThreads = 128;
#ifndef GMR_FK_GROUP
#define GMR_FK_GROUP 8
#endif
constexpr int kFkGroup = GMR_FK_GROUP;             // bodies per output flush
constexpr int kFkPosStride = 3 * kFkGroup + 1;    // LDS words per lane of the position stage (odd: conflict-free)
constexpr int kFkRotStride = 4 * kFkGroup + 1;
constexpr int kFkMaxSlots = 12;

// Everything the chain needs about one body, in one 80-byte record: read with two scalar loads (s_load_dwordx16 + x4) and
// fetched one body ahead of its use, instead of a dozen dependent scalar loads per body in front of the wave-uniform branches.
struct FkBody {
  int src_slot, dofidx, save_slot, pad0;  // src_slot: -1 = the previous body is the parent; dofidx: -1 = no hinge
  float lpos[3], pad1;                    // local translation
  float lrot[4];                          // local rotation xyzw, raw XML values (not normalised)
  double axis[3], pad2;                   // unit hinge axis in float64 (torch promotes the hinge quaternion to float64)
};
static_assert(sizeof(FkBody) == 80, "FkBody layout");

struct FkTree {     // device arrays, [nbody]
  const int *parent, *dofidx, *src_slot, *save_slot;  // dofidx: -1 if no hinge; src_slot: -1 = previous body
  const float *lpos;   // [nb][3] local translation
  const float *lrot;   // [nb][4] local rotation xyzw, raw XML values (not normalised)
  const float *jaxis;  // [nb][3] hinge axis, unit (double normalised, then rounded)
  const double *jaxis64;  // [nb][3] unit axis in float64 (torch promotes the hinge quaternion to float64)
  const FkBody *body;     // [nb] the same, one record per body (what the kernels read)
  int nbody, ndof, nslots, dof_in_order;  // dof_in_order: dofidx never decreases along the bodies (the register window needs it)
};

// ---- the rest of the KinematicsModel operator surface (kin_ops_kernel.hip.h) ----
struct KinTables {            // device arrays
  const int *dof_body;        // [ndof] body that owns hinge d
  const float *lim_lo, *lim_hi;  // [ndof] float32 of the XML range (KinematicsModel._dof_lower_limits / _dof_upper_limits)
  const uint8_t *depth;       // [nb] tree level of body j (0 for the root)
  const uint8_t *order;       // [nb] bodies sorted by level (stable)
  int max_depth;
};

}  // namespace gmr

// model_plan.h -- from a model blob (gmr_blob.h) to everything the kernels want of a model: the pruned IK tree, the active dofs in
// elimination order, the FK pointer-jumping plans, the core-plus-limbs partition of the structured QP, the composites and their pass
// schedule, the LDS layout, the H pair plan, the FK branch slots, the kin-ops and clip-report tables, and the model image that holds
// all of it (call_block.h).
//
// Host only, C++17, no HIP runtime call: plan_model() is a pure function of (blob, min_nvp, force_generic), so a stand-alone program
// can plan every registry model under the sanitizers and check what the kernels assume of the tables (tests/test_model_plan_host.py).
// api.hip allocates the image's bytes on the device, resolves the handles and copies (build_device_model).
//
// One function per stage, in the order plan_model() runs them; what passes between them are the small structs of PlanStages.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <numeric>
#include <string>
#include <type_traits>
#include <vector>

#include "call_block.h"
#include "dev_model.h"
#include "target_blocks.h"

namespace gmr {

// Kernel variants by padded system size.  GMR_IK_DEV_ONLY36 (experiments only, never the shipped library) builds just
// ik_kernel<36, true> to cut compile time.
#ifdef GMR_IK_DEV_ONLY36
#define GMR_FOR_EACH_NVP(X) X(36)
#else
#define GMR_FOR_EACH_NVP(X) X(32) X(36) X(40) X(48) X(64)
#endif

// Shaped kernel instances (dev_model.h, IkShapeAny): X(struct, NVP).  Each entry costs one more ik_kernel and ik_probe_kernel
// instance at compile time; a model that matches none runs the generic instance.  The structs are defined beside IkShapeAny.
#define GMR_FOR_EACH_IK_SHAPE(X) X(IkShapeG1Smplx, 36)

// Do the two task tables of a model differ in their weights (twp, twr) only?  Both used on the same (body, slot) per task, the same
// composite per active dof and the same composite plan, entry for entry: everything else a stage of ik_body reads of its table.
inline bool stage_tables_shared(const DevModel &d) {
  if (!d.use_table[0] || !d.use_table[1] || !d.same_tasks) return false;
  if (d.ntask[0] != d.ntask[1] || d.ncpass[0] != d.ncpass[1]) return false;
  for (int t = 0; t < d.ntask[0]; ++t)
    if (d.tbody[t] != d.tbody[GMR_MAX_TASKS + t] || d.tslot[t] != d.tslot[GMR_MAX_TASKS + t]) return false;
  for (int i = 0; i < d.n_act; ++i)
    if (d.acomp[i] != d.acomp[64 + i]) return false;
  for (int i = 0; i < 4 * d.ncpass[0]; ++i) {
    const uint4 &a = d.comp_plan[i], &b = d.comp_plan[4 * kMaxCompPass + i];
    if (a.x != b.x || a.y != b.y || a.z != b.z || a.w != b.w) return false;
  }
  return true;
}

// Does the host copy of a model carry exactly the values the shape SH fixes, and the properties it assumes?  (SH::plain is the
// launch's side: launch_ik.)
template <class SH>
inline bool ik_shape_matches(const DevModel &d) {
#define GMR_X(f, e) if (SH::f >= 0 && SH::f != (e)) return false;
  GMR_IK_SHAPE_FIELDS(GMR_X)
#undef GMR_X
  return SH::stage_shared <= 0 || stage_tables_shared(d);
}
// The shape (index into GMR_FOR_EACH_IK_SHAPE) of a model built for kernel variant nvp with the structured QP, or -1.
inline int ik_shape_of(const DevModel &d, int nvp, bool sq) {
  int idx = 0;
#define GMR_X(S, v) if (sq && nvp == v && ik_shape_matches<S>(d)) return idx; ++idx;
  GMR_FOR_EACH_IK_SHAPE(GMR_X)
#undef GMR_X
  return -1;
}
// Is `plain` compiled into the shape (its instances take only plain launches and prepare targets in blocks)?
inline bool ik_shape_is_plain(int shape) {
  int idx = 0;
#define GMR_X(S, v) if (shape == idx++) return S::plain > 0;
  GMR_FOR_EACH_IK_SHAPE(GMR_X)
#undef GMR_X
  return false;
}
inline const char *ik_shape_name(int shape) {
  int idx = 0;
#define GMR_X(S, v) if (shape == idx++) return #S;
  GMR_FOR_EACH_IK_SHAPE(GMR_X)
#undef GMR_X
  return "generic";
}

inline int pick_nvp(int n_act) {
#define GMR_X(v) if (n_act <= v) return v;
  GMR_FOR_EACH_NVP(GMR_X)
#undef GMR_X
  return -1;
}

// ------------------------------------------------------------------------------------------------ what plan_model() returns
// The model image: one block of device memory, every table by its typed handle (offsets until the block has an address).  Every
// array holds at least one element, so that no two tables share an address.
struct ModelImage {
  CallBlock block;
  CallBlock::Uploaded<DevModel> dm, dm_eval;  // the IK model (pruned tree) and the same with the full body tree (gmr_evaluate)
  CallBlock::Uploaded<int> parent, dofidx, src_slot, save_slot;
  CallBlock::Uploaded<float> lpos, lrot, jaxis;
  CallBlock::Uploaded<double> jaxis64;
  CallBlock::Uploaded<FkBody> fkbody;
  CallBlock::Uploaded<int> k_dof_body;
  CallBlock::Uploaded<float> k_lo, k_hi;
  CallBlock::Uploaded<uint8_t> k_depth, k_order;
  CallBlock::Uploaded<double> rep_lo, rep_hi;  // [nq - 7]: hinge limits in qpos order, -inf / +inf where unlimited (gmr_clip_report)
};

struct ModelPlan {
  DevModel dm, dm_eval;
  LdsLayout lay, lay_eval;
  int lds_bytes = 0, lds_bytes_eval = 0;
  int nvp = 0, n_act = 0;
  int shape = -1;                                // index into GMR_FOR_EACH_IK_SHAPE of the shape the model matches, -1 = none
  int fk_lds_bytes = 0, fk_lds_bytes_min = 0;    // _min: the min-height mode has no output stage
  int nslots = 0, dof_in_order = 0, k_maxd = 0;  // FkTree::nslots, FkTree::dof_in_order, KinTables::max_depth
  ModelImage image;
};

// ------------------------------------------------------------------------------------------------ what passes between the stages
// The blob's arrays.  `store` is the plan's own 8-byte aligned copy of the blob: every pointer points into it.
struct BlobView {
  std::vector<uint64_t> store;
  gmr_blob_header h;
  const int32_t *parent, *jtype, *qadr, *dadr, *limited;
  const double *bpos, *bquat, *bquat_raw, *axis, *range, *qpos0;
  const double *sscale, *spoff, *sroff;
  const int32_t *sfoot;
  const int32_t *tbody[2], *tslot[2];
  const double *twp[2], *twr[2];
  // body a is an ancestor-or-self of body b ?
  bool above(int a, int b) const {
    while (b > a) b = parent[b];
    return b == a;
  }
};
struct TaskTables {  // table-major [2][GMR_MAX_TASKS]
  std::vector<int> body, slot;
  std::vector<double> wp, wr;
};
struct PrunedTree {
  std::vector<int> keep, bmap;  // IK body -> body; body -> IK body or -1
  int nb_ik = 0;
};
struct ActiveDofs {  // per active dof; in depth-first order until elimination_order() permutes them
  std::vector<int> body, kind, qadr, lim, height;
  std::vector<double> range;
  int n_act = 0, nvp = 0, root_mask = 0x3F;
};
struct DofOrder {
  std::vector<u64> aanc;                // [64] bit b of aanc[a]: dof b is above dof a (both in elimination order, b < a)
  std::vector<unsigned short> hpair;    // structurally non-zero off-diagonal pairs of H: (i << 8) | j with dof j strictly above dof i
};
struct FkJumpPlan {
  std::vector<u64> anc;  // byte r = ancestor folded in round r (0xff: none)
  int rounds = 0;
};
struct StructuredQp {
  std::vector<signed char> gdof, owner;
  std::vector<int> lane_of_dof, diag;
  std::vector<unsigned> dst;  // per pair of DofOrder::hpair: the two entries of H it fills
  int ok = 0, nlimb = 0;
};
struct Composites {
  std::vector<int> acomp;                 // [2][64] composite of a dof; after composite_passes(): its block index from Bt on
  std::vector<unsigned> mask, own, kids;  // task mask [2][2 GMR_MAX_TASKS]; own tasks and child composites [2][32]
  int ncomp[2] = {0, 0};
};
struct CompositePasses {
  std::vector<uint32_t> plan;
  int ncpass[2] = {0, 0};
};
struct FkSlots {
  std::vector<int> dofidx, src_slot, save_slot;
  std::vector<float> lpos, lrot, jaxis;
  std::vector<double> jaxis64;
  int nslots = 0;
};
struct KinReport {
  std::vector<int> dof_body;
  std::vector<float> lo, hi;
  std::vector<uint8_t> depth, order;
  std::vector<double> rep_lo, rep_hi;
  int maxd = 0;
};
// Everything plan_model() derives on the way (a test reads the intermediate tables here).
struct PlanStages {
  BlobView blob;
  TaskTables tasks;
  PrunedTree tree;
  ActiveDofs act;
  DofOrder order;
  FkJumpPlan fk_ik, fk_full;
  StructuredQp sq;
  Composites comp;
  CompositePasses passes;
  std::vector<uint32_t> hplan_pairs, hplan;  // the H pair plan in pair order (padded), and in the order the lanes execute it
  FkSlots slots;
  KinReport kin;
  bool use_sq = false;  // the structured QP applies and is not overridden (force_generic)
};

namespace plan_detail {

#if defined(__GNUC__)
__attribute__((format(printf, 3, 4)))
#endif
inline int fail(std::string &msg, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  msg = buf;
  return code;
}

inline int even(int x) { return (x + 1) & ~1; }

inline bool range_ok(const gmr_blob_header &h, uint32_t off, size_t bytes) {
  return off >= sizeof(gmr_blob_header) && (off & 7u) == 0 && (size_t)off + bytes <= h.total_bytes;
}

}  // namespace plan_detail

// ------------------------------------------------------------------------------------------------ blob validation
// The header and every array inside the blob.  The only stage that reads `blob` itself; it fills `h`.
inline int validate_blob(const void *blob, size_t blob_bytes, gmr_blob_header &h, std::string &msg) {
  using plan_detail::fail;
  using plan_detail::range_ok;
  if (!blob || blob_bytes < sizeof(gmr_blob_header)) return fail(msg, GMR_EINVAL, "blob too small");
  memcpy(&h, blob, sizeof(h));
  if (h.magic != GMR_BLOB_MAGIC || h.version != GMR_BLOB_VERSION) return fail(msg, GMR_EINVAL, "bad blob magic/version");
  if (h.total_bytes != blob_bytes) return fail(msg, GMR_EINVAL, "blob size mismatch");
  if (h.nbody < 1 || h.nbody > GMR_MAX_BODIES) return fail(msg, GMR_EINVAL, "nbody outside [1, 64]");
  if (h.nq != h.nv + 1 || h.nv < 6) return fail(msg, GMR_EINVAL, "bad nq/nv");
  if (h.nslot < 0 || h.nslot > GMR_MAX_SLOTS || h.ntask[0] < 0 || h.ntask[0] > GMR_MAX_TASKS || h.ntask[1] < 0 || h.ntask[1] > GMR_MAX_TASKS)
    return fail(msg, GMR_EINVAL, "slot/task counts out of range");
  if (h.nslot > 0 && (h.root_slot < 0 || h.root_slot >= h.nslot)) return fail(msg, GMR_EINVAL, "root_slot out of range");
  const size_t nb = h.nbody, ns = h.nslot;
  bool ok = range_ok(h, h.off_parent, nb * 4) && range_ok(h, h.off_jnt_type, nb * 4) && range_ok(h, h.off_qpos_adr, nb * 4) &&
            range_ok(h, h.off_dof_adr, nb * 4) && range_ok(h, h.off_jnt_limited, nb * 4) && range_ok(h, h.off_body_pos, nb * 24) &&
            range_ok(h, h.off_body_quat, nb * 32) && range_ok(h, h.off_body_quat_raw, nb * 32) && range_ok(h, h.off_jnt_axis, nb * 24) &&
            range_ok(h, h.off_jnt_range, nb * 16) && range_ok(h, h.off_qpos0, (size_t)h.nq * 8) && range_ok(h, h.off_slot_scale, ns * 8) &&
            range_ok(h, h.off_slot_pos_off, ns * 24) && range_ok(h, h.off_slot_rot_off, ns * 32) && range_ok(h, h.off_slot_is_foot, ns * 4);
  for (int k = 0; k < 2; ++k)
    ok = ok && range_ok(h, h.off_task_body[k], (size_t)h.ntask[k] * 4) && range_ok(h, h.off_task_slot[k], (size_t)h.ntask[k] * 4) &&
         range_ok(h, h.off_task_wp[k], (size_t)h.ntask[k] * 8) && range_ok(h, h.off_task_wr[k], (size_t)h.ntask[k] * 8);
  if (!ok) return fail(msg, GMR_EINVAL, "blob array offsets out of range");
  return GMR_OK;
}

inline int view_blob(const void *blob, size_t blob_bytes, BlobView &B, std::string &msg) {
  const int rc = validate_blob(blob, blob_bytes, B.h, msg);
  if (rc != GMR_OK) return rc;
  B.store.assign((blob_bytes + 7) / 8, 0);
  memcpy(B.store.data(), blob, blob_bytes);
  const uint8_t *base = reinterpret_cast<const uint8_t *>(B.store.data());
  const gmr_blob_header &h = B.h;
  auto i32 = [&](uint32_t off) { return reinterpret_cast<const int32_t *>(base + off); };
  auto f64 = [&](uint32_t off) { return reinterpret_cast<const double *>(base + off); };
  B.parent = i32(h.off_parent); B.jtype = i32(h.off_jnt_type); B.qadr = i32(h.off_qpos_adr); B.dadr = i32(h.off_dof_adr);
  B.limited = i32(h.off_jnt_limited);
  B.bpos = f64(h.off_body_pos); B.bquat = f64(h.off_body_quat); B.bquat_raw = f64(h.off_body_quat_raw); B.axis = f64(h.off_jnt_axis);
  B.range = f64(h.off_jnt_range); B.qpos0 = f64(h.off_qpos0);
  B.sscale = f64(h.off_slot_scale); B.spoff = f64(h.off_slot_pos_off); B.sroff = f64(h.off_slot_rot_off); B.sfoot = i32(h.off_slot_is_foot);
  for (int k = 0; k < 2; ++k) {
    B.tbody[k] = i32(h.off_task_body[k]); B.tslot[k] = i32(h.off_task_slot[k]);
    B.twp[k] = f64(h.off_task_wp[k]); B.twr[k] = f64(h.off_task_wr[k]);
  }
  return GMR_OK;
}

// ------------------------------------------------------------------------------------------------ tree check
// depth-first order, free root, hinges elsewhere
inline int check_tree(const BlobView &B, std::string &msg) {
  using plan_detail::fail;
  const gmr_blob_header &h = B.h;
  if (B.parent[0] != -1 || B.jtype[0] != GMR_JNT_FREE || B.qadr[0] != 0 || B.dadr[0] != 0) return fail(msg, GMR_EINVAL, "body 0 must be the free-joint root");
  int nq = 7, nv = 6;
  for (int b = 1; b < h.nbody; ++b) {
    if (B.parent[b] < 0 || B.parent[b] >= b) return fail(msg, GMR_EINVAL, "bodies are not in depth-first order");
    if (B.jtype[b] == GMR_JNT_HINGE) {
      if (B.qadr[b] != nq || B.dadr[b] != nv) return fail(msg, GMR_EINVAL, "joint addresses out of order at body %d", b);
      ++nq; ++nv;
    } else if (B.jtype[b] != GMR_JNT_NONE) return fail(msg, GMR_EUNSUPPORTED, "unsupported joint type at body %d", b);
  }
  if (nq != h.nq || nv != h.nv) return fail(msg, GMR_EINVAL, "nq/nv do not match the joint list");
  return GMR_OK;
}

// ------------------------------------------------------------------------------------------------ tasks and pruned tree
inline int read_tasks(const BlobView &B, TaskTables &T, std::string &msg) {
  const gmr_blob_header &h = B.h;
  T.body.assign(2 * GMR_MAX_TASKS, 0); T.slot.assign(2 * GMR_MAX_TASKS, 0);
  T.wp.assign(2 * GMR_MAX_TASKS, 0.0); T.wr.assign(2 * GMR_MAX_TASKS, 0.0);
  for (int k = 0; k < 2; ++k)
    for (int t = 0; t < h.ntask[k]; ++t) {
      const int32_t tb = B.tbody[k][t], ts = B.tslot[k][t];
      if (tb < 0 || tb >= h.nbody || ts < 0 || ts >= h.nslot) return plan_detail::fail(msg, GMR_EINVAL, "task %d of table %d out of range", t, k + 1);
      T.body[k * GMR_MAX_TASKS + t] = tb; T.slot[k * GMR_MAX_TASKS + t] = ts;
      T.wp[k * GMR_MAX_TASKS + t] = B.twp[k][t]; T.wr[k * GMR_MAX_TASKS + t] = B.twr[k][t];
    }
  return GMR_OK;
}

// Bodies the IK needs: the task bodies and their ancestors.  Everything else (the 14 finger links of unitree_g1_with_hands, head /
// hand cosmetics) never enters a residual or a screw, so the IK kernel works on this pruned tree (fewer lanes, less LDS per
// wavefront); gmr_evaluate keeps the full tree for configuration.data.xpos.
inline PrunedTree prune_tree(const BlobView &B, const TaskTables &T) {
  const gmr_blob_header &h = B.h;
  const int nb = h.nbody;
  PrunedTree P;
  P.bmap.assign(nb, -1);
  std::vector<char> needed(nb, 0);
  needed[0] = 1;
  for (int k = 0; k < 2; ++k)
    for (int t = 0; t < h.ntask[k]; ++t)
      for (int b = T.body[k * GMR_MAX_TASKS + t]; b >= 0 && !needed[b]; b = B.parent[b]) needed[b] = 1;
  for (int b = 0; b < nb; ++b)
    if (needed[b]) { P.bmap[b] = (int)P.keep.size(); P.keep.push_back(b); }
  P.nb_ik = (int)P.keep.size();
  return P;
}

// ------------------------------------------------------------------------------------------------ active dofs
// root 6 + hinges with at least one task (either table) at or below them
inline int active_dofs(const BlobView &B, const TaskTables &T, int min_nvp, ActiveDofs &A, std::string &msg) {
  using plan_detail::fail;
  const gmr_blob_header &h = B.h;
  // the root's six rows.  A planar base (gmr_blob.h root_dof_mask 0x23) keeps all six in the QP, with z / roll / pitch as *null*
  // dofs (kind 7): the kernel's hinge path gives them the root body's hinge axis -- zero -- hence a zero screw, a zero gradient,
  // a diagonal of damping alone and dq = 0 exactly: the reference's 27-dof problem solved inside the 30-row one, with no
  // branch added to the kernel (rows 3, 4, 5 stay the root's rotation step: 0, 0, yaw).  They keep their place in the
  // elimination order but are left out of the ancestor relation (no H pairs) and of the structured QP's core.
  A.root_mask = h.root_dof_mask ? h.root_dof_mask : 0x3F;
  if (A.root_mask != 0x3F && A.root_mask != 0x23) return fail(msg, GMR_EUNSUPPORTED, "root_dof_mask 0x%x: only a free joint (0x3f) or a planar base (0x23) is supported", A.root_mask);
  if (B.axis[0] != 0.0 || B.axis[1] != 0.0 || B.axis[2] != 0.0) return fail(msg, GMR_EINVAL, "the root body must not carry a hinge axis");
  for (int k = 0; k < 6; ++k) {
    A.body.push_back(0); A.kind.push_back(((A.root_mask >> k) & 1) ? k : 7); A.qadr.push_back(k < 3 ? k : 3); A.lim.push_back(0);
    A.range.push_back(0); A.range.push_back(0);
  }
  for (int b = 1; b < h.nbody; ++b) {
    if (B.jtype[b] != GMR_JNT_HINGE) continue;
    bool used = false;
    for (int k = 0; k < 2 && !used; ++k)
      for (int t = 0; t < h.ntask[k] && !used; ++t) used = B.above(b, T.body[k * GMR_MAX_TASKS + t]);
    if (!used) continue;
    A.body.push_back(b); A.kind.push_back(6); A.qadr.push_back(B.qadr[b]); A.lim.push_back(B.limited[b] ? 1 : 0);
    A.range.push_back(B.range[2 * b]); A.range.push_back(B.range[2 * b + 1]);
  }
  A.n_act = (int)A.body.size();
  A.nvp = pick_nvp(std::max(A.n_act, min_nvp));
  if (A.nvp < 0) return fail(msg, GMR_EUNSUPPORTED, "%d active dofs exceed the kernel limit of 64", A.n_act);
  return GMR_OK;
}

// ------------------------------------------------------------------------------------------------ elimination order and ancestor masks
// Elimination order of the QP: sort dofs by height (longest chain of dofs below), tallest first.  Dofs of equal height are never
// above one another, so a kinematic tree eliminates leaves-first without fill-in and all dofs of one height can be eliminated in the
// same step (level-scheduled sparse U D U' in ik_kernel's box_qp).  Permutes A into that order.
inline int elimination_order(const BlobView &B, ActiveDofs &A, DofOrder &O, std::string &msg) {
  using plan_detail::fail;
  const int n_act = A.n_act, n_root = 6;
  // ancestor relation among active dofs in depth-first order (j above i implies j < i)
  auto dfs_anc = [&](int j, int i) {
    if (j >= i) return false;
    if (A.kind[i] != 6) return true;      // root dofs (null ones included) form a chain 0 <- 1 <- ... <- 5
    if (A.kind[j] != 6) return true;      // every hinge hangs below the root's six dofs
    return A.body[j] != A.body[i] && B.above(A.body[j], A.body[i]);
  };
  std::vector<int> height(n_act, 0), perm(n_act);
  for (int i = n_act - 1; i >= 0; --i)
    for (int j = 0; j < i; ++j)
      if (dfs_anc(j, i)) height[j] = std::max(height[j], height[i] + 1);
  std::vector<u64> anc_dfs(n_act, 0);  // relation in depth-first indices, taken before the arrays are permuted
  for (int i = 0; i < n_act; ++i)
    for (int j = 0; j < i; ++j)
      if (dfs_anc(j, i) && A.kind[i] != 7 && A.kind[j] != 7) anc_dfs[i] |= 1ull << j;  // a null dof keeps its place in the order but couples with nothing
  std::iota(perm.begin(), perm.end(), 0);
  std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return height[a] > height[b]; });
  for (int k = 0; k < n_root; ++k)
    if (perm[k] != k) return fail(msg, GMR_EINVAL, "internal: root dofs must lead the elimination order");
  {
    std::vector<int> b2(n_act), k2(n_act), q2(n_act), l2(n_act), h2(n_act);
    std::vector<double> r2(2 * n_act);
    for (int a = 0; a < n_act; ++a) {
      const int o = perm[a];
      b2[a] = A.body[o]; k2[a] = A.kind[o]; q2[a] = A.qadr[o]; l2[a] = A.lim[o]; h2[a] = height[o];
      r2[2 * a] = A.range[2 * o]; r2[2 * a + 1] = A.range[2 * o + 1];
    }
    A.body = b2; A.kind = k2; A.qadr = q2; A.lim = l2; A.range = r2; A.height = h2;
  }
  O.aanc.assign(64, 0);
  for (int a = 0; a < n_act; ++a)
    for (int b = 0; b < n_act; ++b)
      if ((anc_dfs[perm[a]] >> perm[b]) & 1ull) {
        if (b >= a) return fail(msg, GMR_EINVAL, "internal: elimination order breaks ancestor-first indexing");
        O.aanc[a] |= 1ull << b;
      }
  // structurally non-zero off-diagonal pairs of H: (i, j) with dof j strictly above dof i
  O.hpair.clear();
  for (int i = 0; i < n_act; ++i)
    for (int j = 0; j < i; ++j)
      if ((O.aanc[i] >> j) & 1ull) O.hpair.push_back((unsigned short)((i << 8) | j));
  return GMR_OK;
}

// ------------------------------------------------------------------------------------------------ FK jump plan
// FK pointer-jumping plan of a tree given by its parents: ancestor folded in each round, one byte per round.  false: too deep.
inline bool fk_jump_plan(const std::vector<int> &par, FkJumpPlan &J) {
  const int n = (int)par.size();
  int maxd = 0;
  std::vector<int> dep(n, 0);
  for (int b2 = 1; b2 < n; ++b2) { dep[b2] = dep[par[b2]] + 1; maxd = std::max(maxd, dep[b2]); }
  J.rounds = 0;
  while ((1 << J.rounds) <= maxd) ++J.rounds;
  if (J.rounds > 8) return false;
  J.anc.assign(n, ~0ull);
  std::vector<int> anc(par);
  for (int r = 0; r < J.rounds; ++r) {
    std::vector<int> nxt(n, -1);
    for (int b2 = 0; b2 < n; ++b2) {
      const u64 byte = anc[b2] < 0 ? 0xffull : (u64)anc[b2];
      J.anc[b2] = (J.anc[b2] & ~(0xffull << (8 * r))) | (byte << (8 * r));
      nxt[b2] = anc[b2] < 0 ? -1 : anc[anc[b2]];
    }
    anc = nxt;
  }
  for (int b2 = 0; b2 < n; ++b2) if (anc[b2] >= 0) return false;
  return true;
}
// ... for the pruned IK tree and the full tree
inline int fk_jump_plans(const BlobView &B, const PrunedTree &P, FkJumpPlan &ik, FkJumpPlan &full, std::string &msg) {
  const int nb = B.h.nbody;
  std::vector<int> par_full(B.parent, B.parent + nb), par_ik(P.nb_ik);
  for (int i = 0; i < P.nb_ik; ++i) par_ik[i] = P.keep[i] == 0 ? -1 : P.bmap[B.parent[P.keep[i]]];
  if (!fk_jump_plan(par_ik, ik) || !fk_jump_plan(par_full, full)) return plan_detail::fail(msg, GMR_EUNSUPPORTED, "tree too deep");
  return GMR_OK;
}

// ------------------------------------------------------------------------------------------------ structured-QP partition
// Structured QP layout ("core + limbs"): the active dofs are split into an upward-closed core C (root + trunk) and the connected
// pieces left when C is removed (limbs), which never couple with one another.  Four 16-lane groups each hold one bin of limbs
// (rows 0 .. 15-|C|) and a copy of the core (rows 16-|C| .. 15); see box_qp_struct in ik_kernel.hip.h.  Q.ok = 0: no such split.
inline int structured_qp(const ActiveDofs &A, const DofOrder &O, StructuredQp &Q, std::string &msg) {
  const int n_act = A.n_act, n_root = 6;
  const std::vector<u64> &aanc = O.aanc;
  Q.gdof.assign(64, -1); Q.owner.assign(64, 0);
  Q.lane_of_dof.assign(64, 0); Q.diag.assign(64, 0);
  Q.dst.clear();
  Q.ok = 0; Q.nlimb = 0;
  std::vector<int> dparent(n_act, -1), nanc(n_act, 0);
  for (int i = 0; i < n_act; ++i) nanc[i] = __builtin_popcountll(aanc[i]);
  for (int i = 0; i < n_act; ++i)
    for (int j = 0; j < i; ++j)
      if (((aanc[i] >> j) & 1ull) && (dparent[i] < 0 || nanc[j] > nanc[dparent[i]])) dparent[i] = j;
  std::vector<char> in_core(n_act, 0);
  for (int k = 0; k < n_root; ++k) in_core[k] = A.kind[k] != 7;  // null dofs are one-row "limbs": they need no core column
  std::vector<std::vector<int>> bins;
  for (int guard = 0; guard < 64 && !Q.ok; ++guard) {
    const int nc = (int)std::count(in_core.begin(), in_core.end(), (char)1);
    if (nc > 10) break;
    // components of the non-core dofs (dofs are indexed ancestors-first, so a parent is labelled before its children)
    std::vector<int> comp(n_act, -1), csize, ctop;
    for (int i = 0; i < n_act; ++i) {
      if (in_core[i]) continue;
      if (dparent[i] < 0 || in_core[dparent[i]]) { comp[i] = (int)csize.size(); csize.push_back(1); ctop.push_back(i); }
      else { comp[i] = comp[dparent[i]]; csize[comp[i]]++; }
    }
    const int cap = 16 - nc;
    int worst = -1;
    for (size_t c = 0; c < csize.size(); ++c)
      if (csize[c] > cap && (worst < 0 || csize[c] > csize[worst])) worst = (int)c;
    bool packed = worst < 0;
    if (packed) {  // first-fit decreasing into <= 4 bins
      std::vector<int> order(csize.size());
      std::iota(order.begin(), order.end(), 0);
      std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return csize[a] > csize[b]; });
      bins.assign(4, {});
      std::vector<int> fill(4, 0);
      for (int c : order) {
        int g = 0;
        while (g < 4 && fill[g] + csize[c] > cap) ++g;
        if (g == 4) { packed = false; break; }
        fill[g] += csize[c];
        for (int i = 0; i < n_act; ++i) if (comp[i] == c) bins[g].push_back(i);
      }
      if (!packed) for (size_t c = 0; c < csize.size(); ++c) if (worst < 0 || csize[c] > csize[worst]) worst = (int)c;
    }
    if (packed) { Q.ok = 1; Q.nlimb = cap; break; }
    in_core[ctop[worst]] = 1;  // grow the core by the top dof of the largest piece and try again
  }
  if (!Q.ok) return GMR_OK;
  const int nl = Q.nlimb;
  std::vector<int> core;
  for (int i = 0; i < n_act; ++i) if (in_core[i]) core.push_back(i);
  std::vector<int> grp(n_act, 0), loc(n_act, 0);
  for (int g = 0; g < 4; ++g) {
    std::sort(bins[g].begin(), bins[g].end());
    for (size_t a = 0; a < bins[g].size(); ++a) {
      const int i = bins[g][a], L = 16 * g + (int)a;
      grp[i] = g; loc[i] = (int)a; Q.gdof[L] = (signed char)i; Q.owner[L] = 1; Q.lane_of_dof[i] = L;
    }
    for (size_t c = 0; c < core.size(); ++c) {
      const int L = 16 * g + nl + (int)c;
      Q.gdof[L] = (signed char)core[c]; Q.owner[L] = g == 0;
      if (g == 0) { Q.lane_of_dof[core[c]] = L; loc[core[c]] = nl + (int)c; grp[core[c]] = 0; }
    }
  }
  for (int i = 0; i < n_act; ++i) Q.diag[i] = loc[i] * 64 + Q.lane_of_dof[i];
  auto hs = [](int lane, int col) { return (unsigned)(col * 64 + lane); };
  for (unsigned short pr : O.hpair) {
    const int i = pr >> 8, j = pr & 0xff;  // j above i
    unsigned a, b;
    if (in_core[i]) { a = hs(Q.lane_of_dof[i], loc[j]); b = hs(Q.lane_of_dof[j], loc[i]); }  // both core: group 0
    else {
      const int g = grp[i], Li = Q.lane_of_dof[i];
      const int Lj = in_core[j] ? 16 * g + loc[j] : Q.lane_of_dof[j];  // the copy of the core dof inside i's group
      if (!in_core[j] && grp[j] != g) return plan_detail::fail(msg, GMR_EINVAL, "internal: structured QP partition");
      a = hs(Li, loc[j]); b = hs(Lj, loc[i]);
    }
    Q.dst.push_back(a | (b << 16));
  }
  return GMR_OK;
}

// ------------------------------------------------------------------------------------------------ composites
// Composites per table: dofs sharing the same set of tasks below them share one 6x6 block.
inline int composites(const BlobView &B, const TaskTables &T, const ActiveDofs &A, Composites &C, std::string &msg) {
  using plan_detail::fail;
  const gmr_blob_header &h = B.h;
  const int n_act = A.n_act;
  C.acomp.assign(2 * 64, 0);
  C.mask.assign(2 * 2 * GMR_MAX_TASKS, 0u); C.own.assign(64, 0u); C.kids.assign(64, 0u);
  C.ncomp[0] = C.ncomp[1] = 0;
  for (int k = 0; k < 2; ++k) {
    std::map<unsigned, int> ids;
    for (int i = 0; i < n_act; ++i) {
      unsigned mk = 0;
      for (int t = 0; t < h.ntask[k]; ++t)
        if (A.kind[i] != 6 || B.above(A.body[i], T.body[k * GMR_MAX_TASKS + t])) mk |= 1u << t;
      auto it = ids.find(mk);
      if (it == ids.end()) {
        it = ids.emplace(mk, C.ncomp[k]).first;
        C.mask[k * 2 * GMR_MAX_TASKS + C.ncomp[k]] = mk;
        ++C.ncomp[k];
      }
      C.acomp[k * 64 + i] = it->second;
    }
    if (C.ncomp[k] > 2 * GMR_MAX_TASKS) return fail(msg, GMR_EUNSUPPORTED, "too many composite nodes");
    // renumber the composites so that a composite's children (maximal strict subsets) always have lower ids, and split
    // each into "own tasks" + "child composites": Bc[c] = sum_{t in own} Bt[t] + sum_{d in kids} Bc[d]  (any number of either:
    // the pass plan splits a long sum into entries of four sources)
    const int nc = C.ncomp[k];
    if (nc > 32) return fail(msg, GMR_EUNSUPPORTED, "more than 32 composite nodes");
    std::vector<int> order(nc), newid(nc);
    std::iota(order.begin(), order.end(), 0);
    auto mask_of = [&](int c) { return C.mask[k * 2 * GMR_MAX_TASKS + c]; };
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return __builtin_popcount(mask_of(a)) < __builtin_popcount(mask_of(b)); });
    std::vector<unsigned> sorted_mask(nc);
    for (int o = 0; o < nc; ++o) { newid[order[o]] = o; sorted_mask[o] = mask_of(order[o]); }
    for (int i = 0; i < n_act; ++i) C.acomp[k * 64 + i] = newid[C.acomp[k * 64 + i]];
    for (int o = 0; o < nc; ++o) {
      C.mask[k * 2 * GMR_MAX_TASKS + o] = sorted_mask[o];
      unsigned own = sorted_mask[o], kids = 0, covered = 0;
      for (int d = o - 1; d >= 0; --d) {
        const unsigned md = sorted_mask[d];
        if (md == 0 || md == sorted_mask[o] || (md & ~sorted_mask[o]) != 0 || (md & covered) != 0) continue;
        kids |= 1u << d; covered |= md;
      }
      own &= ~covered;
      C.own[k * 32 + o] = own; C.kids[k * 32 + o] = kids;
    }
  }
  return GMR_OK;
}

// ------------------------------------------------------------------------------------------------ LDS layout
// The plans hold LDS byte offsets in 16 bits.
inline int check_lds_16bit(int lds_bytes, std::string &msg) {
  if (lds_bytes > 65535) return plan_detail::fail(msg, GMR_EUNSUPPORTED, "model needs %d bytes of LDS per wavefront (plan offsets are 16 bit)", lds_bytes);
  return GMR_OK;
}
inline int lds_bytes_of(const LdsLayout &L) { return L.total_doubles * (int)sizeof(double); }

// LDS layout of the IK kernel (doubles), without the composite plan's passes and the target ring, which are added once they are
// known (composite_passes, plan_model).  Lifetimes inside one solve:
//   poses (FK .. screws) | Bt (task blocks .. composites) | Bc (composites .. F)   -> Bc overwrites the dead poses
//   S, F (screws / F .. H assembly)                                                 -> the factorisation's broadcast rows Lb overwrite S
//   H (H assembly .. QP) overwrites [Bt | poses/Bc]
inline LdsLayout lds_layout(const gmr_blob_header &h, int nb_ik, int nvp, int npairs, const int ncomp[2], bool sq) {
  using plan_detail::even;
  const int ns = h.nslot;
  const int ntmax = std::max(h.ntask[0], h.ntask[1]), ncmax = std::max(ncomp[0], ncomp[1]);
  LdsLayout L;
  memset(&L, 0, sizeof(L));
  int o = 0;
  L.zero = o; o += kBT;  // a block of zeros: the absent sources of the composite plan (never aliased)
  const int npairp_host = (npairs + 127) / 128 * 128;
  // H pair plan, 8 bytes per entry, staged once per wavefront -- unless the structured kernel keeps all of it in registers
  const bool hplan_in_regs = sq && npairp_host <= 64 * kHPlanRegsSQ;
  L.hplan = o; o += hplan_in_regs ? 0 : npairp_host;
  L.q = o; o += even(h.nq);
  L.tp = o; o += even(3 * ns);
  L.tq = o; o += 4 * ns;
  L.bodyc = GMR_IK_STAGE_TREE ? o : -1; o += GMR_IK_STAGE_TREE ? even(kBodyC * nb_ik) : 0;
  L.S = o; L.Lb = o; o += std::max(6 * nvp, sq ? 128 : 2 * (nvp + 2));
  L.F = o; o += 6 * nvp;
  L.B = o; L.H = o;
  const int bt = even(kBT * ntmax), px = std::max(even(7 * nb_ik), even(kBT * ncmax));
  L.xpos = o + bt; L.xquat = L.xpos + even(3 * nb_ik); L.Bc = o + bt;
  o += std::max(bt + px, (sq ? 1024 : nvp * nvp) + 2);  // + a dummy slot for the unused lanes of the pair rounds
  L.cplan = o;  // composite plan, 16 bytes per (table, pass, quarter-wave); sized once the passes are scheduled
  L.total_doubles = o;
  L.tring = -1;
  return L;
}

// LDS layout of eval_kernel: state, targets, poses of the full tree
inline LdsLayout lds_layout_eval(const gmr_blob_header &h) {
  using plan_detail::even;
  LdsLayout E;
  memset(&E, 0, sizeof(E));
  int oe = 0;
  E.q = oe; oe += even(h.nq);
  E.tp = oe; oe += even(3 * h.nslot);
  E.tq = oe; oe += 4 * h.nslot;
  E.xpos = oe; oe += even(3 * h.nbody);
  E.xquat = oe; oe += 4 * h.nbody;
  E.total_doubles = oe;
  return E;
}

// ------------------------------------------------------------------------------------------------ composite pass schedule
// Composite plan: passes of <= 4 entries, an entry = one composite summed from <= 4 blocks, children before parents.  Turns
// C.acomp into block indices and appends the passes to the layout.
inline int composite_passes(const gmr_blob_header &h, int n_act, Composites &C, LdsLayout &lay, CompositePasses &S, std::string &msg) {
  using plan_detail::fail;
  const int ntmax = std::max(h.ntask[0], h.ntask[1]);
  S.plan.assign((size_t)2 * kMaxCompPass * 4 * 4, 0u);
  S.ncpass[0] = S.ncpass[1] = 0;
  for (int k = 0; k < 2; ++k) {
    struct Entry { int dst; std::vector<int> src; std::vector<int> deps; int done_pass = -1; int height = 0; };
    // src / dst are block ids: task t -> t, composite c -> 64 + c;  deps: entries that must have run in an earlier pass
    std::vector<Entry> ent;
    std::vector<int> last_entry_of_comp(C.ncomp[k], -1);
    // Shallow plan: a composite of ONE task is that task's block (no entry, the dof lanes read the task block itself); a
    // composite of up to four tasks is summed from the task blocks directly (no dependency on its children); only larger ones
    // build on child composites.  G1: 3 dependent passes instead of 5.
    std::vector<int> alias_task(C.ncomp[k], -1);
    for (int c = 0; c < C.ncomp[k]; ++c) {
      const unsigned mk = C.mask[k * 2 * GMR_MAX_TASKS + c];
      if (__builtin_popcount(mk) == 1) alias_task[c] = __builtin_ctz(mk);
    }
    for (int i = 0; i < n_act; ++i) {
      const int c = C.acomp[k * 64 + i];
      C.acomp[k * 64 + i] = alias_task[c] >= 0 ? alias_task[c] : ntmax + c;  // block index from Bt on (Bc = Bt + kBT ntmax)
    }
    for (int c = 0; c < C.ncomp[k]; ++c) {
      if (alias_task[c] >= 0) continue;
      const unsigned mk = C.mask[k * 2 * GMR_MAX_TASKS + c];
      std::vector<int> srcs;
      if (__builtin_popcount(mk) <= 4) {
        for (unsigned t = mk; t; t &= t - 1) srcs.push_back(__builtin_ctz(t));
      } else {
        for (unsigned own = C.own[k * 32 + c]; own; own &= own - 1) srcs.push_back(__builtin_ctz(own));
        for (unsigned kids = C.kids[k * 32 + c]; kids; kids &= kids - 1) {
          const int d = __builtin_ctz(kids);
          srcs.push_back(alias_task[d] >= 0 ? alias_task[d] : 64 + d);
        }
      }
      // child composites first: the entries that wait for them should be few
      std::stable_sort(srcs.begin(), srcs.end(), [](int a, int b) { return (a >= 64) > (b >= 64); });
      size_t i = 0;
      bool first = true;
      while (i < srcs.size() || first) {
        Entry e;
        e.dst = 64 + c;
        if (!first) { e.src.push_back(64 + c); e.deps.push_back(last_entry_of_comp[c]); }
        while (i < srcs.size() && e.src.size() < 4) {
          const int sidx = srcs[i++];
          e.src.push_back(sidx);
          if (sidx >= 64) e.deps.push_back(last_entry_of_comp[sidx - 64]);
        }
        last_entry_of_comp[c] = (int)ent.size();
        ent.push_back(std::move(e));
        first = false;
      }
    }
    const int ne = (int)ent.size();
    // height = longest chain of dependants above an entry (critical-path priority)
    for (int i = ne - 1; i >= 0; --i)
      for (int d : ent[i].deps) ent[d].height = std::max(ent[d].height, ent[i].height + 1);
    int done = 0, pass = 0;
    const int boff = lay.B * 8, coff = lay.Bc * 8, zoff = lay.zero * 8, scratch = lay.F * 8;  // F is dead during this phase
    auto block_off = [&](int id) { return id >= 64 ? coff + kBT * 8 * (id - 64) : boff + kBT * 8 * id; };
    while (done < ne) {
      if (pass >= kMaxCompPass) return fail(msg, GMR_EUNSUPPORTED, "composite plan of table %d needs more than %d passes", k + 1, kMaxCompPass);
      int pick[4] = {-1, -1, -1, -1};
      for (int slot = 0; slot < 4; ++slot) {
        int best = -1;
        for (int i = 0; i < ne; ++i) {
          if (ent[i].done_pass >= 0 || i == pick[0] || i == pick[1] || i == pick[2]) continue;
          bool ready = true;
          for (int d : ent[i].deps) ready = ready && ent[d].done_pass >= 0 && ent[d].done_pass < pass;
          if (ready && (best < 0 || ent[i].height > ent[best].height)) best = i;
        }
        pick[slot] = best;
      }
      if (pick[0] < 0) return fail(msg, GMR_EINVAL, "internal: composite plan stalled");
      for (int quarter = 0; quarter < 4; ++quarter) {
        uint32_t *row = S.plan.data() + ((size_t)(k * kMaxCompPass + pass) * 4 + quarter) * 4;
        const int ei = pick[quarter];
        uint32_t so[4] = {(uint32_t)zoff, (uint32_t)zoff, (uint32_t)zoff, (uint32_t)zoff}, dst = (uint32_t)scratch;
        if (ei >= 0) {
          for (size_t j = 0; j < ent[ei].src.size(); ++j) so[j] = (uint32_t)block_off(ent[ei].src[j]);
          dst = (uint32_t)block_off(ent[ei].dst);
        }
        row[0] = so[0] | (so[1] << 16); row[1] = so[2] | (so[3] << 16); row[2] = dst; row[3] = 0;
      }
      for (int slot = 0; slot < 4; ++slot)
        if (pick[slot] >= 0) { ent[pick[slot]].done_pass = pass; ++done; }
      ++pass;
    }
    S.ncpass[k] = pass;
  }
  if (getenv("GMR_DEBUG_PLAN")) fprintf(stderr, "gmr: composite plan: %d / %d composites, %d / %d passes\n", C.ncomp[0], C.ncomp[1], S.ncpass[0], S.ncpass[1]);
  lay.total_doubles += 8 * (S.ncpass[0] + S.ncpass[1]);
  return GMR_OK;
}

// ------------------------------------------------------------------------------------------------ H pair plan and its ordering
// H assembly plan: per pair the LDS byte offsets of S_j, F_i and of the two entries of H it fills, in pair order, padded to a
// multiple of 128 entries with ones that land in the two dummy slots behind H.
inline std::vector<uint32_t> h_pair_plan(const LdsLayout &Ly, const DofOrder &O, const StructuredQp &Q, bool sq, int nvp) {
  std::vector<uint32_t> hplan;
  const int hsize = sq ? 1024 : nvp * nvp;  // the two doubles after H are the dummy slots of the padding entries
  for (size_t p = 0; p < O.hpair.size(); ++p) {
    const int i = O.hpair[p] >> 8, j = O.hpair[p] & 0xff;
    const unsigned d0 = sq ? (Q.dst[p] & 0xffffu) : (unsigned)(j * nvp + i), d1 = sq ? (Q.dst[p] >> 16) : (unsigned)(i * nvp + j);
    hplan.push_back((uint32_t)((Ly.S + 6 * j) * 8) | ((uint32_t)((Ly.F + 6 * i) * 8) << 16));
    hplan.push_back((uint32_t)((Ly.H + (int)d0) * 8) | ((uint32_t)((Ly.H + (int)d1) * 8) << 16));
  }
  while ((hplan.size() / 2) % 128 != 0) {
    hplan.push_back((uint32_t)(Ly.S * 8) | ((uint32_t)(Ly.F * 8) << 16));
    hplan.push_back((uint32_t)((Ly.H + hsize) * 8) | ((uint32_t)((Ly.H + hsize + 1) * 8) << 16));
  }
  return hplan;
}

// Order of the entries = (round, lane) that executes them.  The gathers of S_j / F_i are ds_read_b128 (serviced in four
// fixed 16-lane groups, a lane occupying the 16-byte slot (addr / 16) mod 16; equal addresses broadcast) and the two
// scatters are ds_write_b64 (16 contiguous lanes per group, unit (addr / 8) mod 16): entries are swapped between positions
// while that lowers the number of extra LDS cycles (hill climbing with a fixed seed -- the plan is a pure function of the
// model).  Measured on G1: SQ_LDS_BANK_CONFLICT of the H phase (profiles/experiment_log_r01_r02.md, v11).
inline std::vector<uint32_t> order_h_pair_plan(const std::vector<uint32_t> &hplan) {
  const int ne = (int)hplan.size() / 2, nr = ne / 64;
  static const int rgroup[64] = {0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1,
                                 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3, 2, 2, 2, 2, 3, 3, 3, 3, 2, 2, 2, 2, 2, 2, 2, 2, 3, 3, 3, 3};
  std::vector<int> at(ne);  // position -> entry
  for (int i = 0; i < ne; ++i) at[i] = i;
  // extra cycles of one 16-lane group: max over slots of the number of distinct addresses on it, minus one
  auto extra = [&](const int *pos, int shift, int word, int half) {
    unsigned addr[16]; int slot[16];
    for (int l = 0; l < 16; ++l) {
      const uint32_t wv = hplan[2 * at[pos[l]] + word];
      addr[l] = half ? (wv >> 16) : (wv & 0xffffu);
      slot[l] = (int)(addr[l] >> shift) & 15;
    }
    int worst = 1;
    for (int sl = 0; sl < 16; ++sl) {
      int nd = 0; unsigned seen[16];
      for (int l = 0; l < 16; ++l) {
        if (slot[l] != sl) continue;
        bool dup = false;
        for (int t = 0; t < nd; ++t) dup = dup || seen[t] == addr[l];
        if (!dup) seen[nd++] = addr[l];
      }
      worst = std::max(worst, nd);
    }
    return worst - 1;
  };
  auto round_cost = [&](int r) {
    int c = 0;
    for (int g = 0; g < 4; ++g) {
      int rp[16], wp[16], n = 0;
      for (int l = 0; l < 64; ++l) if (rgroup[l] == g) rp[n++] = 64 * r + l;
      for (int l = 0; l < 16; ++l) wp[l] = 64 * r + 16 * g + l;
      c += 3 * (extra(rp, 4, 0, 0) + extra(rp, 4, 0, 1));  // three b128 reads each of S_j and F_i
      c += extra(wp, 3, 1, 0) + extra(wp, 3, 1, 1);
    }
    return c;
  };
  std::vector<int> rc(nr);
  for (int r = 0; r < nr; ++r) rc[r] = round_cost(r);
  int total0 = 0;
  for (int r = 0; r < nr; ++r) total0 += rc[r];
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (uint32_t)(rng >> 32); };
  for (int iter = 0; iter < 40000 && nr > 0; ++iter) {
    const int a = (int)(next() % (uint32_t)ne), b = (int)(next() % (uint32_t)ne);
    if (a == b) continue;
    const int ra = a / 64, rb = b / 64;
    std::swap(at[a], at[b]);
    const int na = round_cost(ra), nb2 = ra == rb ? na : round_cost(rb);
    const int before = rc[ra] + (ra == rb ? 0 : rc[rb]), after = na + (ra == rb ? 0 : nb2);
    if (after <= before) { rc[ra] = na; rc[rb] = nb2; }
    else std::swap(at[a], at[b]);
  }
  std::vector<uint32_t> ordered(hplan.size());
  for (int i = 0; i < ne; ++i) { ordered[2 * i] = hplan[2 * at[i]]; ordered[2 * i + 1] = hplan[2 * at[i] + 1]; }
  int total = 0;
  for (int r = 0; r < nr; ++r) total += rc[r];
  if (getenv("GMR_DEBUG_PLAN")) fprintf(stderr, "gmr: H pair plan %d entries, modelled conflict cycles per solve %d -> %d\n", ne, total0, total);
  return ordered;
}

// ------------------------------------------------------------------------------------------------ FK slot plan
// FK (KinematicsModel convention) tables and branch-slot plan: a body whose parent is not the previous body reads its parent's pose
// from the slot the parent saved it in; a slot is free again behind the parent's last child.
inline int fk_slot_plan(const BlobView &B, FkSlots &F, std::string &msg) {
  using plan_detail::fail;
  const int nb = B.h.nbody;
  const int32_t *parent = B.parent;
  F.dofidx.assign(nb, -1); F.src_slot.assign(nb, -1); F.save_slot.assign(nb, -1);
  std::vector<int> last_child(nb, -1), nchild_other(nb, 0);
  F.lpos.assign(3 * nb, 0.f); F.lrot.assign(4 * nb, 0.f); F.jaxis.assign(3 * nb, 0.f);
  F.jaxis64.assign(3 * nb, 0.0);
  for (int b = 0; b < nb; ++b) {
    if (B.jtype[b] == GMR_JNT_HINGE) F.dofidx[b] = B.qadr[b] - 7;
    for (int i = 0; i < 3; ++i) { F.lpos[3 * b + i] = (float)B.bpos[3 * b + i]; F.jaxis[3 * b + i] = (float)B.axis[3 * b + i]; F.jaxis64[3 * b + i] = B.axis[3 * b + i]; }
    F.lrot[4 * b + 0] = (float)B.bquat_raw[4 * b + 1]; F.lrot[4 * b + 1] = (float)B.bquat_raw[4 * b + 2];
    F.lrot[4 * b + 2] = (float)B.bquat_raw[4 * b + 3]; F.lrot[4 * b + 3] = (float)B.bquat_raw[4 * b + 0];
    if (b > 0) { last_child[parent[b]] = b; if (parent[b] != b - 1) nchild_other[parent[b]]++; }
  }
  std::vector<int> free_slots;
  F.nslots = 0;
  for (int b = 0; b < nb; ++b) {
    if (b > 0 && parent[b] != b - 1) {
      F.src_slot[b] = F.save_slot[parent[b]];
      if (F.src_slot[b] < 0) return fail(msg, GMR_EINVAL, "internal: FK slot plan");
    }
    if (b > 0 && last_child[parent[b]] == b && F.save_slot[parent[b]] >= 0) free_slots.push_back(F.save_slot[parent[b]]);
    if (nchild_other[b] > 0) {
      if (!free_slots.empty()) { F.save_slot[b] = free_slots.back(); free_slots.pop_back(); }
      else F.save_slot[b] = F.nslots++;
    }
  }
  if (F.nslots > kFkMaxSlots) return fail(msg, GMR_EUNSUPPORTED, "tree too bushy for the FK kernel (%d branch slots)", F.nslots);
  return GMR_OK;
}

// ------------------------------------------------------------------------------------------------ kin-ops and report tables
// kin_ops tables: hinge -> body, float32 limits, tree level of every body, bodies by level; clip report: float64 limits of every
// hinge in qpos order, infinite where the hinge is unlimited
inline KinReport kin_report_tables(const BlobView &B, const FkSlots &F) {
  const int nb = B.h.nbody, ndof_k = B.h.nq - 7;
  KinReport K;
  K.dof_body.assign(ndof_k, 0);
  K.lo.assign(ndof_k, 0.f); K.hi.assign(ndof_k, 0.f);
  for (int b = 0; b < nb; ++b)
    if (F.dofidx[b] >= 0 && F.dofidx[b] < ndof_k) { K.dof_body[F.dofidx[b]] = b; K.lo[F.dofidx[b]] = (float)B.range[2 * b]; K.hi[F.dofidx[b]] = (float)B.range[2 * b + 1]; }
  K.depth.assign(nb, 0); K.order.assign(nb, 0);
  K.maxd = 0;
  for (int b = 1; b < nb; ++b) { K.depth[b] = (uint8_t)(K.depth[B.parent[b]] + 1); K.maxd = std::max<int>(K.maxd, K.depth[b]); }
  std::iota(K.order.begin(), K.order.end(), (uint8_t)0);
  std::stable_sort(K.order.begin(), K.order.end(), [&](uint8_t a, uint8_t b) { return K.depth[a] < K.depth[b]; });
  K.rep_lo.assign(ndof_k, -INFINITY); K.rep_hi.assign(ndof_k, INFINITY);
  for (int b = 1; b < nb; ++b)
    if (B.jtype[b] == GMR_JNT_HINGE && B.limited[b]) { K.rep_lo[B.qadr[b] - 7] = B.range[2 * b]; K.rep_hi[B.qadr[b] - 7] = B.range[2 * b + 1]; }
  return K;
}

// ------------------------------------------------------------------------------------------------ pack
// The two DevModels: the IK model on the pruned tree, and the evaluation model -- same tables, full body tree (gmr_evaluate returns
// xpos / xquat of every body).  Both start from zeroed bytes, padding included: what is uploaded (and hashed) is determinate.
inline int pack_dev_models(const PlanStages &s, DevModel &dm, DevModel &de, std::string &msg) {
  const BlobView &B = s.blob;
  const gmr_blob_header &h = B.h;
  const int nb = h.nbody, ns = h.nslot, nb_ik = s.tree.nb_ik, n_act = s.act.n_act;
  std::vector<int> v_jtype(B.jtype, B.jtype + nb), v_qadr(B.qadr, B.qadr + nb);
  std::vector<double> v_bpos(B.bpos, B.bpos + 3 * nb), v_bquat(B.bquat, B.bquat + 4 * nb), v_axis(B.axis, B.axis + 3 * nb), v_qpos0(B.qpos0, B.qpos0 + h.nq);
  std::vector<int> p_jtype(nb_ik), p_qadr(nb_ik);
  std::vector<double> p_bpos(3 * nb_ik), p_bquat(4 * nb_ik), p_axis(3 * nb_ik);
  for (int i = 0; i < nb_ik; ++i) {
    const int b = s.tree.keep[i];
    p_jtype[i] = B.jtype[b]; p_qadr[i] = B.qadr[b];
    for (int c = 0; c < 3; ++c) { p_bpos[3 * i + c] = B.bpos[3 * b + c]; p_axis[3 * i + c] = B.axis[3 * b + c]; }
    for (int c = 0; c < 4; ++c) p_bquat[4 * i + c] = B.bquat[4 * b + c];
  }
  const std::vector<int> &tbody = s.tasks.body, &tslot = s.tasks.slot;
  std::vector<int> tbody_ik(tbody), abody_ik(s.act.body);
  for (int &b : tbody_ik) b = s.tree.bmap[b] < 0 ? 0 : s.tree.bmap[b];
  for (int &b : abody_ik) b = s.tree.bmap[b];
  std::vector<double> v_sscale(B.sscale, B.sscale + ns), v_spoff(B.spoff, B.spoff + 3 * ns), v_sroff(B.sroff, B.sroff + 4 * ns);
  std::vector<int> v_sfoot(B.sfoot, B.sfoot + ns);
  std::vector<int> abody(s.act.body), akind(s.act.kind), aqadr(s.act.qadr), alim(s.act.lim);
  std::vector<double> arange(s.act.range);
  abody_ik.resize(64, 0); abody.resize(64, 0); akind.resize(64, 0); aqadr.resize(64, 0); alim.resize(64, 0); arange.resize(128, 0.0);

  memset(&dm, 0, sizeof(dm));
  dm.nbody = nb_ik; dm.nq = h.nq; dm.nv = h.nv; dm.nslot = ns; dm.root_slot = h.root_slot; dm.n_act = n_act;
  {  // both tables used and task t of either table ties the same robot body to the same human slot: stage 2 inherits the residual
    bool same = h.use_table[0] && h.use_table[1] && h.ntask[0] == h.ntask[1] && h.ntask[0] > 0;
    for (int t = 0; same && t < h.ntask[0]; ++t)
      same = tbody_ik[t] == tbody_ik[GMR_MAX_TASKS + t] && tslot[t] == tslot[GMR_MAX_TASKS + t];
    dm.same_tasks = same ? 1 : 0;
  }
  dm.root_planar = s.act.root_mask == 0x23;
  dm.root_tslot = -1;  // GMR_INIT_ROOT_TARGET: the slot whose prepared target the floating base (body 0) is asked to track
  for (int k = 0; k < 2 && dm.root_tslot < 0; ++k)
    for (int t = 0; h.use_table[k] && t < h.ntask[k] && dm.root_tslot < 0; ++t)
      if (tbody[k * GMR_MAX_TASKS + t] == 0) dm.root_tslot = tslot[k * GMR_MAX_TASKS + t];
  for (int k = 0; k < 2; ++k) {
    dm.ntask[k] = h.ntask[k]; dm.use_table[k] = h.use_table[k] && h.ntask[k] > 0; dm.ncomp[k] = s.comp.ncomp[k]; dm.ncpass[k] = s.passes.ncpass[k];
  }
  dm.npairp = (int)s.hplan.size() / 2; dm.fkrounds = s.fk_ik.rounds; dm.sq_ok = s.sq.ok; dm.sq_nlimb = s.sq.nlimb;
  bool fits = true;
  auto put = [&](auto &dst, const auto &src) {  // vector -> fixed-capacity array of the device struct
    using D = std::remove_reference_t<decltype(dst[0])>;
    static_assert(sizeof(D) % sizeof(src[0]) == 0, "element size mismatch");
    if (src.size() * sizeof(src[0]) > sizeof(dst)) { fits = false; return; }
    if (!src.empty()) memcpy(&dst[0], src.data(), src.size() * sizeof(src[0]));
  };
  put(dm.jtype, p_jtype); put(dm.qadr, p_qadr);
  put(dm.bpos, p_bpos); put(dm.bquat, p_bquat); put(dm.axis, p_axis); put(dm.qpos0, v_qpos0);
  put(dm.sscale, v_sscale); put(dm.spoff, v_spoff); put(dm.sroff, v_sroff); put(dm.sfoot, v_sfoot);
  put(dm.tbody, tbody_ik); put(dm.tslot, tslot); put(dm.twp, s.tasks.wp); put(dm.twr, s.tasks.wr);
  put(dm.abody, abody_ik); put(dm.akind, akind); put(dm.aqadr, aqadr); put(dm.alimited, alim);
  put(dm.arange, arange); put(dm.acomp, s.comp.acomp);
  put(dm.hplan, s.hplan); put(dm.fkanc, s.fk_ik.anc); put(dm.comp_plan, s.passes.plan);
  put(dm.sq_gdof, s.sq.gdof); put(dm.sq_owner, s.sq.owner); put(dm.sq_lane_of_dof, s.sq.lane_of_dof); put(dm.sq_diag, s.sq.diag);
  memcpy(&de, &dm, sizeof(de));
  de.nbody = nb; de.fkrounds = s.fk_full.rounds;
  put(de.jtype, v_jtype); put(de.qadr, v_qadr);
  put(de.bpos, v_bpos); put(de.bquat, v_bquat); put(de.axis, v_axis);
  put(de.tbody, tbody); put(de.abody, abody); put(de.fkanc, s.fk_full.anc);
  if (!fits) return plan_detail::fail(msg, GMR_EUNSUPPORTED, "internal: a model table exceeds its fixed capacity");
  return GMR_OK;
}

inline void pack_image(const PlanStages &s, const ModelPlan &plan, ModelImage &I) {
  const BlobView &B = s.blob;
  const int nb = B.h.nbody;
  const FkSlots &F = s.slots;
  CallBlock &P = I.block;
  I.dm = P.put(&plan.dm, 1, 1);
  I.dm_eval = P.put(&plan.dm_eval, 1, 1);
  I.parent = P.put(std::vector<int>(B.parent, B.parent + nb), 1);
  I.dofidx = P.put(F.dofidx, 1); I.src_slot = P.put(F.src_slot, 1); I.save_slot = P.put(F.save_slot, 1);
  I.lpos = P.put(F.lpos, 1); I.lrot = P.put(F.lrot, 1); I.jaxis = P.put(F.jaxis, 1);
  I.jaxis64 = P.put(F.jaxis64, 1);
  std::vector<FkBody> fkbody(nb);
  for (int b = 0; b < nb; ++b) {
    FkBody &r = fkbody[b];
    memset(&r, 0, sizeof(r));
    r.src_slot = F.src_slot[b]; r.dofidx = F.dofidx[b]; r.save_slot = F.save_slot[b];
    for (int i = 0; i < 3; ++i) { r.lpos[i] = F.lpos[3 * b + i]; r.axis[i] = F.jaxis64[3 * b + i]; }
    for (int i = 0; i < 4; ++i) r.lrot[i] = F.lrot[4 * b + i];
  }
  I.fkbody = P.put(fkbody, 1);
  I.k_dof_body = P.put(s.kin.dof_body, 1);
  I.k_lo = P.put(s.kin.lo, 1); I.k_hi = P.put(s.kin.hi, 1);
  I.k_depth = P.put(s.kin.depth, 1); I.k_order = P.put(s.kin.order, 1);
  I.rep_lo = P.put(s.kin.rep_lo, 1); I.rep_hi = P.put(s.kin.rep_hi, 1);
}

// ------------------------------------------------------------------------------------------------ the entry
// Plans the model of `blob` for a kernel variant of at least min_nvp rows (group members are built for a common variant), with the
// dense generic QP where force_generic says so.  Returns GMR_OK, or an error code with its message in `msg`.  stages: NULL, or where
// to leave the intermediate tables.
inline int plan_model(const void *blob, size_t blob_bytes, int min_nvp, bool force_generic, ModelPlan &plan, std::string &msg,
                      PlanStages *stages = nullptr) {
  PlanStages local;
  PlanStages &s = stages ? *stages : local;
  int rc;
  if ((rc = view_blob(blob, blob_bytes, s.blob, msg)) != GMR_OK) return rc;
  const gmr_blob_header &h = s.blob.h;
  if ((rc = check_tree(s.blob, msg)) != GMR_OK) return rc;
  if ((rc = read_tasks(s.blob, s.tasks, msg)) != GMR_OK) return rc;
  s.tree = prune_tree(s.blob, s.tasks);
  if ((rc = active_dofs(s.blob, s.tasks, min_nvp, s.act, msg)) != GMR_OK) return rc;
  if ((rc = elimination_order(s.blob, s.act, s.order, msg)) != GMR_OK) return rc;
  if ((rc = fk_jump_plans(s.blob, s.tree, s.fk_ik, s.fk_full, msg)) != GMR_OK) return rc;
  if ((rc = structured_qp(s.act, s.order, s.sq, msg)) != GMR_OK) return rc;
  if ((rc = composites(s.blob, s.tasks, s.act, s.comp, msg)) != GMR_OK) return rc;
  s.use_sq = s.sq.ok && !force_generic;
  plan.nvp = s.act.nvp;
  plan.n_act = s.act.n_act;
  plan.lay = lds_layout(h, s.tree.nb_ik, plan.nvp, (int)s.order.hpair.size(), s.comp.ncomp, s.use_sq);
  if ((rc = check_lds_16bit(lds_bytes_of(plan.lay), msg)) != GMR_OK) return rc;
  if ((rc = composite_passes(h, plan.n_act, s.comp, plan.lay, s.passes, msg)) != GMR_OK) return rc;
  if ((rc = check_lds_16bit(lds_bytes_of(plan.lay), msg)) != GMR_OK) return rc;
  s.hplan_pairs = h_pair_plan(plan.lay, s.order, s.sq, s.use_sq, plan.nvp);
  s.hplan = order_h_pair_plan(s.hplan_pairs);
  if ((rc = fk_slot_plan(s.blob, s.slots, msg)) != GMR_OK) return rc;
  if ((rc = pack_dev_models(s, plan.dm, plan.dm_eval, msg)) != GMR_OK) return rc;
  plan.lay_eval = lds_layout_eval(h);
  plan.lds_bytes_eval = lds_bytes_of(plan.lay_eval);
  plan.shape = ik_shape_of(plan.dm, plan.nvp, s.use_sq);
  // A model that matches a plain shape gets the ring of target images its instances prepare four frames at a time (target_blocks.h):
  // kTargetBlockFrames x [tp | tq] behind everything else.  G1 / smplx: 16 176 + 3 136 = 19 312 bytes, still eight wavefronts per CU.
  if (ik_shape_is_plain(plan.shape) && h.nslot <= kTargetBlockLanes) {
    plan.lay.tring = plan.lay.total_doubles;
    plan.lay.total_doubles += kTargetBlockFrames * (plan.lay.tq - plan.lay.tp + 4 * h.nslot);
    if ((rc = check_lds_16bit(lds_bytes_of(plan.lay), msg)) != GMR_OK) return rc;
  }
  plan.lds_bytes = lds_bytes_of(plan.lay);
  s.kin = kin_report_tables(s.blob, s.slots);
  plan.nslots = s.slots.nslots;
  plan.k_maxd = s.kin.maxd;
  plan.dof_in_order = 1;
  for (int b = 0, prev = -1; b < h.nbody; ++b)
    if (s.slots.dofidx[b] >= 0) { if (s.slots.dofidx[b] < prev) plan.dof_in_order = 0; prev = s.slots.dofidx[b]; }
  // branch slots + dof tile + position / rotation stages (fk_kernel.hip.h)
  plan.fk_lds_bytes = (std::max(1, plan.nslots) * 7 + kFkPosStride + kFkRotStride) * kFkThreads * (int)sizeof(float);
  plan.fk_lds_bytes_min = std::max(1, plan.nslots) * 7 * kFkThreads * (int)sizeof(float);
  pack_image(s, plan, plan.image);
  return GMR_OK;
}

}  // namespace gmr

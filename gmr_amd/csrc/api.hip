// api.hip -- C ABI of libgmr_amd.so (include/gmr_amd.h): model handle, scheduling, kernel launches.
//
// Host side is plain C++: one device allocation per model for the image that model_plan.h plans from the
// blob (validation, active-dof list, ancestor masks, composite nodes of the task tree, LDS layout, FK
// branch-slot plan: host-only code, tested without a device), stream-ordered scheduling scratch, and shape
// checks in front of every launch.  No torch, no CPU fallback: every failure is reported, nothing is
// silently computed elsewhere.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <numeric>
#include <string>
#include <vector>

#include "fk_kernel.hip.h"
#include "ik_kernel.hip.h"
#include "bvh_kernel.hip.h"
#include "smplx_kernel.hip.h"
#include "smplx_body_kernel.hip.h"
#include "bvh_parse_kernel.hip.h"
#include "kin_ops_kernel.hip.h"
#include "motion_kernel.hip.h"
#include "track_kernel.hip.h"
#include "lowpass_kernel.hip.h"
#include "sample_kernel.hip.h"
#include "report_kernel.hip.h"
#include "contact_kernel.hip.h"
#include "dynamics_kernel.hip.h"
#include "footlock_kernel.hip.h"
#include "self_collision_kernel.hip.h"
#include "self_collision_repair_kernel.hip.h"
#include "mirror_kernel.hip.h"
#include "compose_kernel.hip.h"
#include "transitions_kernel.hip.h"
#include "retime_kernel.hip.h"
#include "retime_torque_kernel.hip.h"
#include "bvh_text.h"
#include "call_block.h"
#include "clip_launch.h"
#include "model_plan.h"

using gmr::u64;

struct gmr_model {
  int device = -1;
  gmr_blob_header h{};
  std::vector<uint8_t> blob;
  std::string err;
  // device storage
  void *dev = nullptr;
  size_t dev_bytes = 0;
  gmr::DevModel dm{};                      // host copy of the device model (scalars are read back by the host API)
  const gmr::DevModel *dm_dev = nullptr;  // the struct in device memory: the one model argument of the IK kernels
  const gmr::DevModel *dm_eval_dev = nullptr;  // the same with the full body tree (gmr_evaluate)
  gmr::LdsLayout lay_eval{};
  int lds_bytes_eval = 0;
  gmr::FkTree fk{};
  gmr::KinTables kin{};                    // dof_to_rot / rot_to_dof / local -> global (kin_ops_kernel.hip.h)
  const double *rep_lo = nullptr, *rep_hi = nullptr;  // device [nq - 7]: hinge limits in qpos order, -inf / +inf where unlimited (gmr_clip_report)
  gmr::LdsLayout lay{};
  int nvp = 0, n_act = 0, lds_bytes = 0, fk_lds_bytes = 0, fk_lds_bytes_min = 0;  // _min: the min-height mode has no output stage
  unsigned long long *dbg = nullptr;  // diagnostic builds (GMR_IK_STAMPS) only
  int min_nvp = 0;                    // group members are built for a common kernel variant (gmr_group_create)
  hipMemPool_t pool = nullptr;        // the library's scratch pool of this device (scratch_pool)
  int fk_pos_parts = 1;               // gmr_fk without rotations: fk_pos_kernel<parts> (GMR_AMD_FK_PARTS=0 falls back to fk_kernel<0>)
  bool force_generic = false;         // GMR_AMD_GENERIC_QP=1: use the dense generic QP even where the structured one applies
  bool force_generic_shape = false;   // GMR_AMD_GENERIC_SHAPE=1: never a shaped kernel instance (tests, A/B runs)
  int shape = -1;                     // index into GMR_FOR_EACH_IK_SHAPE of the shape this model matches, -1 = none (ik_shape_of)
  // per-solve step cap (gmr_model_set_step_cap): the caller's table in dof order, and on the device [64] by active dof
  std::vector<double> cap_host;       // [nv]; empty = off
  double *cap_dev = nullptr;          // allocated by the first set, rewritten in place by later ones
  const double *step_cap() const { return cap_host.empty() ? nullptr : cap_dev; }
  // sliced launches (ik_kernel_sliced): the pinned word a wavefront that hit the poll cap sets, and the wavefront slots of the device
  unsigned *slice_err = nullptr, *slice_err_dev = nullptr;  // allocated with the handle
  int slots = 0;
};

// State of a single-sequence session (gmr_session_*): one frame per call, warm start carried on the device.
struct gmr_session {
  gmr_model *m = nullptr;
  hipStream_t st = nullptr;
  uint8_t *host = nullptr;   // pinned, device-visible: [pos | quat | qpos_out(nq) | solves]
  uint8_t *dev = nullptr;    // [qpos state (nq doubles) | work item | slot_col]
  size_t pos_bytes = 0, quat_bytes = 0, quat_off = 0, out_off = 0;
  gmr::IkLaunch L{};
  // persistent mode (gmr_session_set_persistent): a resident wavefront fed through a pinned mailbox
  gmr::IkSessionBox *box = nullptr;        // inside `host`
  gmr::IkSessionBox *box_dev = nullptr;    // its device address
  gmr::IkGroupEntry *entries = nullptr;    // device: the one-frame work item with offset_to_ground = 0 / 1
  int idle_ms = 0;                         // 0 = one launch per frame
  unsigned seq = 0, gen = 0;               // frames posted; resident wavefronts launched (alive: box->exited_gen != gen)
};

// Several models built for one kernel variant (gmr_group_*).
struct gmr_group {
  std::vector<gmr_model *> models;
  int device = -1, nvp = 0;
  bool sq = false;
  std::string err;
};


namespace {

void set_err(gmr_model *m, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (m) m->err = buf;
}

// HIP_TRY's error sink: a model (its last error) or the message string a shared host path was given.
std::string &err_of(gmr_model *m) { return m->err; }
std::string &err_of(std::string &err) { return err; }

#define HIP_TRY(sink, expr)                                                           \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess) {                                                           \
      err_of(sink) = std::string(#expr " failed: ") + hipGetErrorString(e_);          \
      return GMR_EDEVICE;                                                             \
    }                                                                                 \
  } while (0)

template <class T>
const T *blob_ptr(const std::vector<uint8_t> &b, uint32_t off) {
  return reinterpret_cast<const T *>(b.data() + off);
}

// Per-call scheduling data (work items, slot columns, clip offsets) lives in stream-ordered memory: allocated on the call's
// stream and released on it right behind the launch that reads it.  Calls on the same handle from different streams or host
// threads therefore never share (or pull away) each other's launch metadata; the pool keeps released blocks for reuse
// (release threshold set in gmr_model_create), so a call costs no device synchronisation.
struct CallScratch {
  void *p = nullptr;
  hipStream_t st = nullptr;
  ~CallScratch() { if (p) (void)hipFreeAsync(p, st); }
};
// The library's own pool, one per device, created on first use and kept for the life of the process: the few KB of per-call
// scheduling data never touch the device's default pool, whose settings belong to the host application.  Released
// blocks stay cached up to 64 MiB, so a call costs no device synchronisation.
hipMemPool_t scratch_pool(int device) {
  static std::mutex mu;
  static std::map<int, hipMemPool_t> pools;
  std::lock_guard<std::mutex> lock(mu);
  auto it = pools.find(device);
  if (it != pools.end()) return it->second;
  hipMemPoolProps props{};
  props.allocType = hipMemAllocationTypePinned;
  props.handleTypes = hipMemHandleTypeNone;
  props.location.type = hipMemLocationTypeDevice;
  props.location.id = device;
  hipMemPool_t pool = nullptr;
  if (hipMemPoolCreate(&pool, &props) != hipSuccess) { (void)hipGetLastError(); pool = nullptr; }
  if (pool) {
    uint64_t keep = 64ull << 20;
    (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
  }
  pools[device] = pool;
  return pool;
}
int scratch_alloc(const gmr_model *m, CallScratch &sc, size_t bytes, hipStream_t st, std::string &err) {
  sc.st = st;
  if (m->pool) HIP_TRY(err, hipMallocFromPoolAsync(&sc.p, std::max<size_t>(bytes, 256), m->pool, st));
  else HIP_TRY(err, hipMallocAsync(&sc.p, std::max<size_t>(bytes, 256), st));
  return GMR_OK;
}
int scratch_alloc(gmr_model *m, CallScratch &sc, size_t bytes, hipStream_t st) { return scratch_alloc(m, sc, bytes, st, m->err); }

// The members of a member-wise call (motion_run, track_run, report_run): a group's models, or one model as a group of one.
// Errors land in `err`; a group call names the member in its messages.
struct Members {
  gmr_model *const *models;
  int n, device;
  bool group;
  std::string &err;
  std::string who(int i) const { return group ? "member " + std::to_string(i) + ": " : ""; }
};

// The single form (m) and the group form (g) of a member-wise entry: `run` takes the Members.
template <class In, class Run>
int member_call(gmr_model *m, gmr_group *g, const In *inputs, Run run) {
  if (!m && !g) return GMR_EINVAL;
  std::string &err = g ? g->err : m->err;
  err.clear();
  if (!inputs) { err = g ? "null inputs" : "null input"; return GMR_EINVAL; }
  if (g) return run(Members{g->models.data(), (int)g->models.size(), g->device, true, err});
  return run(Members{&m, 1, m->device, false, err});
}

// The HIP half of a call block (call_block.h): one stream-ordered allocation (from the first member's pool), then `fill`, which
// writes into the host image what needs the block's device address, then one copy of the uploaded prefix.
template <class Fill>
int send_call_block(const Members &g, gmr::CallBlock &blk, CallScratch &sc, hipStream_t st, Fill fill) {
  gmr_model *m0 = g.models[0];
  if (scratch_alloc(m0, sc, blk.total_bytes(), st) != GMR_OK) { g.err = m0->err; return GMR_EDEVICE; }
  const int rc = fill(blk.on(sc.p));
  if (rc != GMR_OK) return rc;
  if (hipMemcpyAsync(sc.p, blk.image(), blk.uploaded_bytes(), hipMemcpyHostToDevice, st) != hipSuccess) { g.err = "hipMemcpyAsync failed"; return GMR_EDEVICE; }
  return GMR_OK;
}

// The rules of a clip-offset table [n_seq + 1] over n_frames rows, NULL or what is wrong: the table's ends, clip s, all of it.
const char *seq_ends_error(const int64_t *offs, int n_seq, int64_t n_frames) {
  return !offs || n_seq < 1 || offs[0] != 0 || offs[n_seq] != n_frames ? "seq_offsets must run from 0 to n_frames" : nullptr;
}
const char *seq_clip_error(const int64_t *offs, int s) { return offs[s + 1] < offs[s] ? "seq_offsets must not decrease" : nullptr; }
const char *seq_offsets_error(const int64_t *offs, int n_seq, int64_t n_frames) {
  const char *why = seq_ends_error(offs, n_seq, n_frames);
  for (int s = 0; !why && s < n_seq; ++s) why = seq_clip_error(offs, s);
  return why;
}

// The kernel variants (GMR_FOR_EACH_NVP), the shaped instances (GMR_FOR_EACH_IK_SHAPE) and the match of a model against them live in
// model_plan.h: planning a model needs them.
using gmr::ik_shape_name;
using gmr::ik_shape_of;

// The instance a launch takes: the model's shape where the launch is what `plain` stands for in a shape (float32 key-points, no
// offset_to_ground, every item plain, no step cap), else -1 = the generic instance.  This is the only guard: a shape with `plain`
// compiled in (IkShapeG1Smplx) has no code for float64 input, offset_to_ground, the verification walk or the chunk start.
int ik_launch_shape(int model_shape, bool force_generic_shape, bool plain, bool in_f64, bool offset_to_ground, bool capped) {
  return model_shape >= 0 && !force_generic_shape && plain && !in_f64 && !offset_to_ground && !capped ? model_shape : -1;
}

// plain: every item of the launch is a plain one (no verification walk, no speculative chunk start; ik_run).  A shaped instance runs
// only where the model matched its shape (m->shape) AND the launch is what the shape's `plain` stands for; it does not re-check.
template <int NVP>
void launch_ik(const gmr_model *m, const gmr::IkLaunch &L, hipStream_t st, bool probe, bool plain) {
  const bool sq = m->dm.sq_ok && !m->force_generic;
  const int shape = sq ? ik_launch_shape(m->shape, m->force_generic_shape, plain, L.in_f64 != 0, L.prm.offset_to_ground != 0, L.step_cap != nullptr) : -1;
  if (getenv("GMR_DEBUG_PLAN")) fprintf(stderr, "gmr: ik launch: %s instance %s\n", probe ? "probe" : "solve", ik_shape_name(shape));
  if (shape >= 0) {
    int idx = 0;
#define GMR_X(S, v)                                                                                                                      \
  if constexpr (NVP == v) {                                                                                                              \
    if (shape == idx) {                                                                                                                  \
      if (probe) hipLaunchKernelGGL((gmr::ik_probe_kernel<NVP, gmr::S>), dim3(L.n_items), dim3(64), m->lds_bytes, st, m->dm_dev, L, m->lay); \
      else hipLaunchKernelGGL((gmr::ik_kernel<NVP, gmr::S>), dim3(L.n_items), dim3(64), m->lds_bytes, st, m->dm_dev, L, m->lay);           \
      return;                                                                                                                            \
    }                                                                                                                                    \
  }                                                                                                                                      \
  ++idx;
    GMR_FOR_EACH_IK_SHAPE(GMR_X)
#undef GMR_X
    (void)idx;
  }
  if (probe) {
    if (sq) hipLaunchKernelGGL((gmr::ik_probe_kernel<NVP, true>), dim3(L.n_items), dim3(64), m->lds_bytes, st, m->dm_dev, L, m->lay);
#ifndef GMR_IK_DEV_ONLY36
    else hipLaunchKernelGGL((gmr::ik_probe_kernel<NVP, false>), dim3(L.n_items), dim3(64), m->lds_bytes, st, m->dm_dev, L, m->lay);
#endif
    return;
  }
  if (sq)
    hipLaunchKernelGGL((gmr::ik_kernel<NVP, true>), dim3(L.n_items), dim3(64), m->lds_bytes, st, m->dm_dev, L, m->lay);
#ifndef GMR_IK_DEV_ONLY36
  else
    hipLaunchKernelGGL((gmr::ik_kernel<NVP, false>), dim3(L.n_items), dim3(64), m->lds_bytes, st, m->dm_dev, L, m->lay);
#endif
}

int launch_ik_variant(gmr_model *m, const gmr::IkLaunch &L, hipStream_t st, bool probe = false, bool plain = false) {
  switch (m->nvp) {
#define GMR_X(v) case v: launch_ik<v>(m, L, st, probe, plain); break;
    GMR_FOR_EACH_NVP(GMR_X)
#undef GMR_X
    default: set_err(m, "internal: no kernel variant for nvp=%d", m->nvp); return GMR_EUNSUPPORTED;
  }
  HIP_TRY(m, hipGetLastError());
  return GMR_OK;
}

// The sliced launch of a plain batch (ik_kernel_sliced): `grid` = n_items x rounds one-wavefront workgroups; same choice of instance
// as launch_ik.
template <int NVP>
void launch_ik_sliced(const gmr_model *m, const gmr::IkLaunch &L, const gmr::IkSliceArgs &S, unsigned grid, hipStream_t st, bool plain) {
  const bool sq = m->dm.sq_ok && !m->force_generic;
  const int shape = sq ? ik_launch_shape(m->shape, m->force_generic_shape, plain, L.in_f64 != 0, L.prm.offset_to_ground != 0, L.step_cap != nullptr) : -1;
  if (getenv("GMR_DEBUG_PLAN")) {
    std::string taper = S.plan.n_taper > 0 ? ", taper" : ", no taper";  // the taper's slice lengths, in order
    for (int j = 0; j < S.plan.n_taper; ++j) taper += " " + std::to_string(S.plan.taper_end[j] - (j ? S.plan.taper_end[j - 1] : S.plan.t_body));
    fprintf(stderr, "gmr: ik launch: sliced instance %s, slice %d frames, %u tickets for %d items%s\n", ik_shape_name(shape), S.plan.slice_len, grid,
            L.n_items, taper.c_str());
  }
  if (shape >= 0) {
    int idx = 0;
#define GMR_X(SH, v)                                                                                                                   \
  if constexpr (NVP == v) {                                                                                                            \
    if (shape == idx) {                                                                                                                \
      hipLaunchKernelGGL((gmr::ik_kernel_sliced<NVP, gmr::SH>), dim3(grid), dim3(64), m->lds_bytes, st, m->dm_dev, L, m->lay, S);          \
      return;                                                                                                                          \
    }                                                                                                                                  \
  }                                                                                                                                    \
  ++idx;
    GMR_FOR_EACH_IK_SHAPE(GMR_X)
#undef GMR_X
    (void)idx;
  }
  if (sq)
    hipLaunchKernelGGL((gmr::ik_kernel_sliced<NVP, true>), dim3(grid), dim3(64), m->lds_bytes, st, m->dm_dev, L, m->lay, S);
#ifndef GMR_IK_DEV_ONLY36
  else
    hipLaunchKernelGGL((gmr::ik_kernel_sliced<NVP, false>), dim3(grid), dim3(64), m->lds_bytes, st, m->dm_dev, L, m->lay, S);
#endif
}

// Slice length in frames.  Swept on the headline batch (8192 x 3000 frames, profiles/sliced_slice_sweep.md): 32 / 64 / 128 / 256 / 512
// frames take 516.3 / 515.4 / 513.6 / 518.3 / 525.3 ms against 539.0 ms for probe + ordered launch -- shorter slices shorten the
// last round's tail, longer ones pay the per-slice set-up less often.  256, not 128: with the four-slice rule below a 128-frame
// slice would also take the batches of 512 .. 1023 frames, for which nothing was measured and which the probe policy serves
// (Engine.PROBE_*, measured down to 300 frames).
constexpr int kBalanceSlice = 256;
// Taper floor in frames, 0 = off: the last kBalanceSlice frames of the longest clip run as halving slices down to this length
// (slice_plan.h), which takes the short last round of a short slice without its set-ups over the whole clip.  Swept on the headline
// batch (profiles/slice_taper_sweep.md): off / 128 / 64 / 32 / 16 / 8 take 508.6 / 506.5 / 503.2 / 502.1 / 501.3 / 499.8 ms, a uniform
// 128-frame slice 504.1 ms.  16, not 8: over both visits' rows the two are within the spread of repeated rows (500.7 .. 501.3 against
// 499.8 .. 501.0 ms), and 16 draws fewer tickets: 256 frames end as 128 64 32 16 16, 16 rounds on 3000 frames against 12.
constexpr int kBalanceTaperFloor = 16;
constexpr bool kBalanceDefault = true;          // without GMR_AMD_BALANCE: take the sliced path where the plan says it pays
constexpr double kBalanceMaxLengthSpread = 0.10;  // "equal lengths": the band Engine.PROBE_MAX_LENGTH_SPREAD uses
constexpr int kBalanceMinSlices = 4;            // mean item length, in slices, from which slicing pays
// Slice length of a batch, 0 = whole-clip launch: see gmr_ik_balance_plan (gmr_amd.h).
int balance_plan(const gmr_work_item *items, int n_items, int slots) {
  if (!items || n_items <= 0) return 0;
  const char *sw = getenv("GMR_AMD_BALANCE");
  const int mode = sw && sw[0] == '0' ? 0 : sw && sw[0] == '1' ? 1 : sw && sw[0] == '2' ? 2 : (kBalanceDefault ? 2 : 0);  // 0 off, 1 forced, 2 where it pays
  if (mode == 0) return 0;
  const int slice = (int)gmr::env_int("GMR_AMD_BALANCE_SLICE", 1, INT32_MAX, kBalanceSlice);
  double sum = 0.0, sum2 = 0.0;
  for (int i = 0; i < n_items; ++i) {
    const gmr_work_item &w = items[i];
    if (w.check_stride != 0 || w.n_burn != 0 || w.init_row == GMR_INIT_ROOT_TARGET || w.n_out < 0) return 0;  // plain items only
    sum += w.n_out; sum2 += (double)w.n_out * w.n_out;
  }
  if (mode == 1) return slice;
  if (n_items <= slots) return 0;  // everything starts at once: nothing to balance
  const double mean = sum / n_items, var = std::max(0.0, sum2 / n_items - mean * mean);
  if (std::sqrt(var) > kBalanceMaxLengthSpread * mean) return 0;  // unequal lengths: round-robin would leave the long clips to finish alone
  if (mean < (double)kBalanceMinSlices * slice) return 0;
  return slice;
}

int launch_ik_sliced_variant(gmr_model *m, const gmr::IkLaunch &L, const gmr::IkSliceArgs &S, unsigned grid, hipStream_t st, bool plain) {
  switch (m->nvp) {
#define GMR_X(v) case v: launch_ik_sliced<v>(m, L, S, grid, st, plain); break;
    GMR_FOR_EACH_NVP(GMR_X)
#undef GMR_X
    default: set_err(m, "internal: no kernel variant for nvp=%d", m->nvp); return GMR_EUNSUPPORTED;
  }
  HIP_TRY(m, hipGetLastError());
  return GMR_OK;
}

// perm: NULL or the global launch order (gmr_group_ik_solve_ordered); probe: the cost probe (gmr_group_plan_order)
template <int NVP>
void launch_ik_group(const gmr_group *g, const gmr::IkGroupEntry *entries, const int *block_entry, int n_blocks, int lds_bytes, hipStream_t st,
                     const int *perm = nullptr, bool probe = false) {
  if (probe) {
    if (g->sq) hipLaunchKernelGGL((gmr::ik_group_probe_kernel<NVP, true>), dim3(n_blocks), dim3(64), lds_bytes, st, entries, block_entry);
#ifndef GMR_IK_DEV_ONLY36
    else hipLaunchKernelGGL((gmr::ik_group_probe_kernel<NVP, false>), dim3(n_blocks), dim3(64), lds_bytes, st, entries, block_entry);
#endif
    return;
  }
  if (g->sq)
    hipLaunchKernelGGL((gmr::ik_group_kernel<NVP, true>), dim3(n_blocks), dim3(64), lds_bytes, st, entries, block_entry, perm, n_blocks);
#ifndef GMR_IK_DEV_ONLY36
  else
    hipLaunchKernelGGL((gmr::ik_group_kernel<NVP, false>), dim3(n_blocks), dim3(64), lds_bytes, st, entries, block_entry, perm, n_blocks);
#endif
}


template <int NVP>
void launch_ik_session(const gmr_model *m, const gmr::IkGroupEntry *entries, gmr::IkSessionBox *box, unsigned long long idle_ticks,
                       unsigned max_polls, unsigned max_frames, unsigned gen, hipStream_t st) {
  if (m->dm.sq_ok && !m->force_generic)
    hipLaunchKernelGGL((gmr::ik_session_kernel<NVP, true>), dim3(1), dim3(64), m->lds_bytes, st, entries, box, idle_ticks, max_polls, max_frames, gen);
#ifndef GMR_IK_DEV_ONLY36
  else
    hipLaunchKernelGGL((gmr::ik_session_kernel<NVP, false>), dim3(1), dim3(64), m->lds_bytes, st, entries, box, idle_ticks, max_polls, max_frames, gen);
#endif
}

// The host's copy of what a plan (model_plan.h) says of a model; no device pointer yet.
void adopt_plan(gmr_model *m, const gmr::ModelPlan &p) {
  m->dm = p.dm;
  m->lay = p.lay; m->lay_eval = p.lay_eval;
  m->lds_bytes = p.lds_bytes; m->lds_bytes_eval = p.lds_bytes_eval;
  m->nvp = p.nvp; m->n_act = p.n_act; m->shape = p.shape;
  m->fk_lds_bytes = p.fk_lds_bytes; m->fk_lds_bytes_min = p.fk_lds_bytes_min;
}

// Plan the model on the host (model_plan.h), then: one device allocation, the image's handles resolved into the handle's tables, one
// copy, and the opt-in to more than 64 KiB of dynamic LDS.
int build_device_model(gmr_model *m) {
  gmr::ModelPlan plan;
  const int rc = gmr::plan_model(m->blob.data(), m->blob.size(), m->min_nvp, m->force_generic, plan, m->err);
  if (rc != GMR_OK) return rc;
  adopt_plan(m, plan);
  gmr::ModelImage &I = plan.image;
  HIP_TRY(m, hipMalloc(&m->dev, I.block.total_bytes()));
  m->dev_bytes = I.block.total_bytes();
  const gmr::CallBlock::Device D = I.block.on(m->dev);
  m->dm_dev = D(I.dm);
  m->dm_eval_dev = D(I.dm_eval);
  gmr::FkTree &fk = m->fk;
  fk.parent = D(I.parent); fk.dofidx = D(I.dofidx); fk.src_slot = D(I.src_slot); fk.save_slot = D(I.save_slot);
  fk.lpos = D(I.lpos); fk.lrot = D(I.lrot); fk.jaxis = D(I.jaxis); fk.jaxis64 = D(I.jaxis64); fk.body = D(I.fkbody);
  fk.nbody = m->h.nbody; fk.ndof = m->h.nq - 7; fk.nslots = plan.nslots; fk.dof_in_order = plan.dof_in_order;
  m->kin.dof_body = D(I.k_dof_body); m->kin.lim_lo = D(I.k_lo); m->kin.lim_hi = D(I.k_hi);
  m->kin.depth = D(I.k_depth); m->kin.order = D(I.k_order);
  m->kin.max_depth = plan.k_maxd;
  m->rep_lo = D(I.rep_lo); m->rep_hi = D(I.rep_hi);
  HIP_TRY(m, hipMemcpy(m->dev, I.block.image(), I.block.uploaded_bytes(), hipMemcpyHostToDevice));

  if (m->lds_bytes > 160 * 1024) { set_err(m, "model needs %d bytes of LDS per wavefront", m->lds_bytes); return GMR_EUNSUPPORTED; }
  // opt in to > 64 KiB of dynamic LDS where a variant needs it
#define GMR_LDS_OPT_IN(k) hipFuncSetAttribute(reinterpret_cast<const void *>(&k), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
#ifdef GMR_IK_DEV_ONLY36
#define GMR_X(v) GMR_LDS_OPT_IN((gmr::ik_kernel<v, true>)) GMR_LDS_OPT_IN((gmr::ik_probe_kernel<v, true>)) GMR_LDS_OPT_IN((gmr::ik_group_kernel<v, true>)) GMR_LDS_OPT_IN((gmr::ik_group_probe_kernel<v, true>)) \
  GMR_LDS_OPT_IN((gmr::ik_session_kernel<v, true>))
#else
#define GMR_X(v)                                                                                                                         \
  GMR_LDS_OPT_IN((gmr::ik_kernel<v, false>)) GMR_LDS_OPT_IN((gmr::ik_kernel<v, true>)) GMR_LDS_OPT_IN((gmr::ik_probe_kernel<v, false>))       \
  GMR_LDS_OPT_IN((gmr::ik_probe_kernel<v, true>)) GMR_LDS_OPT_IN((gmr::ik_group_kernel<v, false>)) GMR_LDS_OPT_IN((gmr::ik_group_kernel<v, true>)) \
  GMR_LDS_OPT_IN((gmr::ik_group_probe_kernel<v, false>)) GMR_LDS_OPT_IN((gmr::ik_group_probe_kernel<v, true>))                            \
  GMR_LDS_OPT_IN((gmr::ik_session_kernel<v, false>)) GMR_LDS_OPT_IN((gmr::ik_session_kernel<v, true>))
#endif
  GMR_FOR_EACH_NVP(GMR_X)
#undef GMR_X
#define GMR_X(S, v) GMR_LDS_OPT_IN((gmr::ik_kernel<v, gmr::S>)) GMR_LDS_OPT_IN((gmr::ik_probe_kernel<v, gmr::S>))
  GMR_FOR_EACH_IK_SHAPE(GMR_X)
#undef GMR_X
  GMR_LDS_OPT_IN(gmr::eval_kernel)
  GMR_LDS_OPT_IN(gmr::fk_pos_kernel<1>) GMR_LDS_OPT_IN(gmr::fk_pos_kernel<2>)
  GMR_LDS_OPT_IN(gmr::fk_kernel<0>) GMR_LDS_OPT_IN(gmr::fk_kernel<1>)
  GMR_LDS_OPT_IN(gmr::motion_epilogue_kernel)
  GMR_LDS_OPT_IN(gmr::motion_track_kernel)
  GMR_LDS_OPT_IN(gmr::motion_sample_kernel)
  GMR_LDS_OPT_IN(gmr::clip_report_kernel)
  GMR_LDS_OPT_IN(gmr::motion_transitions_pair_kernel<8>) GMR_LDS_OPT_IN(gmr::motion_transitions_pair_kernel<gmr::kTrMaxWindow>)
#undef GMR_LDS_OPT_IN
  (void)hipGetLastError();
  return GMR_OK;
}

}  // namespace

extern "C" {

int gmr_abi_version(void) { return GMR_ABI_VERSION; }

static gmr_model *model_create_impl(const void *blob, size_t blob_bytes, int device, int min_nvp, int force_generic, char *err, size_t err_len) {
  auto fail = [&](gmr_model *m, const char *msg) -> gmr_model * {
    if (err && err_len) snprintf(err, err_len, "%s", m && !m->err.empty() ? m->err.c_str() : msg);
    if (m) gmr_model_destroy(m);
    return nullptr;
  };
  gmr_blob_header h;
  std::string blob_err;
  if (gmr::validate_blob(blob, blob_bytes, h, blob_err) != GMR_OK) return fail(nullptr, blob_err.c_str());

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, "no HIP device available (libgmr_amd has no CPU path)");
  if (device < 0 || device >= ndev) return fail(nullptr, "device ordinal out of range");
  gmr_model *m = new gmr_model();
  m->device = device;
  m->h = h;
  m->blob.assign(static_cast<const uint8_t *>(blob), static_cast<const uint8_t *>(blob) + blob_bytes);
  if (hipSetDevice(device) != hipSuccess) return fail(m, "hipSetDevice failed");
  {  // what a sliced launch needs beside its per-call scratch, made here so that gmr_ik_solve allocates nothing outside its stream
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) return fail(m, "hipDeviceGetAttribute failed");
    m->slots = 8 * cus;  // two wavefronts per SIMD
    void *d = nullptr;
    if (hipHostMalloc(reinterpret_cast<void **>(&m->slice_err), 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return fail(m, "hipHostMalloc failed");
    memset(m->slice_err, 0, 64);
    if (hipHostGetDevicePointer(&d, m->slice_err, 0) != hipSuccess) return fail(m, "hipHostGetDevicePointer failed");
    m->slice_err_dev = static_cast<unsigned *>(d);
  }
  m->pool = scratch_pool(device);  // (nullptr: no pool support on this runtime -- per-call scratch then comes from the device's default pool as it is)
  if (const char *e = getenv("GMR_AMD_GENERIC_QP")) m->force_generic = e[0] == '1';
  if (force_generic) m->force_generic = true;
  if (const char *e = getenv("GMR_AMD_GENERIC_SHAPE")) m->force_generic_shape = e[0] == '1';
  m->min_nvp = min_nvp;
  if (const char *e = getenv("GMR_AMD_FK_PARTS")) m->fk_pos_parts = e[0] == '0' ? 0 : e[0] == '2' ? 2 : 1;
  if (build_device_model(m) != GMR_OK) return fail(m, "model build failed");
  return m;
}

gmr_model *gmr_model_create(const void *blob, size_t blob_bytes, int device, char *err, size_t err_len) {
  return model_create_impl(blob, blob_bytes, device, 0, 0, err, err_len);
}

void gmr_model_destroy(gmr_model *m) {
  if (!m) return;
  if (m->device >= 0) (void)hipSetDevice(m->device);
  if (m->dev) (void)hipFree(m->dev);
  if (m->slice_err) (void)hipHostFree(m->slice_err);
  if (m->dbg) (void)hipFree(m->dbg);
  if (m->cap_dev) (void)hipFree(m->cap_dev);
  delete m;
}

const char *gmr_last_error(const gmr_model *m) { return m ? m->err.c_str() : "null model"; }

int gmr_model_set_step_cap(gmr_model *m, const double *cap) {
  if (!m) return GMR_EINVAL;
  m->err.clear();
  if (!cap) { m->cap_host.clear(); return GMR_OK; }
  const int nv = m->h.nv;
  for (int k = 0; k < nv; ++k) {
    if (!(cap[k] > 0.0)) { set_err(m, "step cap of dof %d must be > 0 or +inf", k); return GMR_EINVAL; }
    if (k < 6 && std::isfinite(cap[k])) { set_err(m, "the root's dofs (dof %d) cannot be capped", k); return GMR_EINVAL; }
  }
  // by active dof, as the kernel's lanes index it: a hinge row takes its dof's entry (dof = qpos address - 1 behind a free joint);
  // the root's six rows (null dofs of a planar base among them) and the padding stay +inf
  double rows[64];
  for (int a = 0; a < 64; ++a) rows[a] = a < m->n_act && m->dm.akind[a] == 6 ? cap[m->dm.aqadr[a] - 1] : INFINITY;
  HIP_TRY(m, hipSetDevice(m->device));
  if (!m->cap_dev) HIP_TRY(m, hipMalloc(reinterpret_cast<void **>(&m->cap_dev), sizeof(rows)));
  HIP_TRY(m, hipMemcpy(m->cap_dev, rows, sizeof(rows), hipMemcpyHostToDevice));
  m->cap_host.assign(cap, cap + nv);
  return GMR_OK;
}

int gmr_model_get_step_cap(const gmr_model *m, double *cap_out) {
  if (!m || !cap_out) return GMR_EINVAL;
  for (int k = 0; k < m->h.nv; ++k) cap_out[k] = m->cap_host.empty() ? INFINITY : m->cap_host[k];
  return GMR_OK;
}

int gmr_model_info_get(const gmr_model *m, gmr_model_info *out) {
  if (!m || !out) return GMR_EINVAL;
  memset(out, 0, sizeof(*out));
  out->nbody = m->h.nbody; out->nq = m->h.nq; out->nv = m->h.nv; out->nslot = m->h.nslot;
  out->ntask[0] = m->h.ntask[0]; out->ntask[1] = m->h.ntask[1];
  out->n_active_dof = m->n_act; out->nv_padded = m->nvp; out->lds_bytes = m->lds_bytes; out->device = m->device;
  out->reserved[0] = m->dm.sq_ok && !m->force_generic ? 16 - m->dm.sq_nlimb : 0;  // core size of the structured QP, 0 = generic QP
  return GMR_OK;
}

// Debug / test hook, host only (no device is touched, so it works on a machine without one; not part of gmr_amd.h): builds the model
// of a blob as gmr_model_create does (model_plan.h) and reports which kernel instance a launch of it would take.
// alter_field >= 0: first add alter_delta to that shape field (in GMR_IK_SHAPE_FIELDS order) of the host model; the four indices behind the fields
// (15 .. 18) add it to one word of table 1 that stage_tables_shared compares: tbody[0], tslot[0], acomp[0], comp_plan[0].x.  launch flags as
// launch_ik sees them.  fields_out: NULL or room for 16 ints, receives the (altered) shape fields.  name_out receives the instance's
// name ("generic" or the shape's).  Returns the shape's index, -1 for the generic instance, -2 on a blob that does not validate (its
// header, or an array that does not lie inside it), -3 on one that does not plan.
int gmr_debug_ik_shape(const void *blob, size_t blob_bytes, int force_generic, int alter_field, int alter_delta, int in_f64,
                       int offset_to_ground, int plain, int *fields_out, char *name_out, size_t name_len) {
  gmr_blob_header h;
  std::string why;
  if (gmr::validate_blob(blob, blob_bytes, h, why) != GMR_OK) return -2;
  gmr::ModelPlan plan;
  if (gmr::plan_model(blob, blob_bytes, 0, force_generic != 0, plan, why) != GMR_OK) return -3;
  gmr::DevModel &d = plan.dm;
  int k = 0;
#define GMR_X(f, e) if (k++ == alter_field) (e) += alter_delta;
  GMR_IK_SHAPE_FIELDS(GMR_X)
#undef GMR_X
  // behind the fields: one equality of stage_tables_shared each, broken in table 1 (its first task's body and slot, the composite of
  // its first active dof, the first word of its composite plan)
  if (alter_field == k) d.tbody[GMR_MAX_TASKS] += alter_delta;
  if (alter_field == k + 1) d.tslot[GMR_MAX_TASKS] += alter_delta;
  if (alter_field == k + 2) d.acomp[64] += alter_delta;
  if (alter_field == k + 3) d.comp_plan[4 * gmr::kMaxCompPass].x += (unsigned)alter_delta;
  k = 0;
#define GMR_X(f, e) if (fields_out) fields_out[k++] = (e);
  GMR_IK_SHAPE_FIELDS(GMR_X)
#undef GMR_X
  const bool sq = d.sq_ok && !force_generic;
  const int shape = ik_launch_shape(ik_shape_of(d, plan.nvp, sq), false, plain != 0, in_f64 != 0, offset_to_ground != 0, false);
  if (name_out && name_len) snprintf(name_out, name_len, "%s", ik_shape_name(shape));
  return shape;
}

// Validate one model's batch (`in`: its arguments exactly as gmr_ik_solve takes them), put its scheduling data (length-sorted work
// items, the caller's index of each, the slot columns) into stream-ordered scratch and fill the launch arguments.
static int prepare_ik_launch(gmr_model *m, const gmr_group_input &in, const gmr_ik_params *params, gmr_ik_stats *stats, hipStream_t st,
                             CallScratch &sc, gmr::IkLaunch &L, std::vector<gmr_work_item> &sorted, bool keep_order) {
  const gmr_work_item *items = in.items;
  const int32_t *slot_col = in.slot_col;
  const int n_items = in.n_items, n_cols = in.n_cols;
  if (m->h.nslot == 0 || (m->h.ntask[0] == 0 && m->h.ntask[1] == 0)) { set_err(m, "model has no IK config"); return GMR_ENOCONFIG; }
  if (!in.human_pos || !in.human_quat || !slot_col || !params || !in.qpos_out || (!items && n_items > 0)) { set_err(m, "null argument"); return GMR_EINVAL; }
  if (in.in_dtype != GMR_DTYPE_F32 && in.in_dtype != GMR_DTYPE_F64) { set_err(m, "in_dtype must be f32 or f64"); return GMR_EINVAL; }
  if (n_cols <= 0 || in.n_frames < 0 || n_items < 0) { set_err(m, "negative size"); return GMR_EINVAL; }
  if (params->max_iter < 0 || !(params->damping > 0.0)) { set_err(m, "damping must be > 0 (H must be positive definite) and max_iter >= 0"); return GMR_EINVAL; }
  for (int s = 0; s < m->h.nslot; ++s)
    if (slot_col[s] < 0 || slot_col[s] >= n_cols) { set_err(m, "slot_col[%d]=%d outside [0,%d)", s, slot_col[s], n_cols); return GMR_EINVAL; }
  int64_t tot = 0, out = 0;
  bool need_init = false, need_final = false;
  for (int i = 0; i < n_items; ++i) {
    const gmr_work_item &w = items[i];
    if (w.n_burn < 0 || w.n_out < 0 || w.frame_begin < 0 || w.frame_begin + w.n_burn + w.n_out > in.n_frames) {
      set_err(m, "work item %d covers frames outside [0,%lld)", i, (long long)in.n_frames);
      return GMR_EINVAL;
    }
    if (w.check_stride < 0 || (w.check_stride > 0 && (w.burn_row < 0 || w.final_row < 0 || w.n_burn != 0))) {
      set_err(m, "work item %d: a verification walk (check_stride) needs burn_row, final_row and n_burn = 0", i);
      return GMR_EINVAL;
    }
    if (w.init_row < GMR_INIT_ROOT_TARGET || !(w.height_scale >= 0.0) || !std::isfinite(w.height_scale)) {
      set_err(m, "work item %d: init_row must be a row, GMR_INIT_QPOS0 or GMR_INIT_ROOT_TARGET, and height_scale finite and >= 0", i);
      return GMR_EINVAL;
    }
    tot += w.n_burn + w.n_out; out += w.n_out;
    need_init |= w.init_row >= 0; need_final |= w.final_row >= 0 || w.burn_row >= 0;
  }
  if (need_init && !in.qpos_init) { set_err(m, "items reference qpos_init but it is NULL"); return GMR_EINVAL; }
  if (need_final && !in.qpos_final) { set_err(m, "items reference qpos_final but it is NULL"); return GMR_EINVAL; }
  if (stats) { memset(stats, 0, sizeof(*stats)); stats->n_items = n_items; stats->n_frames_total = tot; stats->n_frames_out = out; }
  L = gmr::IkLaunch{};
  L.n_items = n_items;
  sorted.clear();
  if (n_items == 0) return GMR_OK;  // (before any device call)

  HIP_TRY(m, hipSetDevice(m->device));
  // longest item first so that the tail of the grid is made of short ones
  std::vector<int> order(n_items);
  std::iota(order.begin(), order.end(), 0);
  if (!keep_order)  // (an ordered launch brings its own order: gmr_ik_solve_ordered)
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return items[a].n_burn + items[a].n_out > items[b].n_burn + items[b].n_out; });
  sorted.resize(n_items);
  for (int i = 0; i < n_items; ++i) sorted[i] = items[order[i]];
  const size_t items_bytes = sizeof(gmr_work_item) * (size_t)n_items, col_bytes = sizeof(int32_t) * (size_t)m->h.nslot;
  const size_t order_off = (items_bytes + 15) & ~size_t(15), order_bytes = sizeof(int) * (size_t)n_items;
  const size_t col_off = (order_off + order_bytes + 15) & ~size_t(15);
  int rc = scratch_alloc(m, sc, col_off + col_bytes, st);
  if (rc != GMR_OK) return rc;
  uint8_t *ws = static_cast<uint8_t *>(sc.p);
  // The sources are pageable host memory (vectors that die with the call, the caller's own slot_col).  Observed on ROCm 7 behind a
  // busy stream (tests/test_gpu_stream_order.py): hipMemcpyAsync takes its copy of the bytes when it is called -- the
  // sources may be overwritten or freed as soon as it returns -- and up to 512 KiB it does not wait for the stream; at 1 MiB it
  // returns only when the earlier work on the stream has finished.  Every table copy in this file relies on the first part.
  HIP_TRY(m, hipMemcpyAsync(ws, sorted.data(), items_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(m, hipMemcpyAsync(ws + order_off, order.data(), order_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(m, hipMemcpyAsync(ws + col_off, slot_col, col_bytes, hipMemcpyHostToDevice, st));

  L.hpos = in.human_pos; L.hquat = in.human_quat; L.slot_col = reinterpret_cast<const int *>(ws + col_off);
  L.items = reinterpret_cast<const gmr_work_item *>(ws);
  L.order = reinterpret_cast<const int *>(ws + order_off); L.frames_done = in.frames_done;
  L.qinit = in.qpos_init; L.qfinal = in.qpos_final; L.qout = in.qpos_out; L.iters = in.iters_out;
  L.in_f64 = in.in_dtype == GMR_DTYPE_F64; L.n_cols = n_cols; L.n_items = n_items; L.prm = *params;
#ifdef GMR_IK_STAMPS
  if (!m->dbg) { HIP_TRY(m, hipMalloc(&m->dbg, 16 * sizeof(unsigned long long))); HIP_TRY(m, hipMemset(m->dbg, 0, 16 * sizeof(unsigned long long))); }
#endif
  L.dbg = m->dbg;
  L.step_cap = m->step_cap();
  return GMR_OK;
}

// The probe copy of a batch (gmr_ik_plan_order): every item cut to its first probe_frames frames, solved for their cost alone.
// `in` is redirected to the copy and loses its outputs; frames[k] / probed[k] receive item k's frames in total / in the probe.
static int probe_batch(gmr_group_input &in, int probe_frames, std::vector<gmr_work_item> &probe, int *frames, int *probed, std::string &err) {
  static double dummy_out;  // (prepare_ik_launch insists on an output array; a probe item has no output frame to write)
  if (in.n_items < 0 || (!in.items && in.n_items > 0)) { err = "null argument"; return GMR_EINVAL; }
  probe.assign(in.items, in.items + in.n_items);
  for (int k = 0; k < in.n_items; ++k) {
    gmr_work_item &w = probe[k];
    if (w.check_stride != 0) { err = "work item " + std::to_string(k) + ": verification walks cannot be probed"; return GMR_EINVAL; }
    if (w.n_burn < 0 || w.n_out < 0) { err = "work item " + std::to_string(k) + " has a negative frame count"; return GMR_EINVAL; }
    const int total = w.n_burn + w.n_out, p = std::min(total, probe_frames);
    frames[k] = total; probed[k] = p;
    w.n_burn = p; w.n_out = 0; w.final_row = -1; w.burn_row = -1;  // frames solved, nothing written
  }
  in.items = probe.data();
  in.qpos_final = nullptr; in.qpos_out = &dummy_out; in.iters_out = nullptr; in.frames_done = nullptr;
  return GMR_OK;
}

enum IkMode { IK_PLAIN, IK_PROBE, IK_ORDERED };

// The sliced launch of a model's own plain call, where balance_plan says so (`sliced` tells): ticket counter, `done` words and the
// hand-over records in stream-ordered scratch, the first two cleared on the stream in front of the launch.  `sorted`: the items as
// the launch runs them (longest first).
static int ik_run_sliced(gmr_model *m, const gmr::IkLaunch &L, const std::vector<gmr_work_item> &sorted, hipStream_t st, CallScratch &ss,
                         bool plain, bool &sliced) {
  sliced = false;
  const int n_items = (int)sorted.size();
  const int slice = balance_plan(sorted.data(), n_items, m->slots);
  if (slice <= 0) {
    if (getenv("GMR_DEBUG_PLAN")) fprintf(stderr, "gmr: ik launch: whole clips (balance plan 0)\n");
    return GMR_OK;
  }
  const int longest = sorted[0].n_burn + sorted[0].n_out;
  const int taper_floor = (int)gmr::env_int("GMR_AMD_BALANCE_TAPER", 0, INT32_MAX, kBalanceTaperFloor);  // read per call, like the two above
  const gmr::SlicePlan plan = gmr::slice_plan_make(longest, slice, taper_floor);
  const int64_t rounds = gmr::slice_plan_rounds(plan), grid = rounds * n_items;
  const size_t rec = (size_t)m->dm.nq + 7 * (size_t)m->dm.nbody;  // (the kernel's own tree: DevModel::nbody)
  const size_t flag_bytes = (sizeof(unsigned) * ((size_t)n_items + 1) + 15) & ~size_t(15);  // [head | done[n_items]], cleared every call
  const size_t lane_off = flag_bytes, state_off = lane_off + sizeof(int) * 64 * (size_t)n_items;
  const size_t total = state_off + sizeof(double) * rec * (size_t)n_items;
  if (grid > INT32_MAX || total > (size_t(1) << 30)) {  // (beyond one grid or 1 GiB of records: whole clips, as before)
    if (getenv("GMR_DEBUG_PLAN")) fprintf(stderr, "gmr: ik launch: whole clips (sliced launch too large)\n");
    return GMR_OK;
  }
  if (!m->slice_err_dev || m->slots <= 0) { set_err(m, "internal: the handle has no sliced-launch state"); return GMR_EDEVICE; }
  int rc = scratch_alloc(m, ss, total, st);
  if (rc != GMR_OK) return rc;
  uint8_t *ws = static_cast<uint8_t *>(ss.p);
  HIP_TRY(m, hipMemsetAsync(ws, 0, flag_bytes, st));
  gmr::IkSliceArgs S{};
  S.head = reinterpret_cast<unsigned *>(ws);
  S.done = S.head + 1;
  S.timeouts = m->slice_err_dev;
  S.lane_state = reinterpret_cast<int *>(ws + lane_off);
  S.state = reinterpret_cast<double *>(ws + state_off);
  S.plan = plan;
  S.rec_doubles = (int)rec;
  // The poll cap, a guard far beyond the longest wait of a correct run.  With more items than slots a predecessor finished rounds ago; with
  // fewer, ceil(slots / n_items) slices of one clip are resident at once and the last of them waits for the whole chain before it.  2048
  // polls (3-4 us each) per frame waited for, against the 0.05-0.2 ms a frame takes.
  const int64_t chain = std::max<int64_t>(1, std::min<int64_t>(rounds, ((int64_t)m->slots + n_items - 1) / n_items));
  S.max_polls = (unsigned)std::min<int64_t>((int64_t)UINT32_MAX, ((int64_t)1 << 18) + (int64_t)2048 * slice * chain);
  sliced = true;
  return launch_ik_sliced_variant(m, L, S, (unsigned)grid, st, plain);
}

// Every batched IK call.  `models[i]` goes with `inputs[i]`.  With `g` NULL it is a model's own call (n = 1): ik_kernel / ik_probe_kernel
// with the launch arguments by value; with a group, one grid of the ik_group_* kernels over all members' items -- a block finds its
// entry in block_entry[] and its item as its global index - item_base.  Members without work get an empty entry.
//   IK_PLAIN    each member's items longest first, the member with the longest item first
//   IK_ORDERED  items in the caller's order, member i's at base_i = the sum of n_items over the members before it; workgroup b runs
//               global item launch_order[b]
//   IK_PROBE    the first probe_frames frames of every item for their cost (entry i's cost array starts at base_i), then one device
//               sort over all of them into order_out
// Errors land in `err` (a model's call passes its own); a group call names the member.
static int ik_run(const gmr_group *g, gmr_model *const *models, const gmr_group_input *inputs, int n, const gmr_ik_params *params, hipStream_t st,
                  IkMode mode, int probe_frames, int32_t *order_out, const int32_t *launch_order, gmr_ik_stats *stats, std::string &err) {
  auto who = [&](int i) { return g ? "member " + std::to_string(i) + ": " : std::string(); };
  std::vector<gmr_group_input> pin;
  std::vector<std::vector<gmr_work_item>> probe(n), sorted(n);
  std::vector<int> meta;  // IK_PROBE: [cost | frames | probed] by global item index
  int tot = 0;
  if (mode == IK_PROBE) {
    if (!order_out || probe_frames < 1) { err = "order_out is NULL or probe_frames < 1"; return GMR_EINVAL; }
    int64_t total64 = 0;
    for (int i = 0; i < n; ++i) total64 += std::max(0, inputs[i].n_items);
    if (total64 > INT32_MAX) { err = "more than 2^31 - 1 work items in one group launch"; return GMR_EINVAL; }
    tot = (int)total64;
    meta.resize(3 * (size_t)std::max(tot, 1));
    pin.assign(inputs, inputs + n);
    for (int i = 0, base = 0; i < n; ++i) {
      int rc = probe_batch(pin[i], probe_frames, probe[i], meta.data() + tot + base, meta.data() + 2 * (size_t)tot + base, err);
      if (rc != GMR_OK) { err = who(i) + err; return rc; }
      base += pin[i].n_items;
    }
    if (tot == 0) return GMR_OK;
    inputs = pin.data();
  }
  std::vector<CallScratch> scratch(n);
  CallScratch ms, gs, ss;
  std::vector<gmr::IkGroupEntry> entries(n);
  int total = 0, lds_bytes = 0;
  for (int i = 0; i < n; ++i) {
    gmr_model *m = models[i];
    const gmr_group_input &in = inputs[i];
    m->err.clear();
    if (g && in.n_items == 0) continue;  // no work for this member (a model's own call of zero items is still checked)
    int rc = prepare_ik_launch(m, in, params, stats, st, scratch[i], entries[i].L, sorted[i], mode == IK_ORDERED);
    if (rc != GMR_OK) { err = who(i) + m->err; return rc; }
    if (in.n_items > INT32_MAX - total) { err = "more than 2^31 - 1 work items in one group launch"; return GMR_EINVAL; }
    entries[i].m = m->dm_dev; entries[i].lay = m->lay;
    total += in.n_items;
    if (in.n_items > 0) lds_bytes = std::max(lds_bytes, m->lds_bytes);
  }
  if (total == 0) return GMR_OK;
  if (mode == IK_ORDERED && !launch_order) { err = "launch_order is NULL"; return GMR_EINVAL; }
  int *meta_dev = nullptr;
  if (mode == IK_PROBE) {
    int rc = scratch_alloc(models[0], ms, sizeof(int) * meta.size(), st, err);
    if (rc != GMR_OK) return rc;
    meta_dev = static_cast<int *>(ms.p);
    HIP_TRY(err, hipMemcpyAsync(meta_dev, meta.data(), sizeof(int) * meta.size(), hipMemcpyHostToDevice, st));
  }
  std::vector<int> eorder(n), block_entry(g ? total : 0);
  std::iota(eorder.begin(), eorder.end(), 0);
  auto longest = [&](int e) { return sorted[e].empty() ? -1 : sorted[e][0].n_burn + sorted[e][0].n_out; };
  if (mode == IK_PLAIN) std::stable_sort(eorder.begin(), eorder.end(), [&](int a, int b) { return longest(a) > longest(b); });
  int blk = 0;
  for (int e : eorder) {
    entries[e].item_base = blk;
    if (g) std::fill_n(block_entry.begin() + blk, sorted[e].size(), e);
    blk += (int)sorted[e].size();
    if (mode == IK_PROBE) { entries[e].L.qout = nullptr; entries[e].L.cost = meta_dev + entries[e].item_base; }  // (cost[order[k]]: global item base + k)
  }
  if (!g) {
    if (mode == IK_ORDERED) entries[0].L.perm = launch_order;
    bool plain = true;  // (the items were validated in prepare_ik_launch)
    for (const gmr_work_item &w : sorted[0]) plain = plain && w.check_stride == 0 && w.init_row != GMR_INIT_ROOT_TARGET;
    int rc = GMR_OK;
    bool sliced = false;
    if (mode == IK_PLAIN) {  // a plain call of equal-length clips runs as slices drawn by ticket (gmr_ik_balance_plan)
      rc = ik_run_sliced(models[0], entries[0].L, sorted[0], st, ss, plain, sliced);
      if (rc != GMR_OK) { err = models[0]->err; return rc; }
    }
    if (!sliced) rc = launch_ik_variant(models[0], entries[0].L, st, mode == IK_PROBE, plain);
    if (rc != GMR_OK) { err = models[0]->err; return rc; }
  } else {  // the entries and the block -> entry table go into stream-ordered scratch
    const size_t ent_bytes = sizeof(gmr::IkGroupEntry) * (size_t)n, be_off = (ent_bytes + 15) & ~size_t(15);
    int rc = scratch_alloc(models[0], gs, be_off + sizeof(int) * (size_t)total, st, err);
    if (rc != GMR_OK) return rc;
    uint8_t *ws = static_cast<uint8_t *>(gs.p);
    HIP_TRY(err, hipMemcpyAsync(ws, entries.data(), ent_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(err, hipMemcpyAsync(ws + be_off, block_entry.data(), sizeof(int) * (size_t)total, hipMemcpyHostToDevice, st));
    const auto *d_entries = reinterpret_cast<const gmr::IkGroupEntry *>(ws);
    const int *d_be = reinterpret_cast<const int *>(ws + be_off);
    switch (g->nvp) {
#define GMR_X(v) case v: launch_ik_group<v>(g, d_entries, d_be, total, lds_bytes, st, launch_order, mode == IK_PROBE); break;
      GMR_FOR_EACH_NVP(GMR_X)
#undef GMR_X
      default: err = "internal: no kernel variant"; return GMR_EUNSUPPORTED;
    }
    HIP_TRY(err, hipGetLastError());
  }
  if (mode == IK_PROBE) {
    hipLaunchKernelGGL(gmr::plan_order_kernel, dim3(1), dim3(1024), 0, st, meta_dev, meta_dev + tot, meta_dev + 2 * (size_t)tot, tot, order_out);
    HIP_TRY(err, hipGetLastError());
  }
  return GMR_OK;
}

int gmr_ik_solve(gmr_model *m, const void *human_pos, const void *human_quat, int in_dtype, int n_cols, const int32_t *slot_col,
                 int64_t n_frames, const gmr_work_item *items, int n_items, const gmr_ik_params *params, const double *qpos_init,
                 double *qpos_final, double *qpos_out, int32_t *iters_out, int32_t *frames_done, gmr_ik_stats *stats, void *stream) {
  if (!m) return GMR_EINVAL;
  m->err.clear();
  const gmr_group_input in = {human_pos, human_quat, in_dtype, n_cols, slot_col, n_frames, items, n_items, 0,
                              qpos_init, qpos_final, qpos_out, iters_out, frames_done};
  return ik_run(nullptr, &m, &in, 1, params, static_cast<hipStream_t>(stream), IK_PLAIN, 0, nullptr, nullptr, stats, m->err);
}

// Host only: the slice length gmr_ik_solve would run this batch with on a device of `slots` wavefront slots, 0 = whole clips.
int gmr_ik_balance_plan(const gmr_work_item *items, int n_items, int slots) { return balance_plan(items, n_items, slots); }

// Host only: 1 if a wavefront of a sliced launch of this handle has hit its poll cap (the item's remaining frames were not
// written) since the last call, 0 otherwise.  Reads and clears the handle's pinned word; call it after synchronising the stream.
int gmr_ik_sliced_timeouts(gmr_model *m) {
  if (!m || !m->slice_err) return 0;
  volatile unsigned *w = m->slice_err;
  const unsigned v = *w;
  if (v) *w = 0;
  return v != 0;
}

// ---- launch order by predicted cost.  Items of equal length still differ in cost (solves per frame: 1.15 max / mean on the
// bench mix), and with only a few items per wavefront slot the order they start in decides how long the last ones run alone:
// 8192 x 3000 frames take 608 ms in array order and 549 ms most-expensive-first.  Lengths being equal, the only predictor is the
// clip itself: gmr_ik_plan_order solves the first probe_frames of every item for their cost alone (nothing else is written)
// and sorts on the device; gmr_ik_solve_ordered then runs the full items in that order.  Everything stays on the stream.
int gmr_ik_plan_order(gmr_model *m, const void *human_pos, const void *human_quat, int in_dtype, int n_cols, const int32_t *slot_col,
                      int64_t n_frames, const gmr_work_item *items, int n_items, const gmr_ik_params *params, const double *qpos_init,
                      int probe_frames, int32_t *order_out, void *stream) {
  if (!m) return GMR_EINVAL;
  m->err.clear();
  const gmr_group_input in = {human_pos, human_quat, in_dtype, n_cols, slot_col, n_frames, items, n_items, 0,
                              qpos_init, nullptr, nullptr, nullptr, nullptr};
  return ik_run(nullptr, &m, &in, 1, params, static_cast<hipStream_t>(stream), IK_PROBE, probe_frames, order_out, nullptr, nullptr, m->err);
}

int gmr_ik_solve_ordered(gmr_model *m, const void *human_pos, const void *human_quat, int in_dtype, int n_cols, const int32_t *slot_col,
                         int64_t n_frames, const gmr_work_item *items, int n_items, const gmr_ik_params *params, const double *qpos_init,
                         double *qpos_final, double *qpos_out, int32_t *iters_out, int32_t *frames_done, gmr_ik_stats *stats,
                         const int32_t *launch_order, void *stream) {
  if (!m) return GMR_EINVAL;
  m->err.clear();
  if (!launch_order && n_items > 0) { set_err(m, "launch_order is NULL"); return GMR_EINVAL; }
  const gmr_group_input in = {human_pos, human_quat, in_dtype, n_cols, slot_col, n_frames, items, n_items, 0,
                              qpos_init, qpos_final, qpos_out, iters_out, frames_done};
  return ik_run(nullptr, &m, &in, 1, params, static_cast<hipStream_t>(stream), IK_ORDERED, 0, nullptr, launch_order, stats, m->err);
}

// ------------------------------------------------------------------ several models in one launch (BASELINE config 4)
gmr_group *gmr_group_create(const void *const *blobs, const size_t *blob_bytes, int n_models, int device, char *err, size_t err_len) {
  auto fail = [&](gmr_group *g, const char *msg) -> gmr_group * {
    if (err && err_len && msg) snprintf(err, err_len, "%s", msg);
    if (g) gmr_group_destroy(g);
    return nullptr;
  };
  if (!blobs || !blob_bytes || n_models < 1 || n_models > 64) return fail(nullptr, "a group holds 1 .. 64 models");
  gmr_group *g = new gmr_group();
  g->device = device;
  // pass 1: every model as it would be built alone -> the common kernel variant; pass 2: rebuild the members that differ
  int nvp = 0;
  bool all_sq = true;
  for (int i = 0; i < n_models; ++i) {
    gmr_model *m = model_create_impl(blobs[i], blob_bytes[i], device, 0, 0, err, err_len);
    if (!m) return fail(g, nullptr);
    g->models.push_back(m);
    if (m->h.nslot == 0 || (m->h.ntask[0] == 0 && m->h.ntask[1] == 0)) return fail(g, "every group member needs an IK config");
    nvp = std::max(nvp, m->nvp);
    all_sq = all_sq && m->dm.sq_ok && !m->force_generic;
  }
  for (int i = 0; i < n_models; ++i) {
    gmr_model *m = g->models[i];
    const bool sq = m->dm.sq_ok && !m->force_generic;
    if (m->nvp == nvp && sq == all_sq) continue;
    gmr_model_destroy(m);
    g->models[i] = model_create_impl(blobs[i], blob_bytes[i], device, nvp, all_sq ? 0 : 1, err, err_len);
    if (!g->models[i]) return fail(g, nullptr);
    if (g->models[i]->nvp != nvp) return fail(g, "internal: group member did not take the common kernel variant");
  }
  g->nvp = nvp;
  g->sq = all_sq;
  return g;
}

void gmr_group_destroy(gmr_group *g) {
  if (!g) return;
  for (gmr_model *m : g->models) gmr_model_destroy(m);
  delete g;
}

int gmr_group_size(const gmr_group *g) { return g ? (int)g->models.size() : 0; }
gmr_model *gmr_group_model(gmr_group *g, int i) { return g && i >= 0 && i < (int)g->models.size() ? g->models[i] : nullptr; }
const char *gmr_group_last_error(const gmr_group *g) { return g ? g->err.c_str() : "null group"; }

int gmr_group_ik_solve(gmr_group *g, const gmr_group_input *inputs, const gmr_ik_params *params, void *stream) {
  if (!g || !inputs || !params) return GMR_EINVAL;
  g->err.clear();
  return ik_run(g, g->models.data(), inputs, (int)g->models.size(), params, static_cast<hipStream_t>(stream), IK_PLAIN, 0, nullptr, nullptr,
                nullptr, g->err);
}

// Launch order across robots: gmr_ik_plan_order's probe for every member's items in one grid, one device sort over all of them.
int gmr_group_plan_order(gmr_group *g, const gmr_group_input *inputs, const gmr_ik_params *params, int probe_frames, int32_t *order_out,
                         void *stream) {
  if (!g || !inputs || !params) return GMR_EINVAL;
  g->err.clear();
  return ik_run(g, g->models.data(), inputs, (int)g->models.size(), params, static_cast<hipStream_t>(stream), IK_PROBE, probe_frames, order_out,
                nullptr, nullptr, g->err);
}

int gmr_group_ik_solve_ordered(gmr_group *g, const gmr_group_input *inputs, const gmr_ik_params *params, const int32_t *launch_order,
                               void *stream) {
  if (!g || !inputs || !params) return GMR_EINVAL;
  g->err.clear();
  return ik_run(g, g->models.data(), inputs, (int)g->models.size(), params, static_cast<hipStream_t>(stream), IK_ORDERED, 0, nullptr,
                launch_order, nullptr, g->err);
}

// ------------------------------------------------------------------ single-sequence sessions (teleop)

gmr_session *gmr_session_create(gmr_model *m, int in_dtype, int n_cols, const int32_t *slot_col, const gmr_ik_params *params) {
  if (!m) return nullptr;
  m->err.clear();
  if (m->h.nslot == 0 || (m->h.ntask[0] == 0 && m->h.ntask[1] == 0)) { set_err(m, "model has no IK config"); return nullptr; }
  if (!slot_col || !params || n_cols <= 0 || (in_dtype != GMR_DTYPE_F32 && in_dtype != GMR_DTYPE_F64)) { set_err(m, "bad session argument"); return nullptr; }
  if (params->max_iter < 0 || !(params->damping > 0.0)) { set_err(m, "damping must be > 0 and max_iter >= 0"); return nullptr; }
  for (int s = 0; s < m->h.nslot; ++s)
    if (slot_col[s] < 0 || slot_col[s] >= n_cols) { set_err(m, "slot_col[%d]=%d outside [0,%d)", s, slot_col[s], n_cols); return nullptr; }
  gmr_session *s = new gmr_session();
  s->m = m;
  auto fail = [&](const char *what, hipError_t e) -> gmr_session * {
    set_err(m, "%s failed: %s", what, hipGetErrorString(e));
    gmr_session_destroy(s);
    return nullptr;
  };
  hipError_t e;
  if ((e = hipSetDevice(m->device)) != hipSuccess) return fail("hipSetDevice", e);
  if ((e = hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreate", e);
  const size_t elt = in_dtype == GMR_DTYPE_F64 ? 8 : 4, nq = (size_t)m->h.nq;
  s->pos_bytes = (size_t)n_cols * 3 * elt; s->quat_bytes = (size_t)n_cols * 4 * elt;
  s->quat_off = (s->pos_bytes + 15) & ~size_t(15);
  s->out_off = (s->quat_off + s->quat_bytes + 15) & ~size_t(15);
  const size_t box_off = (s->out_off + (nq + 1) * 8 + 63) & ~size_t(63);
  const size_t host_bytes = box_off + sizeof(gmr::IkSessionBox);
  if ((e = hipHostMalloc(reinterpret_cast<void **>(&s->host), host_bytes, hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess) return fail("hipHostMalloc", e);
  memset(s->host, 0, host_bytes);
  void *host_dev = nullptr;
  if ((e = hipHostGetDevicePointer(&host_dev, s->host, 0)) != hipSuccess) return fail("hipHostGetDevicePointer", e);
  const size_t item_off = (nq * 8 + 15) & ~size_t(15), col_off = item_off + sizeof(gmr_work_item);
  const size_t ent_off = (col_off + sizeof(int32_t) * (size_t)m->h.nslot + 15) & ~size_t(15);
  const size_t cap_off = (ent_off + 2 * sizeof(gmr::IkGroupEntry) + 15) & ~size_t(15);  // the model's step cap as it is now: the session keeps its own copy
  if ((e = hipMalloc(reinterpret_cast<void **>(&s->dev), cap_off + 64 * sizeof(double))) != hipSuccess) return fail("hipMalloc", e);
  if (m->step_cap() && (e = hipMemcpy(s->dev + cap_off, m->step_cap(), 64 * sizeof(double), hipMemcpyDeviceToDevice)) != hipSuccess) return fail("hipMemcpy", e);
  gmr_work_item w{};
  w.frame_begin = 0; w.n_burn = 0; w.n_out = 1; w.init_row = 0; w.final_row = 0; w.burn_row = -1; w.height_scale = 1.0;
  if ((e = hipMemcpy(s->dev + item_off, &w, sizeof(w), hipMemcpyHostToDevice)) != hipSuccess) return fail("hipMemcpy", e);
  if ((e = hipMemcpy(s->dev + col_off, slot_col, sizeof(int32_t) * (size_t)m->h.nslot, hipMemcpyHostToDevice)) != hipSuccess) return fail("hipMemcpy", e);
  uint8_t *hd = static_cast<uint8_t *>(host_dev);
  gmr::IkLaunch &L = s->L;
  L.hpos = hd; L.hquat = hd + s->quat_off;
  L.slot_col = reinterpret_cast<const int *>(s->dev + col_off);
  L.items = reinterpret_cast<const gmr_work_item *>(s->dev + item_off);
  L.qinit = reinterpret_cast<const double *>(s->dev); L.qfinal = reinterpret_cast<double *>(s->dev);
  L.qout = reinterpret_cast<double *>(hd + s->out_off); L.iters = reinterpret_cast<int *>(hd + s->out_off + nq * 8);
  L.in_f64 = in_dtype == GMR_DTYPE_F64; L.n_cols = n_cols; L.n_items = 1; L.prm = *params;
  L.dbg = nullptr;
  L.step_cap = m->step_cap() ? reinterpret_cast<const double *>(s->dev + cap_off) : nullptr;
  s->box = reinterpret_cast<gmr::IkSessionBox *>(s->host + box_off);
  s->box_dev = reinterpret_cast<gmr::IkSessionBox *>(hd + box_off);
  s->entries = reinterpret_cast<gmr::IkGroupEntry *>(s->dev + ent_off);
  gmr::IkGroupEntry ent[2];
  for (int k = 0; k < 2; ++k) {
    ent[k] = gmr::IkGroupEntry{};
    ent[k].m = m->dm_dev; ent[k].L = L; ent[k].L.prm.offset_to_ground = k; ent[k].lay = m->lay;
  }
  if ((e = hipMemcpy(s->entries, ent, sizeof(ent), hipMemcpyHostToDevice)) != hipSuccess) return fail("hipMemcpy", e);
  if (gmr_session_reset(s, nullptr) != GMR_OK) { gmr_session_destroy(s); return nullptr; }
  return s;
}

// Persistent mode: ask the resident wavefront to leave and wait until it has (it also leaves by itself when idle).
static void session_park(gmr_session *s) {
  if (!s->box || !s->st) return;
  __atomic_store_n(&s->box->stop, 1u, __ATOMIC_RELEASE);
  (void)hipStreamSynchronize(s->st);
  __atomic_store_n(&s->box->stop, 0u, __ATOMIC_RELEASE);
  __atomic_store_n(&s->box->exited_gen, s->gen, __ATOMIC_RELEASE);  // (what the wavefront wrote itself, unless it faulted)
}

void gmr_session_destroy(gmr_session *s) {
  if (!s) return;
  if (s->m && s->m->device >= 0) (void)hipSetDevice(s->m->device);
  session_park(s);
  if (s->st) { (void)hipStreamSynchronize(s->st); (void)hipStreamDestroy(s->st); }
  if (s->host) (void)hipHostFree(s->host);
  if (s->dev) (void)hipFree(s->dev);
  delete s;
}

int gmr_session_reset(gmr_session *s, const double *qpos) {
  if (!s) return GMR_EINVAL;
  gmr_model *m = s->m;
  const double *src = qpos ? qpos : blob_ptr<double>(m->blob, m->h.off_qpos0);
  HIP_TRY(m, hipSetDevice(m->device));
  session_park(s);
  HIP_TRY(m, hipStreamSynchronize(s->st));
  HIP_TRY(m, hipMemcpy(s->dev, src, sizeof(double) * (size_t)m->h.nq, hipMemcpyHostToDevice));
  return GMR_OK;
}

int gmr_session_set_persistent(gmr_session *s, int idle_ms) {
  if (!s || idle_ms < 0 || idle_ms > 10000) return GMR_EINVAL;
  gmr_model *m = s->m;
  HIP_TRY(m, hipSetDevice(m->device));
  session_park(s);
  s->idle_ms = idle_ms;
  return GMR_OK;
}

// One frame through the resident wavefront.  (Re)launches it when none is alive: the first frame, or after it left for idleness.
static int session_step_persistent(gmr_session *s, int offset_to_ground) {
  gmr_model *m = s->m;
  gmr::IkSessionBox *box = s->box;
  auto alive = [&]() { return __atomic_load_n(&box->exited_gen, __ATOMIC_ACQUIRE) != s->gen; };
  auto launch = [&]() -> int {
    const unsigned gen = ++s->gen;
    const unsigned long long ticks = 100000ull * (unsigned long long)s->idle_ms;  // s_memrealtime: 100 MHz
    const unsigned max_polls = (unsigned)std::min<unsigned long long>(4000ull * (unsigned long long)s->idle_ms, 0x7fffffffull);
    switch (m->nvp) {
#define GMR_X(v) case v: launch_ik_session<v>(m, s->entries, s->box_dev, ticks, max_polls, 1u << 20, gen, s->st); break;
      GMR_FOR_EACH_NVP(GMR_X)
#undef GMR_X
      default: set_err(m, "internal: no kernel variant for nvp=%d", m->nvp); return GMR_EUNSUPPORTED;
    }
    HIP_TRY(m, hipGetLastError());
    return GMR_OK;
  };
  const unsigned seq = (++s->seq << 1) | (offset_to_ground ? 1u : 0u);  // never equal to the previous word: the frame counter moved
  __atomic_store_n(&box->seq, seq, __ATOMIC_RELEASE);
  if (!alive()) {
    int rc = launch();
    if (rc != GMR_OK) return rc;
  }
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spins = 0;; ++spins) {
    if (__atomic_load_n(&box->ack, __ATOMIC_ACQUIRE) == seq) return GMR_OK;
    if (!alive() && __atomic_load_n(&box->ack, __ATOMIC_ACQUIRE) != seq) {
      int rc = launch();  // it left between our post and its last look at the mailbox
      if (rc != GMR_OK) return rc;
    }
    if ((spins & 1023u) == 1023u) {
      if (hipStreamQuery(s->st) != hipErrorNotReady && __atomic_load_n(&box->ack, __ATOMIC_ACQUIRE) != seq && alive()) {  // the kernel is gone without saying so: a fault
        set_err(m, "persistent session kernel ended unexpectedly: %s", hipGetErrorString(hipGetLastError()));
        __atomic_store_n(&box->exited_gen, s->gen, __ATOMIC_RELEASE);
        return GMR_EDEVICE;
      }
      if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10)) { set_err(m, "persistent session: no answer within 10 s"); return GMR_EDEVICE; }
    }
  }
}

int gmr_session_step(gmr_session *s, const void *human_pos, const void *human_quat, int offset_to_ground, double *qpos_out,
                     int32_t *solves_out) {
  if (!s) return GMR_EINVAL;
  gmr_model *m = s->m;
  m->err.clear();
  if (!human_pos || !human_quat || !qpos_out) { set_err(m, "null argument"); return GMR_EINVAL; }
  memcpy(s->host, human_pos, s->pos_bytes);
  memcpy(s->host + s->quat_off, human_quat, s->quat_bytes);
  HIP_TRY(m, hipSetDevice(m->device));
  if (s->idle_ms > 0) {
    int rc = session_step_persistent(s, offset_to_ground);
    if (rc != GMR_OK) return rc;
  } else {
    gmr::IkLaunch L = s->L;
    L.prm.offset_to_ground = offset_to_ground ? 1 : 0;
    int rc = launch_ik_variant(m, L, s->st);
    if (rc != GMR_OK) return rc;
    HIP_TRY(m, hipStreamSynchronize(s->st));
  }
  const size_t nq = (size_t)m->h.nq;
  memcpy(qpos_out, s->host + s->out_off, nq * 8);
  if (solves_out) memcpy(solves_out, s->host + s->out_off + nq * 8, sizeof(int32_t));
  return GMR_OK;
}

int gmr_session_state(gmr_session *s, double *qpos_out) {
  if (!s || !qpos_out) return GMR_EINVAL;
  gmr_model *m = s->m;
  HIP_TRY(m, hipSetDevice(m->device));
  session_park(s);
  HIP_TRY(m, hipStreamSynchronize(s->st));
  HIP_TRY(m, hipMemcpy(qpos_out, s->dev, sizeof(double) * (size_t)m->h.nq, hipMemcpyDeviceToHost));
  return GMR_OK;
}

int gmr_evaluate(gmr_model *m, const double *qpos, int64_t n_frames, const void *human_pos, const void *human_quat, int in_dtype,
                 int n_cols, const int32_t *slot_col, int offset_to_ground, const double *height_scale, double *err_out,
                 double *task_err_out, double *xpos_out, double *xquat_out, void *stream) {
  if (!m) return GMR_EINVAL;
  m->err.clear();
  if (!qpos || n_frames < 0) { set_err(m, "null argument / negative size"); return GMR_EINVAL; }
  if (n_frames > 0x7fffffff) { set_err(m, "too many frames for one launch"); return GMR_EINVAL; }
  if (err_out || task_err_out) {
    if (m->h.nslot == 0) { set_err(m, "model has no IK config"); return GMR_ENOCONFIG; }
    if (!human_pos || !human_quat || !slot_col || n_cols <= 0 || (in_dtype != GMR_DTYPE_F32 && in_dtype != GMR_DTYPE_F64)) {
      set_err(m, "err_out needs the human key-points, their dtype and slot_col");
      return GMR_EINVAL;
    }
    for (int s = 0; s < m->h.nslot; ++s)
      if (slot_col[s] < 0 || slot_col[s] >= n_cols) { set_err(m, "slot_col[%d]=%d outside [0,%d)", s, slot_col[s], n_cols); return GMR_EINVAL; }
  }
  if (n_frames == 0) return GMR_OK;
  HIP_TRY(m, hipSetDevice(m->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  gmr::EvalLaunch L{};
  L.qpos = qpos; L.err_out = err_out; L.xpos_out = xpos_out; L.xquat_out = xquat_out; L.n_frames = n_frames;
  L.offset_to_ground = offset_to_ground; L.hscale = height_scale; L.task_err_out = task_err_out;
  CallScratch sc;
  if (err_out || task_err_out) {
    const size_t col_bytes = sizeof(int32_t) * (size_t)m->h.nslot;
    int rc = scratch_alloc(m, sc, col_bytes, st);
    if (rc != GMR_OK) return rc;
    HIP_TRY(m, hipMemcpyAsync(sc.p, slot_col, col_bytes, hipMemcpyHostToDevice, st));
    L.hpos = human_pos; L.hquat = human_quat; L.slot_col = static_cast<const int *>(sc.p);
    L.in_f64 = in_dtype == GMR_DTYPE_F64; L.n_cols = n_cols;
  }
  hipLaunchKernelGGL(gmr::eval_kernel, dim3((unsigned)n_frames), dim3(64), m->lds_bytes_eval, st, m->dm_eval_dev, L, m->lay_eval);
  HIP_TRY(m, hipGetLastError());
  return GMR_OK;
}

/* One FK launch over `fk` (the model's tree, or a copy whose record table is a call's scaled one). */
static int fk_launch(gmr_model *m, const gmr::FkTree &fk, const float *root_pos, const float *root_rot_xyzw, const float *dof, int64_t n_frames,
                     float *body_pos_out, float *body_rot_out, void *stream) {
  const int64_t nblk = (n_frames + gmr::kFkThreads - 1) / gmr::kFkThreads;
  if (nblk > 0x7fffffff) { set_err(m, "too many frames for one launch"); return GMR_EINVAL; }
  // the rotation stage is the last LDS region: a positions-only call does not allocate it (more workgroups per CU)
  if (!body_rot_out && m->fk_pos_parts > 0) {  // positions only: one wavefront per tile, the whole tile image in LDS (fk_pos_kernel)
    const int64_t nw = (n_frames + gmr::kFkWave - 1) / gmr::kFkWave;
    if (nw > 0x7fffffff) { set_err(m, "too many frames for one launch"); return GMR_EINVAL; }
    const int nb = fk.nbody;
    auto image = [&](int parts) { return (std::max(1, fk.nslots) * 7 + (parts == 1 ? 3 * nb : 3 * ((nb + parts - 1) / parts))) * gmr::kFkWave * (int)sizeof(float); };
    int parts = m->fk_pos_parts;
    if (parts == 1 && image(1) > 160 * 1024) parts = 2;  // a tile image beyond the CU's LDS: two half images, else the grouped flush below
    const int lds = image(parts);
    if (lds > 160 * 1024) parts = 0;
    if (parts == 0) goto grouped;
    if (parts == 1)
      hipLaunchKernelGGL((gmr::fk_pos_kernel<1>), dim3((unsigned)nw), dim3(gmr::kFkWave), lds, static_cast<hipStream_t>(stream), fk, root_pos,
                         root_rot_xyzw, dof, n_frames, body_pos_out);
    else
      hipLaunchKernelGGL((gmr::fk_pos_kernel<2>), dim3((unsigned)nw), dim3(gmr::kFkWave), lds, static_cast<hipStream_t>(stream), fk, root_pos,
                         root_rot_xyzw, dof, n_frames, body_pos_out);
    HIP_TRY(m, hipGetLastError());
    return GMR_OK;
  }
grouped : {
  const int fk_lds = body_rot_out ? m->fk_lds_bytes : m->fk_lds_bytes - gmr::kFkRotStride * gmr::kFkThreads * (int)sizeof(float);
  hipLaunchKernelGGL((gmr::fk_kernel<0>), dim3((unsigned)nblk), dim3(gmr::kFkThreads), fk_lds, static_cast<hipStream_t>(stream), fk,
                     root_pos, root_rot_xyzw, dof, n_frames, body_pos_out, body_rot_out, (const int64_t *)nullptr, 0, (int *)nullptr);
  HIP_TRY(m, hipGetLastError());
  return GMR_OK;
}
}

int gmr_fk(gmr_model *m, const float *root_pos, const float *root_rot_xyzw, const float *dof, int64_t n_frames, float *body_pos_out,
           float *body_rot_out, void *stream) {
  return gmr_fk_shape(m, root_pos, root_rot_xyzw, dof, nullptr, 0, n_frames, body_pos_out, body_rot_out, stream);
}

int gmr_fk_shape(gmr_model *m, const float *root_pos, const float *root_rot_xyzw, const float *dof, const float *fitted_shape, int shape_width,
                 int64_t n_frames, float *body_pos_out, float *body_rot_out, void *stream) {
  if (!m) return GMR_EINVAL;
  m->err.clear();
  if (!root_pos || !root_rot_xyzw || !body_pos_out || (!dof && m->h.nq > 7) || n_frames < 0) { set_err(m, "null argument / negative size"); return GMR_EINVAL; }
  if (fitted_shape && shape_width != 1 && shape_width != 3) { set_err(m, "fitted_shape is [nbody] (width 1) or [nbody][3] (width 3)"); return GMR_EINVAL; }
  if (n_frames == 0) return GMR_OK;
  HIP_TRY(m, hipSetDevice(m->device));
  if (!fitted_shape) return fk_launch(m, m->fk, root_pos, root_rot_xyzw, dof, n_frames, body_pos_out, body_rot_out, stream);
  // the call's own scaled copy of the body records, in stream-ordered scratch released behind the launch that reads it
  hipStream_t st = static_cast<hipStream_t>(stream);
  CallScratch sc;
  const int nb = m->fk.nbody;
  int rc = scratch_alloc(m, sc, sizeof(gmr::FkBody) * (size_t)nb, st);
  if (rc != GMR_OK) return rc;
  hipLaunchKernelGGL(gmr::fk_scale_bodies_kernel, dim3((nb + 63) / 64), dim3(64), 0, st, m->fk.body, fitted_shape, shape_width, nb, static_cast<gmr::FkBody *>(sc.p));
  gmr::FkTree fk = m->fk;
  fk.body = static_cast<const gmr::FkBody *>(sc.p);
  return fk_launch(m, fk, root_pos, root_rot_xyzw, dof, n_frames, body_pos_out, body_rot_out, stream);
}

static unsigned kin_grid(int64_t items) {  // grid-stride kernels: enough workgroups of 256 to fill the chip several times over, never more than the work
  const int64_t want = (items + gmr::kKinThreads - 1) / gmr::kKinThreads;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, 256 * 32));
}

int gmr_dof_to_rot(gmr_model *m, const float *dof, int64_t n_frames, float *joint_rot_out, void *stream) {
  if (!m) return GMR_EINVAL;
  m->err.clear();
  if (n_frames == 0 || (n_frames > 0 && m->fk.nbody < 2)) return GMR_OK;
  if ((!dof && m->fk.ndof > 0) || !joint_rot_out || n_frames < 0) { set_err(m, "null argument / negative size"); return GMR_EINVAL; }
  HIP_TRY(m, hipSetDevice(m->device));
  hipLaunchKernelGGL(gmr::dof_to_rot_kernel, dim3(kin_grid(n_frames * (m->fk.nbody - 1))), dim3(gmr::kKinThreads), 0, static_cast<hipStream_t>(stream), m->fk,
                     dof, n_frames, joint_rot_out);
  HIP_TRY(m, hipGetLastError());
  return GMR_OK;
}

int gmr_rot_to_dof(gmr_model *m, const float *joint_rot, int64_t n_frames, float *dof_out, void *stream) {
  if (!m) return GMR_EINVAL;
  m->err.clear();
  if (n_frames == 0 || (n_frames > 0 && m->fk.ndof == 0)) return GMR_OK;
  if (!joint_rot || !dof_out || n_frames < 0) { set_err(m, "null argument / negative size"); return GMR_EINVAL; }
  HIP_TRY(m, hipSetDevice(m->device));
  hipLaunchKernelGGL(gmr::rot_to_dof_kernel, dim3(kin_grid(n_frames * m->fk.ndof)), dim3(gmr::kKinThreads), 0, static_cast<hipStream_t>(stream), m->fk, m->kin,
                     joint_rot, n_frames, dof_out);
  HIP_TRY(m, hipGetLastError());
  return GMR_OK;
}

int gmr_local_rot_to_global(gmr_model *m, const float *local_rot, int64_t n_frames, float *global_rot_out, void *stream) {
  if (!m) return GMR_EINVAL;
  m->err.clear();
  if (n_frames == 0) return GMR_OK;
  if (!local_rot || !global_rot_out || n_frames < 0) { set_err(m, "null argument / negative size"); return GMR_EINVAL; }
  if (local_rot == global_rot_out) { set_err(m, "local_rot and global_rot_out must not alias"); return GMR_EINVAL; }
  HIP_TRY(m, hipSetDevice(m->device));
  constexpr int P = GMR_KIN_CHAIN_PASSES;
  const int nb = m->fk.nbody, F = 64 * P / nb;
  const int64_t n_batches = (n_frames + F - 1) / F;
  const int lds = 2 * 64 * P * 16;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(n_batches, 256 * 64));
  hipLaunchKernelGGL((gmr::local_to_global_kernel<P>), dim3(grid), dim3(64), lds, static_cast<hipStream_t>(stream), m->fk, m->kin, local_rot, n_frames,
                     global_rot_out);
  HIP_TRY(m, hipGetLastError());
  return GMR_OK;
}

int gmr_fk_min_height(gmr_model *m, const float *root_pos, const float *root_rot_xyzw, const float *dof, const int64_t *seq_offsets,
                      int n_seq, float *min_z_out, void *stream) {
  if (!m) return GMR_EINVAL;
  m->err.clear();
  if (!root_pos || !root_rot_xyzw || !seq_offsets || !min_z_out || n_seq < 0 || (!dof && m->h.nq > 7)) { set_err(m, "null argument / negative size"); return GMR_EINVAL; }
  if (n_seq == 0) return GMR_OK;
  for (int s = 0; s < n_seq; ++s)
    if (seq_offsets[s + 1] < seq_offsets[s] || seq_offsets[0] != 0) { set_err(m, "seq_offsets must start at 0 and be non-decreasing"); return GMR_EINVAL; }
  const int64_t n_frames = seq_offsets[n_seq];
  HIP_TRY(m, hipSetDevice(m->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t off_bytes = sizeof(int64_t) * (size_t)(n_seq + 1), key_off = (off_bytes + 15) & ~size_t(15);
  CallScratch sc;
  int rc = scratch_alloc(m, sc, key_off + sizeof(int) * (size_t)n_seq, st);
  if (rc != GMR_OK) return rc;
  int *keys = reinterpret_cast<int *>(static_cast<uint8_t *>(sc.p) + key_off);
  HIP_TRY(m, hipMemcpyAsync(sc.p, seq_offsets, off_bytes, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(gmr::fk_minkey_init, dim3((n_seq + 255) / 256), dim3(256), 0, st, keys, n_seq);
  if (n_frames > 0) {
    const int64_t nblk = (n_frames + gmr::kFkThreads - 1) / gmr::kFkThreads;
    if (nblk > 0x7fffffff) { set_err(m, "too many frames for one launch"); return GMR_EINVAL; }
    hipLaunchKernelGGL((gmr::fk_kernel<1>), dim3((unsigned)nblk), dim3(gmr::kFkThreads), m->fk_lds_bytes_min, st, m->fk, root_pos, root_rot_xyzw, dof,
                       n_frames, (float *)nullptr, (float *)nullptr, static_cast<const int64_t *>(sc.p), n_seq, keys);
  }
  hipLaunchKernelGGL(gmr::fk_minkey_decode, dim3((n_seq + 255) / 256), dim3(256), 0, st, keys, min_z_out, n_seq);
  HIP_TRY(m, hipGetLastError());
  return GMR_OK;
}

// ------------------------------------------------------------------ dataset epilogue (motion_kernel.hip.h)
// Validate every member with work, send the entries, clip offsets and minimum keys in one call block ("the call
// block"), and run pass 1 over all members' tiles in one grid, pass 2 (height adjust, decoded minima) in a second when any
// member needs it.
static int motion_run(const Members &g, const gmr_motion_input *inputs, hipStream_t st) {
  struct Member { bool work = false; gmr::CallBlock::Uploaded<int64_t> offs; size_t key0 = 0; };  // key0: its first key
  const int n = g.n;
  std::string &err = g.err;
  gmr::CallBlock blk;
  const auto h_ent = blk.uploaded<gmr::MotionEntry>((size_t)n);
  std::vector<gmr::MotionEntry> ent(n);
  std::vector<Member> mem(n);
  size_t n_keys = 0;
  int64_t tiles = 0, finish = 0, lds = 0;
  bool any = false, any_finish = false;
  std::vector<int> empty_min;  // members without frames that want min_z
  for (int i = 0; i < n; ++i) {
    const gmr_motion_input &in = inputs[i];
    const gmr_model *m = g.models[i];
    const std::string who = g.who(i);
    gmr::MotionEntry &e = ent[i];
    e.tile_base = tiles; e.finish_base = finish;
    if (in.n_frames < 0) { err = who + "negative n_frames"; return GMR_EINVAL; }
    if (in.n_frames == 0) {  // no work for this member; its clips (all empty) still report fk_min_height's +inf
      if (in.min_z_out && in.n_seq > 0) empty_min.push_back(i);
      continue;
    }
    if (m->dm.root_planar) { err = who + "the motion schema needs a free-joint root; a planar base is not supported"; return GMR_EUNSUPPORTED; }
    const int ndof = m->fk.ndof;
    if (!in.qpos || !in.seq_offsets || !in.root_pos_out || !in.root_rot_out || !in.local_body_pos_out || (!in.dof_pos_out && ndof > 0)) {
      err = who + "null argument"; return GMR_EINVAL;
    }
    if (in.flags & ~(GMR_MOTION_HEIGHT_ADJUST | GMR_MOTION_ROOT_ORIGIN)) { err = who + "unknown flags"; return GMR_EINVAL; }
    if (const char *why = seq_offsets_error(in.seq_offsets, in.n_seq, in.n_frames)) { err = who + why; return GMR_EINVAL; }
    const int64_t need = gmr::motion_lds_bytes(m->fk.nbody, ndof, m->fk.nslots);
    if (need > 160 * 1024) { err = who + "the epilogue tile needs " + std::to_string(need) + " bytes of LDS"; return GMR_EUNSUPPORTED; }
    lds = std::max(lds, need);
    e.fk = m->fk;
    e.qpos = in.qpos;
    e.root_pos = in.root_pos_out; e.root_rot = in.root_rot_out; e.dof_pos = in.dof_pos_out;
    e.local_body_pos = in.local_body_pos_out; e.min_z = in.min_z_out;
    e.ground_offset = in.ground_offset;
    e.n_frames = in.n_frames; e.n_seq = in.n_seq;
    e.flags = in.flags | (in.min_z_out ? gmr::kMotionWantMin : 0);
    mem[i].work = true;
    mem[i].offs = blk.put(in.seq_offsets, (size_t)in.n_seq + 1);
    mem[i].key0 = n_keys;
    n_keys += (size_t)in.n_seq;
    tiles += (in.n_frames + gmr::kFkWave - 1) / gmr::kFkWave;
    const int64_t items = ((e.flags & gmr::kMotionHeight) ? in.n_frames : 0) + ((e.flags & gmr::kMotionWantMin) ? in.n_seq : 0);
    finish += (items + gmr::kMotionFinishThreads - 1) / gmr::kMotionFinishThreads;
    any = true;
    any_finish = any_finish || items > 0;
  }
  if (!empty_min.empty()) {
    if (hipSetDevice(g.device) != hipSuccess) { err = "hipSetDevice failed"; return GMR_EDEVICE; }
    for (int i : empty_min)
      if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(inputs[i].min_z_out), 0x7f800000, (size_t)inputs[i].n_seq, st) != hipSuccess) {
        err = "hipMemsetD32Async failed"; return GMR_EDEVICE;
      }
  }
  if (!any) return GMR_OK;
  if (tiles > 0x7fffffff || finish > 0x7fffffff || n_keys > 0x7fffffff) { err = "too many frames for one launch"; return GMR_EINVAL; }
  if (hipSetDevice(g.device) != hipSuccess) { err = "hipSetDevice failed"; return GMR_EDEVICE; }
  const auto h_keys = blk.device_only<int>(std::max<size_t>(n_keys, 1));  // all members' keys in a row: one launch sets them
  CallScratch sc;
  const int rc = send_call_block(g, blk, sc, st, [&](const gmr::CallBlock::Device &dev) {
    for (int i = 0; i < n; ++i) {
      if (!mem[i].work) continue;
      ent[i].seq_offsets = dev(mem[i].offs);
      ent[i].keys = dev(h_keys) + mem[i].key0;
    }
    std::copy(ent.begin(), ent.end(), blk[h_ent]);
    return GMR_OK;
  });
  if (rc != GMR_OK) return rc;
  const gmr::CallBlock::Device dev = blk.on(sc.p);
  if (n_keys > 0)
    hipLaunchKernelGGL(gmr::fk_minkey_init, dim3((unsigned)((n_keys + 255) / 256)), dim3(256), 0, st, dev(h_keys), (int)n_keys);
  hipLaunchKernelGGL(gmr::motion_epilogue_kernel, dim3((unsigned)tiles), dim3(gmr::kFkWave), (unsigned)lds, st, dev(h_ent), n);
  if (any_finish)
    hipLaunchKernelGGL(gmr::motion_finish_kernel, dim3((unsigned)finish), dim3(gmr::kMotionFinishThreads), 0, st, dev(h_ent), n);
  if (hipGetLastError() != hipSuccess) { err = "kernel launch failed"; return GMR_EDEVICE; }
  return GMR_OK;
}

int gmr_motion_epilogue(gmr_model *m, const gmr_motion_input *in, void *stream) {
  return member_call(m, nullptr, in, [&](const Members &g) { return motion_run(g, in, static_cast<hipStream_t>(stream)); });
}

int gmr_group_motion_epilogue(gmr_group *g, const gmr_motion_input *inputs, void *stream) {
  return member_call(nullptr, g, inputs, [&](const Members &ms) { return motion_run(ms, inputs, static_cast<hipStream_t>(stream)); });
}

// ------------------------------------------------------------------ tracking export (track_kernel.hip.h)
int gmr_lowpass_coefficients(double cutoff_hz, double fs, double *c) {
#pragma clang fp contract(off)
  if (!c || !std::isfinite(cutoff_hz) || !std::isfinite(fs) || !(cutoff_hz > 0.0) || !(cutoff_hz < fs / 2)) return GMR_EINVAL;
  const double pi = 3.14159265358979323846, r2 = sqrt(2.0);
  const double K = tan(pi * cutoff_hz / fs);
  const double n = 1.0 / (1.0 + r2 * K + K * K);
  const double b0 = K * K * n;
  c[0] = b0; c[1] = 2.0 * b0; c[2] = b0;
  c[3] = 2.0 * (K * K - 1.0) * n;
  c[4] = (1.0 - r2 * K + K * K) * n;
  return GMR_OK;
}

// Validate every member with work, send the entries and the members' plans (clip offsets, output offsets, ratios) in one call
// block ("the call block"), and run all members' tiles in one grid.
// A member with lowpass_hz > 0 is filtered first (lowpass_kernel.hip.h): the entries of the filter launch and the member's five
// coefficients per clip ride in the same block, the filtered qpos goes into a scratch image of its own (n_frames * nq doubles,
// released behind the launches like the block), and the member's TrackEntry reads that image instead of qpos.
static int track_run(const Members &g, const gmr_track_input *inputs, hipStream_t st) {
  struct Member {
    bool work = false, filtered = false;
    gmr::CallBlock::Uploaded<int64_t> offs, outs;
    gmr::CallBlock::Uploaded<double> ratio, coef;  // coef: [n_seq][5], filtered members only
  };
  const int n = g.n;
  std::string &err = g.err;
  gmr::CallBlock blk;
  const auto h_ent = blk.uploaded<gmr::TrackEntry>((size_t)n);
  std::vector<gmr::TrackEntry> ent(n);
  std::vector<Member> mem(n);
  int64_t tiles = 0, lds = 0, clips = 0;
  for (int i = 0; i < n; ++i) {
    const gmr_track_input &in = inputs[i];
    const gmr_model *m = g.models[i];
    const std::string who = g.who(i);
    gmr::TrackEntry &e = ent[i];
    e.tile_base = tiles;
    if (in.n_frames < 0) { err = who + "negative n_frames"; return GMR_EINVAL; }
    if (in.lowpass_hz < 0.0f || !std::isfinite(in.lowpass_hz)) { err = who + "lowpass_hz must be finite and >= 0"; return GMR_EINVAL; }
    if (in.n_frames == 0) continue;  // no work for this member
    if (m->dm.root_planar) { err = who + "the tracking export needs a free-joint root; a planar base is not supported"; return GMR_EUNSUPPORTED; }
    if (!in.qpos || !in.seq_offsets || !in.out_offsets || !in.ratio) { err = who + "null argument"; return GMR_EINVAL; }
    if (!(in.fps_out > 0.0) || !std::isfinite(in.fps_out)) { err = who + "fps_out must be positive"; return GMR_EINVAL; }
    // the rules of seq_offsets_error, with those of the output plan between them in the order they have always been reported in
    if (const char *why = seq_ends_error(in.seq_offsets, in.n_seq, in.n_frames)) { err = who + why; return GMR_EINVAL; }
    if (in.out_offsets[0] != 0) { err = who + "out_offsets must start at 0"; return GMR_EINVAL; }
    for (int s = 0; s < in.n_seq; ++s) {
      if (const char *why = seq_clip_error(in.seq_offsets, s)) { err = who + why; return GMR_EINVAL; }
      if (in.out_offsets[s + 1] < in.out_offsets[s]) { err = who + "out_offsets must not decrease"; return GMR_EINVAL; }
      if (in.out_offsets[s + 1] > in.out_offsets[s] && in.seq_offsets[s + 1] == in.seq_offsets[s]) {
        err = who + "clip " + std::to_string(s) + " has output frames but no source frames"; return GMR_EINVAL;
      }
      if (!(in.ratio[s] > 0.0) || !std::isfinite(in.ratio[s])) { err = who + "ratio (fps_in / fps_out) must be positive"; return GMR_EINVAL; }
      if (in.lowpass_hz != 0.0f && in.seq_offsets[s + 1] > in.seq_offsets[s]) {
        const double fs = in.ratio[s] * in.fps_out;
        if (!((double)in.lowpass_hz < fs / 2)) {
          err = who + "clip " + std::to_string(s) + ": lowpass_hz " + std::to_string(in.lowpass_hz) + " is not below half its frame rate " + std::to_string(fs);
          return GMR_EINVAL;
        }
      }
    }
    if (in.lowpass_hz != 0.0f && m->fk.ndof + 7 > gmr::kLowpassMaxNq) {
      err = who + "the low-pass filter takes at most " + std::to_string(gmr::kLowpassMaxNq) + " qpos columns"; return GMR_EUNSUPPORTED;
    }
    const int64_t n_out = in.out_offsets[in.n_seq];
    if (n_out == 0) continue;
    const int64_t need = gmr::track_lds_bytes(m->fk.nbody, m->fk.ndof, m->fk.nslots);
    if (need > 160 * 1024) { err = who + "the tracking tile needs " + std::to_string(need) + " bytes of LDS"; return GMR_EUNSUPPORTED; }
    lds = std::max(lds, need);
    e.fk = m->fk;
    e.qpos = in.qpos;
    e.root_pos = in.root_pos_out; e.root_rot = in.root_rot_out; e.joint_pos = in.joint_pos_out;
    e.root_lin_vel = in.root_lin_vel_out; e.root_ang_vel = in.root_ang_vel_out; e.joint_vel = in.joint_vel_out;
    e.body_pos = in.body_pos_w_out; e.body_quat = in.body_quat_w_out;
    e.body_lin_vel = in.body_lin_vel_w_out; e.body_ang_vel = in.body_ang_vel_w_out;
    e.dt = 1.0 / in.fps_out;
    e.n_out = n_out; e.n_seq = in.n_seq;
    Member &mb = mem[i];
    mb.work = true;
    mb.offs = blk.put(in.seq_offsets, (size_t)in.n_seq + 1);
    mb.outs = blk.put(in.out_offsets, (size_t)in.n_seq + 1);
    mb.ratio = blk.put(in.ratio, (size_t)in.n_seq);
    tiles += (n_out + gmr::kTrackTile - 1) / gmr::kTrackTile;
    if (in.lowpass_hz != 0.0f) {
      mb.filtered = true;
      mb.coef = blk.uploaded<double>(5 * (size_t)in.n_seq);
      clips += in.n_seq;
    }
  }
  if (tiles == 0) return GMR_OK;
  if (tiles > 0x7fffffff || clips > 0x7fffffff) { err = "too many frames for one launch"; return GMR_EINVAL; }
  if (hipSetDevice(g.device) != hipSuccess) { err = "hipSetDevice failed"; return GMR_EDEVICE; }
  // without a filtered member the block holds nothing of the filter launch
  const auto h_lp = blk.uploaded<gmr::LowpassEntry>(clips ? (size_t)n : 0);
  CallScratch sc;
  std::vector<CallScratch> images(clips ? n : 0);  // the filtered members' qpos
  const int rc = send_call_block(g, blk, sc, st, [&](const gmr::CallBlock::Device &dev) {
    int64_t base = 0;
    for (int i = 0; i < n; ++i) {
      const Member &mb = mem[i];
      const gmr_track_input &in = inputs[i];
      gmr::TrackEntry &e = ent[i];
      if (mb.work) { e.seq_offsets = dev(mb.offs); e.out_offsets = dev(mb.outs); e.ratio = dev(mb.ratio); }
      if (!clips) continue;
      gmr::LowpassEntry &le = blk[h_lp][i];  // (zero so far)
      le.clip_base = base;
      if (!mb.filtered) continue;
      const int nq = g.models[i]->fk.ndof + 7;
      gmr_model *m0 = g.models[0];
      if (scratch_alloc(m0, images[i], sizeof(double) * (size_t)in.n_frames * (size_t)nq, st) != GMR_OK) { err = m0->err; return GMR_EDEVICE; }
      for (int s = 0; s < in.n_seq; ++s)
        if (in.seq_offsets[s + 1] > in.seq_offsets[s] &&
            gmr_lowpass_coefficients((double)in.lowpass_hz, in.ratio[s] * in.fps_out, blk[mb.coef] + 5 * s) != GMR_OK) {
          err = g.who(i) + "clip " + std::to_string(s) + ": no low-pass coefficients";  // (refused above)
          return GMR_EINVAL;
        }
      le.src = in.qpos;
      le.dst = static_cast<double *>(images[i].p);
      le.seq_offsets = dev(mb.offs);
      le.coef = dev(mb.coef);
      le.n_seq = in.n_seq; le.nq = nq;
      e.qpos = le.dst;
      base += in.n_seq;
    }
    std::copy(ent.begin(), ent.end(), blk[h_ent]);
    return GMR_OK;
  });
  if (rc != GMR_OK) return rc;
  const gmr::CallBlock::Device dev = blk.on(sc.p);
  if (clips)
    hipLaunchKernelGGL(gmr::lowpass_kernel, dim3((unsigned)clips), dim3(gmr::kFkWave), 0, st, dev(h_lp), n);
  hipLaunchKernelGGL(gmr::motion_track_kernel, dim3((unsigned)tiles), dim3(gmr::kFkWave), (unsigned)lds, st, dev(h_ent), n);
  if (hipGetLastError() != hipSuccess) { err = "kernel launch failed"; return GMR_EDEVICE; }
  return GMR_OK;
}

int gmr_motion_track(gmr_model *m, const gmr_track_input *in, void *stream) {
  return member_call(m, nullptr, in, [&](const Members &g) { return track_run(g, in, static_cast<hipStream_t>(stream)); });
}

int gmr_group_motion_track(gmr_group *g, const gmr_track_input *inputs, void *stream) {
  return member_call(nullptr, g, inputs, [&](const Members &ms) { return track_run(ms, inputs, static_cast<hipStream_t>(stream)); });
}

// ------------------------------------------------------------------ motion library sampling (sample_kernel.hip.h)
// Validate, fill the kernel argument and launch: one kernel and nothing else -- no scratch, no copy, no synchronisation (the clip
// table, the ids and the times are device arrays; everything else travels in the argument).
int gmr_motion_sample(gmr_model *m, const gmr_sample_input *in, void *stream) {
  if (!m) return GMR_EINVAL;
  m->err.clear();
  if (!in) { set_err(m, "null input"); return GMR_EINVAL; }
  if (in->k_per_id < 1) { set_err(m, "k_per_id must be at least 1"); return GMR_EINVAL; }
  if (in->n_queries < 0 || in->n_frames < 0 || in->n_seq < 0 || in->n_sel < 0) { set_err(m, "negative count"); return GMR_EINVAL; }
  if (in->n_queries % in->k_per_id != 0) { set_err(m, "n_queries must be a multiple of k_per_id"); return GMR_EINVAL; }
  if (!in->body_ids && in->n_sel != 0) { set_err(m, "n_sel without body_ids"); return GMR_EINVAL; }
  if ((in->time_dtype != GMR_DTYPE_F32 && in->time_dtype != GMR_DTYPE_F64) || (in->out_dtype != GMR_DTYPE_F32 && in->out_dtype != GMR_DTYPE_F64)) {
    set_err(m, "unknown element type"); return GMR_EINVAL;
  }
  if (m->dm.root_planar) { set_err(m, "the motion library needs a free-joint root; a planar base is not supported"); return GMR_EUNSUPPORTED; }
  const int64_t lds = gmr::sample_lds(m->fk.nbody, m->fk.ndof, m->fk.nslots, in->body_ids ? in->n_sel : 0).bytes;
  if (lds > 160 * 1024) { set_err(m, "the sampling tile needs %lld bytes of LDS", (long long)lds); return GMR_EUNSUPPORTED; }
  if (in->n_queries == 0) return GMR_OK;
  if (!in->ids || !in->times || (in->n_seq > 0 && (!in->qpos || !in->seq_offsets || !in->fps))) { set_err(m, "null argument"); return GMR_EINVAL; }
  const int64_t tiles = (in->n_queries + gmr::kFkWave - 1) / gmr::kFkWave;
  if (tiles > 0x7fffffff) { set_err(m, "too many queries for one launch"); return GMR_EINVAL; }
  if (hipSetDevice(m->device) != hipSuccess) { set_err(m, "hipSetDevice failed"); return GMR_EDEVICE; }
  gmr::SampleArgs a{};
  a.body = m->fk.body; a.save_slot = m->fk.save_slot;
  a.nbody = m->fk.nbody; a.ndof = m->fk.ndof; a.nslots = m->fk.nslots; a.n_seq = in->n_seq;
  a.qpos = in->qpos; a.n_frames = in->n_frames; a.seq_offsets = in->seq_offsets; a.fps = in->fps;
  a.ids = in->ids; a.times = in->times; a.n_queries = in->n_queries;
  a.body_ids = in->body_ids; a.n_sel = in->n_sel; a.k_per_id = in->k_per_id;
  a.time_f64 = in->time_dtype == GMR_DTYPE_F64; a.out_f64 = in->out_dtype == GMR_DTYPE_F64;
  a.root_pos = in->root_pos_out; a.root_rot = in->root_rot_out; a.joint_pos = in->joint_pos_out;
  a.root_lin_vel = in->root_lin_vel_out; a.root_ang_vel = in->root_ang_vel_out; a.joint_vel = in->joint_vel_out;
  a.body_pos = in->body_pos_w_out; a.body_quat = in->body_quat_w_out;
  a.body_lin_vel = in->body_lin_vel_w_out; a.body_ang_vel = in->body_ang_vel_w_out;
  hipLaunchKernelGGL(gmr::motion_sample_kernel, dim3((unsigned)tiles), dim3(gmr::kFkWave), (unsigned)lds, static_cast<hipStream_t>(stream), a);
  if (hipGetLastError() != hipSuccess) { set_err(m, "kernel launch failed"); return GMR_EDEVICE; }
  return GMR_OK;
}

// ------------------------------------------------------------------ contact labels (contact_kernel.hip.h)
// The launch of gmr_motion_contacts: one kernel, one wavefront per clip, and nothing else -- every array is a device array and
// everything else travels in the kernel's argument.
static int contact_run(gmr_model *m, const gmr_contact_input &in, hipStream_t st) {
  if (hipSetDevice(m->device) != hipSuccess) { set_err(m, "hipSetDevice failed"); return GMR_EDEVICE; }
  gmr::ContactArgs a{};
  a.pos = in.body_pos_w; a.vel = in.body_lin_vel_w;
  a.out_offsets = in.out_offsets; a.body_ids = in.body_ids; a.height_offset = in.height_offset;
  a.n_rows = in.n_rows;
  a.nbody = m->fk.nbody; a.n_contact = in.n_contact; a.clip_min = in.ground_mode == GMR_CONTACT_GROUND_CLIP_MIN;
  a.ground_z = in.ground_z; a.height_on = in.height_on; a.height_off = in.height_off;
  a.speed_on2 = in.speed_on * in.speed_on; a.speed_off2 = in.speed_off * in.speed_off;
  a.contact = in.contact_out; a.frames = in.frames_out; a.touchdowns = in.touchdowns_out;
  a.slide_sum = in.slide_sum_out; a.slide_step_max = in.slide_step_max_out; a.depth_max = in.depth_max_out;
  a.airborne = in.airborne_frames_out; a.base = in.base_out;
  hipLaunchKernelGGL(gmr::motion_contacts_kernel, dim3((unsigned)in.n_seq), dim3(gmr::kFkWave), 0, st, a);
  if (hipGetLastError() != hipSuccess) { set_err(m, "kernel launch failed"); return GMR_EDEVICE; }
  return GMR_OK;
}

int gmr_motion_contacts(gmr_model *m, const gmr_contact_input *in) {
  if (!m) return GMR_EINVAL;
  m->err.clear();
  if (!in) { set_err(m, "null input"); return GMR_EINVAL; }
  if (in->n_rows < 0 || in->n_seq < 0) { set_err(m, "negative count"); return GMR_EINVAL; }
  if (in->n_contact < 1) { set_err(m, "n_contact must be at least 1"); return GMR_EINVAL; }
  if (in->n_contact > gmr::kContactMaxCols) { set_err(m, "at most %d contact bodies per call", gmr::kContactMaxCols); return GMR_EUNSUPPORTED; }
  if (in->ground_mode != GMR_CONTACT_GROUND_FIXED && in->ground_mode != GMR_CONTACT_GROUND_CLIP_MIN) { set_err(m, "unknown ground_mode"); return GMR_EINVAL; }
  if (!std::isfinite(in->height_on) || !std::isfinite(in->height_off) || !std::isfinite(in->speed_on) || !std::isfinite(in->speed_off)) {
    set_err(m, "the contact thresholds must be finite"); return GMR_EINVAL;
  }
  if (in->height_on > in->height_off) { set_err(m, "height_on must not exceed height_off"); return GMR_EINVAL; }
  if (in->speed_on < 0.0 || in->speed_on > in->speed_off) { set_err(m, "0 <= speed_on <= speed_off is required"); return GMR_EINVAL; }
  if (in->ground_mode == GMR_CONTACT_GROUND_FIXED && !std::isfinite(in->ground_z)) { set_err(m, "ground_z must be finite"); return GMR_EINVAL; }
  if (in->n_rows == 0 || in->n_seq == 0) return GMR_OK;
  if (!in->body_pos_w || !in->body_lin_vel_w || !in->out_offsets || !in->body_ids) { set_err(m, "null argument"); return GMR_EINVAL; }
  return contact_run(m, *in, static_cast<hipStream_t>(in->stream));
}

// ------------------------------------------------------------------ foot locking (footlock_kernel.hip.h)
// The chains of gmr_motion_footlock, derived on the host from the blob's tree and the caller's body ids: per column the path from
// the root's child down to the contact body, and of its hinges those that lie on no other column's path.  Everything travels in
// the kernels' argument.
static int footlock_plan(gmr_model *m, const gmr_footlock_input &in, gmr::FootlockArgs &a, int &lds_doubles) {
  const int nb = m->h.nbody, C = in.n_contact;
  const int32_t *parent = blob_ptr<int32_t>(m->blob, m->h.off_parent), *jtype = blob_ptr<int32_t>(m->blob, m->h.off_jnt_type);
  std::vector<int> on_paths(nb, 0);
  for (int c = 0; c < C; ++c) {
    const int id = in.body_ids[c];
    if (id < 0 || id >= nb) { set_err(m, "body_ids[%d] = %d is not a body of the model (%d bodies)", c, id, nb); return GMR_EINVAL; }
    for (int d = 0; d < c; ++d)
      if (in.body_ids[d] == id) { set_err(m, "body %d is named by two contact columns", id); return GMR_EINVAL; }
  }
  lds_doubles = 0;
  for (int c = 0; c < C; ++c) {
    std::vector<int> path;  // the contact body first
    for (int j = in.body_ids[c]; j >= 0 && jtype[j] != GMR_JNT_FREE; j = parent[j]) path.push_back(j);
    if ((int)path.size() > gmr::kFootlockMaxPath) {
      set_err(m, "contact body %d lies %d bodies below the root; at most %d are supported", in.body_ids[c], (int)path.size(), gmr::kFootlockMaxPath);
      return GMR_EUNSUPPORTED;
    }
    a.path_len[c] = (uint8_t)path.size();
    for (size_t i = 0; i < path.size(); ++i) {
      a.path[c][i] = (uint8_t)path[path.size() - 1 - i];
      on_paths[path[i]] += 1;
    }
  }
  for (int c = 0; c < C; ++c) {
    int n = 0;
    uint32_t mask = 0;
    for (int i = 0; i < a.path_len[c]; ++i) {
      const int j = a.path[c][i];
      if (jtype[j] == GMR_JNT_HINGE && on_paths[j] == 1) { mask |= 1u << i; ++n; }
    }
    if (n < 3) { set_err(m, "the chain of contact body %d holds %d hinges of its own; at least 3 are needed", in.body_ids[c], n); return GMR_EINVAL; }
    if (n > gmr::kFootlockMaxChain) {
      set_err(m, "the chain of contact body %d holds %d hinges; at most %d are supported", in.body_ids[c], n, gmr::kFootlockMaxChain);
      return GMR_EUNSUPPORTED;
    }
    a.chain_mask[c] = mask;
    a.n_chain[c] = (uint8_t)n;
    lds_doubles = std::max(lds_doubles, gmr::footlock_solve_doubles(a.path_len[c], n));
  }
  return GMR_OK;
}

// The three launches of gmr_motion_footlock, and nothing else: no allocation, no copy, no synchronisation.
static int footlock_run(gmr_model *m, const gmr_footlock_input &in, gmr::FootlockArgs &a, int lds_doubles, hipStream_t st) {
  if (hipSetDevice(m->device) != hipSuccess) { set_err(m, "hipSetDevice failed"); return GMR_EDEVICE; }
  const int nq = m->fk.ndof + 7;
  a.dm = m->dm_eval_dev; a.lo = m->rep_lo; a.hi = m->rep_hi;
  a.qpos = in.qpos; a.seq_offsets = in.seq_offsets; a.contact = in.contact; a.n_frames = in.n_frames;
  a.n_seq = in.n_seq; a.C = in.n_contact; a.nq = nq; a.blend = in.blend_frames; a.min_run = in.min_run; a.iters = in.iterations;
  a.damping = in.damping; a.step_cap = in.step_cap;
  a.qpos_out = in.qpos_out; a.pos = in.pos_out; a.shift = in.shift_out;
  a.runs = in.runs_out; a.locked = in.locked_frames_out; a.shift_max = in.shift_max_out; a.resid_max = in.residual_max_out;
  a.limit_frames = in.limit_frames_out;
  const unsigned ty = gmr::footlock_clip_waves(in.n_frames, in.n_seq, gmr::kFkWave);  // tiles of one clip in flight
  const unsigned lds_a = (unsigned)(gmr::motion_qpitch(nq) * gmr::kFkWave * sizeof(double));
  const unsigned lds_c = (unsigned)(lds_doubles * gmr::kFkWave * sizeof(double));
  hipLaunchKernelGGL(gmr::footlock_pos_kernel, dim3((unsigned)in.n_seq, ty), dim3(gmr::kFkWave), lds_a, st, a);
  hipLaunchKernelGGL(gmr::footlock_runs_kernel, dim3((unsigned)in.n_seq, (unsigned)in.n_contact), dim3(gmr::kFkWave), 0, st, a);
  hipLaunchKernelGGL(gmr::footlock_solve_kernel, dim3((unsigned)in.n_seq, ty, (unsigned)in.n_contact), dim3(gmr::kFkWave), lds_c, st, a);
  if (hipGetLastError() != hipSuccess) { set_err(m, "kernel launch failed"); return GMR_EDEVICE; }
  return GMR_OK;
}

int gmr_motion_footlock(gmr_model *m, const gmr_footlock_input *in) {
  if (!m) return GMR_EINVAL;
  m->err.clear();
  if (!in) { set_err(m, "null input"); return GMR_EINVAL; }
  if (in->n_frames < 0 || in->n_seq < 0) { set_err(m, "negative count"); return GMR_EINVAL; }
  if (in->n_contact < 1 || in->n_contact > gmr::kFootlockMaxCols) { set_err(m, "n_contact must be 1 .. %d", gmr::kFootlockMaxCols); return GMR_EINVAL; }
  if (in->blend_frames < 0) { set_err(m, "blend_frames must be >= 0"); return GMR_EINVAL; }
  if (in->min_run < 1) { set_err(m, "min_run must be >= 1"); return GMR_EINVAL; }
  if (in->iterations < 1 || in->iterations > gmr::kFootlockMaxIters) { set_err(m, "iterations must be 1 .. %d", gmr::kFootlockMaxIters); return GMR_EINVAL; }
  if (!(in->damping > 0.0) || !std::isfinite(in->damping)) { set_err(m, "damping must be finite and > 0"); return GMR_EINVAL; }
  if (!(in->step_cap > 0.0) || !std::isfinite(in->step_cap)) { set_err(m, "step_cap must be finite and > 0"); return GMR_EINVAL; }
  if (!in->body_ids) { set_err(m, "null body_ids"); return GMR_EINVAL; }
  if (in->qpos_out && in->qpos_out == in->qpos) { set_err(m, "qpos_out must not alias qpos"); return GMR_EINVAL; }
  if (m->dm.root_planar) { set_err(m, "foot locking needs a free-joint root; a planar base is not supported"); return GMR_EUNSUPPORTED; }
  gmr::FootlockArgs a{};
  int lds_doubles = 0;
  const int rc = footlock_plan(m, *in, a, lds_doubles);
  if (rc != GMR_OK) return rc;
  if (in->n_frames == 0 || in->n_seq == 0) return GMR_OK;
  if (!in->qpos || !in->seq_offsets || !in->contact || !in->qpos_out || !in->pos_out || !in->shift_out) { set_err(m, "null argument"); return GMR_EINVAL; }
  if ((int64_t)gmr::motion_qpitch(m->fk.ndof + 7) * gmr::kFkWave * 8 > 64 * 1024) { set_err(m, "the row tile needs more than 64 KiB of LDS"); return GMR_EUNSUPPORTED; }
  return footlock_run(m, *in, a, lds_doubles, static_cast<hipStream_t>(in->stream));
}

// ------------------------------------------------------------------ inverse dynamics (dynamics_kernel.hip.h)
// The two launches of gmr_motion_dynamics, and nothing else: no allocation, no copy, no synchronisation.  Every array is a device
// array and everything else travels in the kernels' argument.
static int dynamics_run(gmr_model *m, const gmr_dynamics_input &in, bool stats, hipStream_t st) {
  if (hipSetDevice(m->device) != hipSuccess) { set_err(m, "hipSetDevice failed"); return GMR_EDEVICE; }
  gmr::DynamicsArgs a{};
  a.dm = m->dm_eval_dev;
  a.qpos = in.qpos; a.qvel = in.qvel; a.qacc = in.qacc; a.seq_offsets = in.seq_offsets; a.n_frames = in.n_frames;
  a.n_seq = in.n_seq; a.nbody = m->fk.nbody; a.nq = m->fk.ndof + 7; a.nh = m->fk.ndof;
  a.dt = 1.0 / in.fps; a.gx = in.gravity_x; a.gy = in.gravity_y; a.gz = in.gravity_z;
  a.gnorm = std::sqrt(in.gravity_x * in.gravity_x + in.gravity_y * in.gravity_y + in.gravity_z * in.gravity_z);
  a.ground_z = in.ground_z; a.fz_min = in.fz_min;
  a.parent = in.body_parent; a.mass = in.body_mass; a.com = in.body_com; a.inertia = in.body_inertia;
  a.armature = in.armature; a.limit = in.torque_limit;
  a.tau = in.tau_out; a.wrench = in.root_wrench_out; a.comw = in.com_out; a.zmp = in.zmp_out;
  a.qvel_out = in.qvel_out; a.qacc_out = in.qacc_out;
  a.tau_abs_max = in.tau_abs_max_out; a.tau_rms = in.tau_rms_out; a.tau_ratio_max = in.tau_ratio_max_out;
  a.frames_over = in.frames_over_limit_out; a.any_over = in.frames_any_over_limit_out;
  a.fz_max = in.fz_ratio_max_out; a.fz_min_out = in.fz_ratio_min_out;
  a.unloaded = in.unloaded_frames_out; a.nonfinite = in.nonfinite_frames_out;
  // wavefronts per clip: the grid rule of clip_launch.h over the mean clip's frame slots
  const unsigned ty = gmr::clip_waves(gmr::kDynTargetWaves, in.n_seq, gmr::mean_clip_slots(in.n_frames, gmr::chain_geom(a.nbody).groups, in.n_seq));
  hipLaunchKernelGGL(gmr::motion_dynamics_kernel, dim3((unsigned)in.n_seq, ty), dim3(gmr::kFkWave), 0, st, a);
  if (stats) hipLaunchKernelGGL(gmr::motion_dynamics_stats_kernel, dim3((unsigned)in.n_seq), dim3(gmr::kFkWave), 0, st, a);
  if (hipGetLastError() != hipSuccess) { set_err(m, "kernel launch failed"); return GMR_EDEVICE; }
  return GMR_OK;
}

int gmr_motion_dynamics(gmr_model *m, const gmr_dynamics_input *in) {
  if (!m) return GMR_EINVAL;
  m->err.clear();
  if (!in) { set_err(m, "null input"); return GMR_EINVAL; }
  if (in->n_frames < 0 || in->n_seq < 0) { set_err(m, "negative count"); return GMR_EINVAL; }
  if (!std::isfinite(in->fps) || !(in->fps > 0.0)) { set_err(m, "fps must be finite and > 0"); return GMR_EINVAL; }
  if (!std::isfinite(in->gravity_x) || !std::isfinite(in->gravity_y) || !std::isfinite(in->gravity_z) || !std::isfinite(in->ground_z)) {
    set_err(m, "gravity and ground_z must be finite"); return GMR_EINVAL;
  }
  if (in->gravity_x == 0.0 && in->gravity_y == 0.0 && in->gravity_z == 0.0) { set_err(m, "gravity must not be zero"); return GMR_EINVAL; }
  if (!std::isfinite(in->fz_min) || in->fz_min < 0.0) { set_err(m, "fz_min must be finite and >= 0"); return GMR_EINVAL; }
  if (m->dm.root_planar) { set_err(m, "inverse dynamics needs a free-joint root; a planar base is not supported"); return GMR_EUNSUPPORTED; }
  const int nb = m->h.nbody;
  if (in->nbody != nb) { set_err(m, "the inertial table holds %d bodies, the model %d", in->nbody, nb); return GMR_EUNSUPPORTED; }
  if (nb > gmr::kFkWave || gmr::kDynLdsBytes > 160 * 1024) { set_err(m, "a model of %d bodies does not fit the dynamics tile", nb); return GMR_EUNSUPPORTED; }
  if (const int b = gmr::tree_first_not_depth_first(blob_ptr<int32_t>(m->blob, m->h.off_parent), nb)) {
    set_err(m, "body %d does not follow its parent's subtree: the bodies are not in depth-first order", b); return GMR_EUNSUPPORTED;
  }
  const bool stats = in->tau_abs_max_out || in->tau_rms_out || in->tau_ratio_max_out || in->frames_over_limit_out ||
                     in->frames_any_over_limit_out || in->fz_ratio_max_out || in->fz_ratio_min_out || in->unloaded_frames_out ||
                     in->nonfinite_frames_out;
  // A model without a hinge (a floating base alone) has arrays of no columns: tau_out, armature and torque_limit may be NULL.
  const bool hinges = m->fk.ndof > 0;
  if (stats && ((hinges && !in->tau_out) || !in->root_wrench_out)) { set_err(m, "the statistics are reduced from tau_out and root_wrench_out: both are required"); return GMR_EINVAL; }
  if (in->n_frames == 0 || in->n_seq == 0) return GMR_OK;
  if (!in->qpos || !in->seq_offsets || !in->body_parent || !in->body_mass || !in->body_com || !in->body_inertia ||
      (hinges && (!in->armature || !in->torque_limit))) {
    set_err(m, "null argument"); return GMR_EINVAL;
  }
  return dynamics_run(m, *in, stats, static_cast<hipStream_t>(in->stream));
}

// ------------------------------------------------------------------ self-collision (self_collision_kernel.hip.h)
// The two launches of gmr_motion_self_collision, and nothing else: no allocation, no copy, no synchronisation.  Every array is a
// device array and everything else -- the tree's parents and depths included -- travels in the kernels' argument.
static int self_collision_run(gmr_model *m, const gmr_self_collision_input &in, bool stats, hipStream_t st) {
  if (hipSetDevice(m->device) != hipSuccess) { set_err(m, "hipSetDevice failed"); return GMR_EDEVICE; }
  gmr::SelfCollisionArgs a{};
  a.dm = m->dm_eval_dev;
  a.qpos = in.qpos; a.seq_offsets = in.seq_offsets; a.n_frames = in.n_frames;
  a.n_seq = in.n_seq; a.nbody = m->h.nbody; a.nq = m->fk.ndof + 7; a.n_caps = in.n_caps; a.n_pairs = in.n_pairs;
  a.cap_body = in.cap_body; a.cap_p0 = in.cap_p0; a.cap_p1 = in.cap_p1; a.cap_radius = in.cap_radius; a.pairs = in.pairs;
  a.margin = in.margin;
  a.clearance = in.clearance_out; a.pair = in.pair_out; a.hits = in.hits_out;
  a.clearance_min = in.clearance_min_out; a.worst_frame = in.worst_frame_out; a.worst_pair = in.worst_pair_out;
  a.colliding = in.colliding_frames_out; a.longest_run = in.longest_run_out; a.hits_sum = in.hits_sum_out;
  a.nonfinite = in.nonfinite_frames_out;
  gmr::tree_parent_depth(blob_ptr<int32_t>(m->blob, m->h.off_parent), a.nbody, a.parent, a.depth);
  // Wavefronts per clip as in dynamics_run; GMR_AMD_COLLISION_WAVES forces a number (the results do not depend on it).
  const unsigned rule = gmr::clip_waves(gmr::kColTargetWaves, in.n_seq, gmr::mean_clip_slots(in.n_frames, gmr::chain_geom(a.nbody).groups, in.n_seq));
  const unsigned ty = (unsigned)gmr::env_int("GMR_AMD_COLLISION_WAVES", 1, gmr::kGridYMax, rule);
  // Where the pair indices live: staged in LDS as 16-bit words while the table is small, re-read from L2 in every
  // frame otherwise.  GMR_AMD_COLLISION_PAIRS=lds / global forces one (lds only where it fits).
  const bool lds = gmr::collision_pairs_in_lds("GMR_AMD_COLLISION_PAIRS", in.n_pairs, gmr::kColPairsLdsMax);
  const unsigned bytes = (unsigned)gmr::self_collision_lds_bytes(in.n_caps, in.n_pairs, lds);
  if (lds) hipLaunchKernelGGL(gmr::motion_self_collision_kernel<true>, dim3((unsigned)in.n_seq, ty), dim3(gmr::kFkWave), bytes, st, a);
  else hipLaunchKernelGGL(gmr::motion_self_collision_kernel<false>, dim3((unsigned)in.n_seq, ty), dim3(gmr::kFkWave), bytes, st, a);
  if (stats) hipLaunchKernelGGL(gmr::motion_self_collision_stats_kernel, dim3((unsigned)in.n_seq), dim3(gmr::kFkWave), 0, st, a);
  if (hipGetLastError() != hipSuccess) { set_err(m, "kernel launch failed"); return GMR_EDEVICE; }
  return GMR_OK;
}

int gmr_motion_self_collision(gmr_model *m, const gmr_self_collision_input *in) {
  if (!m) return GMR_EINVAL;
  m->err.clear();
  if (!in) { set_err(m, "null input"); return GMR_EINVAL; }
  if (in->n_frames < 0 || in->n_seq < 0 || in->n_caps < 0 || in->n_pairs < 0) { set_err(m, "negative count"); return GMR_EINVAL; }
  if (!std::isfinite(in->margin)) { set_err(m, "margin must be finite"); return GMR_EINVAL; }
  const int nb = m->h.nbody;
  if (nb > gmr::kFkWave) { set_err(m, "a model of %d bodies does not fit the self-collision tile", nb); return GMR_EUNSUPPORTED; }
  if (in->n_caps > gmr::kColMaxCaps) { set_err(m, "at most %d capsules per call", gmr::kColMaxCaps); return GMR_EUNSUPPORTED; }
  if (in->n_pairs > gmr::kColMaxPairs) { set_err(m, "at most %d pairs per call", gmr::kColMaxPairs); return GMR_EUNSUPPORTED; }
  const bool stats = in->clearance_min_out || in->worst_frame_out || in->worst_pair_out || in->colliding_frames_out ||
                     in->longest_run_out || in->hits_sum_out || in->nonfinite_frames_out;
  if (in->n_frames == 0 || in->n_seq == 0) return GMR_OK;   // (an array of no rows may well be a NULL pointer)
  if (stats && (!in->clearance_out || !in->pair_out || !in->hits_out)) {
    set_err(m, "the statistics are reduced from clearance_out, pair_out and hits_out: all three are required"); return GMR_EINVAL;
  }
  if (in->n_caps < 1 || in->n_pairs < 1) { set_err(m, "n_caps and n_pairs must be at least 1"); return GMR_EINVAL; }
  if (!in->qpos || !in->seq_offsets || !in->cap_body || !in->cap_p0 || !in->cap_p1 || !in->cap_radius || !in->pairs) {
    set_err(m, "null argument"); return GMR_EINVAL;
  }
  return self_collision_run(m, *in, stats, static_cast<hipStream_t>(in->stream));
}

// ------------------------------------------------------------------ self-collision repair (self_collision_repair_kernel.hip.h)
// The two launches of gmr_motion_self_collision_repair, and nothing else: no allocation, no copy, no synchronisation.  The tree's
// parents and depths and, per body, the set of movable hinge bodies on its path from the root -- the caller's hinge mask, which is in
// qpos order, carried over to body bits here -- travel in the kernels' argument.
static int self_collision_repair_run(gmr_model *m, const gmr_self_collision_repair_input &in, bool stats, hipStream_t st) {
  if (hipSetDevice(m->device) != hipSuccess) { set_err(m, "hipSetDevice failed"); return GMR_EDEVICE; }
  gmr::SelfCollisionRepairArgs a{};
  a.dm = m->dm_eval_dev; a.lo = m->rep_lo; a.hi = m->rep_hi;
  a.qpos = in.qpos; a.seq_offsets = in.seq_offsets; a.n_frames = in.n_frames;
  a.n_seq = in.n_seq; a.nbody = m->h.nbody; a.nq = m->fk.ndof + 7; a.n_caps = in.n_caps; a.n_pairs = in.n_pairs; a.iters = in.iterations;
  a.cap_body = in.cap_body; a.cap_p0 = in.cap_p0; a.cap_p1 = in.cap_p1; a.cap_radius = in.cap_radius; a.pairs = in.pairs;
  a.margin = in.margin; a.damping = in.damping; a.step_cap = in.step_cap; a.resolve_tol = in.resolve_tol;
  a.qpos_out = in.qpos_out; a.before = in.clearance_before_out; a.after = in.clearance_after_out; a.move = in.move_out;
  a.repaired = in.repaired_frames_out; a.unresolved = in.unresolved_frames_out; a.move_max = in.move_max_out;
  a.clearance_min_after = in.clearance_min_after_out; a.nonfinite = in.nonfinite_frames_out;
  const int32_t *parent = blob_ptr<int32_t>(m->blob, m->h.off_parent), *jtype = blob_ptr<int32_t>(m->blob, m->h.off_jnt_type);
  const int32_t *qadr = blob_ptr<int32_t>(m->blob, m->h.off_qpos_adr);
  gmr::tree_parent_depth(parent, a.nbody, a.parent, a.depth);
  for (int b = 0; b < a.nbody; ++b) {   // (a parent precedes its child)
    const int hcol = jtype[b] == GMR_JNT_HINGE ? qadr[b] - 7 : -1;
    const uint64_t own = hcol >= 0 && hcol < 64 && ((in.hinge_mask >> hcol) & 1ull) ? 1ull << b : 0ull;
    a.movable |= own;
    a.anc[b] = (parent[b] >= 0 ? a.anc[parent[b]] : 0ull) | own;
  }
  // Wavefronts per clip by the grid rule of clip_launch.h, one frame per slot; GMR_AMD_COLLISION_REPAIR_WAVES forces a number (the
  // results do not depend on it).  The pair indices: staged in LDS while the table is small, as in self_collision_run
  // (GMR_AMD_COLLISION_REPAIR_PAIRS=global forces the other instance).
  const unsigned rule = gmr::clip_waves(gmr::kScrTargetWaves, in.n_seq, gmr::mean_clip_slots(in.n_frames, 1, in.n_seq));
  const unsigned ty = (unsigned)gmr::env_int("GMR_AMD_COLLISION_REPAIR_WAVES", 1, gmr::kGridYMax, rule);
  const bool lds = gmr::collision_pairs_in_lds("GMR_AMD_COLLISION_REPAIR_PAIRS", in.n_pairs, gmr::kScrPairsLdsMax);
  const unsigned bytes = (unsigned)gmr::self_collision_repair_lds_bytes(in.n_caps, in.n_pairs, lds);
  if (lds) hipLaunchKernelGGL(gmr::self_collision_repair_kernel<true>, dim3((unsigned)in.n_seq, ty), dim3(gmr::kFkWave), bytes, st, a);
  else hipLaunchKernelGGL(gmr::self_collision_repair_kernel<false>, dim3((unsigned)in.n_seq, ty), dim3(gmr::kFkWave), bytes, st, a);
  if (stats) hipLaunchKernelGGL(gmr::self_collision_repair_stats_kernel, dim3((unsigned)in.n_seq), dim3(gmr::kFkWave), 0, st, a);
  if (hipGetLastError() != hipSuccess) { set_err(m, "kernel launch failed"); return GMR_EDEVICE; }
  return GMR_OK;
}

int gmr_motion_self_collision_repair(gmr_model *m, const gmr_self_collision_repair_input *in) {
  if (!m) return GMR_EINVAL;
  m->err.clear();
  if (!in) { set_err(m, "null input"); return GMR_EINVAL; }
  if (in->n_frames < 0 || in->n_seq < 0 || in->n_caps < 0 || in->n_pairs < 0) { set_err(m, "negative count"); return GMR_EINVAL; }
  if (!std::isfinite(in->margin)) { set_err(m, "margin must be finite"); return GMR_EINVAL; }
  if (in->iterations < 1 || in->iterations > gmr::kScrMaxIters) { set_err(m, "iterations must be 1 .. %d", gmr::kScrMaxIters); return GMR_EINVAL; }
  if (!(in->damping > 0.0) || !std::isfinite(in->damping)) { set_err(m, "damping must be finite and > 0"); return GMR_EINVAL; }
  if (!(in->step_cap > 0.0) || !std::isfinite(in->step_cap)) { set_err(m, "step_cap must be finite and > 0"); return GMR_EINVAL; }
  if (!(in->resolve_tol >= 0.0) || !std::isfinite(in->resolve_tol)) { set_err(m, "resolve_tol must be finite and >= 0"); return GMR_EINVAL; }
  if (in->qpos_out && in->qpos_out == in->qpos) { set_err(m, "qpos_out must not alias qpos"); return GMR_EINVAL; }
  if (m->dm.root_planar) { set_err(m, "the self-collision repair needs a free-joint root; a planar base is not supported"); return GMR_EUNSUPPORTED; }
  const int nb = m->h.nbody;
  if (nb > gmr::kFkWave || m->fk.ndof + 7 > gmr::kScrRow) { set_err(m, "a model of %d bodies does not fit the self-collision tile", nb); return GMR_EUNSUPPORTED; }
  if (in->n_caps > gmr::kScrMaxCaps) { set_err(m, "at most %d capsules per call", gmr::kScrMaxCaps); return GMR_EUNSUPPORTED; }
  if (in->n_pairs > gmr::kScrMaxPairs) { set_err(m, "at most %d pairs per call", gmr::kScrMaxPairs); return GMR_EUNSUPPORTED; }
  const bool stats = in->repaired_frames_out || in->unresolved_frames_out || in->move_max_out || in->clearance_min_after_out ||
                     in->nonfinite_frames_out;
  if (in->n_frames == 0 || in->n_seq == 0) return GMR_OK;   // (an array of no rows may well be a NULL pointer)
  if (stats && (!in->clearance_before_out || !in->clearance_after_out || !in->move_out)) {
    set_err(m, "the statistics are reduced from clearance_before_out, clearance_after_out and move_out: all three are required"); return GMR_EINVAL;
  }
  if (in->n_caps < 1 || in->n_pairs < 1) { set_err(m, "n_caps and n_pairs must be at least 1"); return GMR_EINVAL; }
  if (!in->qpos || !in->seq_offsets || !in->cap_body || !in->cap_p0 || !in->cap_p1 || !in->cap_radius || !in->pairs || !in->qpos_out) {
    set_err(m, "null argument"); return GMR_EINVAL;
  }
  return self_collision_repair_run(m, *in, stats, static_cast<hipStream_t>(in->stream));
}

// ------------------------------------------------------------------ mirror augmentation (mirror_kernel.hip.h)
// The one launch of gmr_motion_mirror, and nothing else: no allocation, no copy, no synchronisation.  The grid is (clips, wavefronts
// per clip) by the grid rule of clip_launch.h over the mean clip's tiles.  GMR_AMD_MIRROR_WAVES forces a number (the results do not
// depend on it).
static int mirror_run(gmr_model *m, const gmr_mirror_input &in, int nq, hipStream_t st) {
  if (hipSetDevice(m->device) != hipSuccess) { set_err(m, "hipSetDevice failed"); return GMR_EDEVICE; }
  gmr::MirrorArgs a{};
  a.qpos = in.qpos; a.out = in.qpos_out; a.seq_offsets = in.seq_offsets; a.col_src = in.col_src; a.col_sign = in.col_sign;
  a.n_frames = in.n_frames; a.n_seq = in.n_seq; a.nq = nq; a.mode = in.mode;
  const unsigned rule = gmr::clip_waves(gmr::kMirrorTargetWaves, in.n_seq, gmr::mean_clip_tiles(in.n_frames, in.n_seq, gmr::kMirrorTile));
  const unsigned ty = (unsigned)gmr::env_int("GMR_AMD_MIRROR_WAVES", 1, gmr::kGridYMax, rule);
  hipLaunchKernelGGL(gmr::motion_mirror_kernel, dim3((unsigned)in.n_seq, ty), dim3(gmr::kFkWave), 0, st, a);
  if (hipGetLastError() != hipSuccess) { set_err(m, "kernel launch failed"); return GMR_EDEVICE; }
  return GMR_OK;
}

int gmr_motion_mirror(gmr_model *m, const gmr_mirror_input *in) {
  if (!m) return GMR_EINVAL;
  m->err.clear();
  if (!in) { set_err(m, "null input"); return GMR_EINVAL; }
  if (in->n_frames < 0 || in->n_seq < 0) { set_err(m, "negative count"); return GMR_EINVAL; }
  if (in->mode != GMR_MIRROR_WORLD && in->mode != GMR_MIRROR_CLIP_START) { set_err(m, "unknown mode %d", (int)in->mode); return GMR_EINVAL; }
  if (m->dm.root_planar) { set_err(m, "mirroring needs a free-joint root; a planar base is not supported"); return GMR_EUNSUPPORTED; }
  const int nq = m->fk.ndof + 7;
  if (nq > gmr::kMirrorMaxNq) { set_err(m, "a row of %d columns does not fit one wavefront", nq); return GMR_EUNSUPPORTED; }
  if (in->n_frames == 0 || in->n_seq == 0) return GMR_OK;   // (an array of no rows may well be a NULL pointer)
  if (!in->qpos || !in->qpos_out || !in->seq_offsets || !in->col_src || !in->col_sign) { set_err(m, "null argument"); return GMR_EINVAL; }
  if (in->qpos_out == in->qpos) { set_err(m, "qpos_out must not be qpos: a row is permuted"); return GMR_EINVAL; }
  return mirror_run(m, *in, nq, static_cast<hipStream_t>(in->stream));
}

// ------------------------------------------------------------------ composed clips (compose_kernel.hip.h)
// The two launches of gmr_motion_compose, and nothing else: no allocation, no copy, no synchronisation.  The plan kernel takes one
// wavefront per output clip.  The grid of the other is (segments, wavefronts per segment) by the grid rule of clip_launch.h, a segment
// standing for a clip, over the mean segment's tiles.  GMR_AMD_COMPOSE_WAVES forces a number (the results do not depend on it).
static int compose_run(gmr_model *m, const gmr_compose_input &in, int nq, hipStream_t st) {
  if (hipSetDevice(m->device) != hipSuccess) { set_err(m, "hipSetDevice failed"); return GMR_EDEVICE; }
  gmr::ComposeArgs a{};
  a.qpos = in.qpos; a.out = in.qpos_out; a.seg_transform = in.seg_transform; a.seg_src = in.seg_src; a.seg_len = in.seg_len;
  a.seg_blend = in.seg_blend; a.seg_out = in.seg_out; a.clip_segs = in.clip_segs;
  a.n_frames = in.n_frames; a.n_out_frames = in.n_out_frames; a.n_seg = in.n_seg; a.n_out = in.n_out; a.nq = nq;
  const unsigned rule = gmr::clip_waves(gmr::kComposeTargetWaves, in.n_seg, gmr::mean_clip_tiles(in.n_out_frames, in.n_seg, gmr::kComposeTile));
  const unsigned ty = (unsigned)gmr::env_int("GMR_AMD_COMPOSE_WAVES", 1, gmr::kGridYMax, rule);
  hipLaunchKernelGGL(gmr::motion_compose_plan_kernel, dim3((unsigned)in.n_out), dim3(gmr::kFkWave), 0, st, a);
  if (hipGetLastError() != hipSuccess) { set_err(m, "kernel launch failed"); return GMR_EDEVICE; }
  hipLaunchKernelGGL(gmr::motion_compose_kernel, dim3((unsigned)in.n_seg, ty), dim3(gmr::kFkWave), 0, st, a);
  if (hipGetLastError() != hipSuccess) { set_err(m, "kernel launch failed"); return GMR_EDEVICE; }
  return GMR_OK;
}

int gmr_motion_compose(gmr_model *m, const gmr_compose_input *in) {
  if (!m) return GMR_EINVAL;
  m->err.clear();
  if (!in) { set_err(m, "null input"); return GMR_EINVAL; }
  if (in->n_frames < 0 || in->n_seg < 0 || in->n_out < 0 || in->n_out_frames < 0) { set_err(m, "negative count"); return GMR_EINVAL; }
  if (m->dm.root_planar) { set_err(m, "composing needs a free-joint root; a planar base is not supported"); return GMR_EUNSUPPORTED; }
  const int nq = m->fk.ndof + 7;
  if (nq > gmr::kComposeMaxNq) { set_err(m, "a row of %d columns does not fit one wavefront", nq); return GMR_EUNSUPPORTED; }
  if (in->n_seg == 0 || in->n_out == 0 || in->n_out_frames == 0) return GMR_OK;   // (an array of no rows may well be a NULL pointer)
  if (!in->qpos || !in->qpos_out || !in->seg_transform || !in->seg_src || !in->seg_len || !in->seg_blend || !in->seg_out || !in->clip_segs) {
    set_err(m, "null argument"); return GMR_EINVAL;
  }
  if (in->n_frames == 0) { set_err(m, "segments of a motion without frames"); return GMR_EINVAL; }
  if (in->qpos_out == in->qpos) { set_err(m, "qpos_out must not be qpos: an output row reads other rows"); return GMR_EINVAL; }
  return compose_run(m, *in, nq, static_cast<hipStream_t>(in->stream));
}

// ------------------------------------------------------------------ transition search (transitions_kernel.hip.h)
// The three launches of gmr_motion_transitions, and nothing else: no allocation, no copy, no synchronisation.  Kernels a and b take
// (clips, wavefronts per clip) as the self-collision kernel does.  Kernel c takes one wavefront per work item (a run of `tile`
// sources, a target clip), at most kTrPairWaves of them: each strides over the items.  GMR_AMD_TRANSITIONS_WAVES forces the
// wavefronts per clip of a and b and the wavefronts of c, GMR_AMD_TRANSITIONS_TILE the sources of a work item (the results depend
// on neither).
static int transitions_run(gmr_model *m, const gmr_transitions_input &in, hipStream_t st) {
  if (hipSetDevice(m->device) != hipSuccess) { set_err(m, "hipSetDevice failed"); return GMR_EDEVICE; }
  gmr::TransitionsArgs a{};
  a.dm = m->dm_eval_dev;
  a.qpos = in.qpos; a.seq_offsets = in.seq_offsets; a.n_frames = in.n_frames;
  a.n_seq = in.n_seq; a.nbody = m->h.nbody; a.nq = m->fk.ndof + 7; a.P = in.n_bodies; a.L = in.window; a.stride = in.src_stride;
  a.min_gap = in.min_gap; a.n_src = in.n_src_clips; a.n_dst = in.n_dst_clips;
  a.body_ids = in.body_ids; a.weights = in.weights; a.src_clips = in.src_clips; a.dst_clips = in.dst_clips;
  a.src_offsets = in.src_offsets; a.dst_offsets = in.dst_offsets; a.n_sources = in.n_sources; a.n_targets = in.n_targets;
  a.points = in.points; a.moments = in.moments; a.best_cost = in.best_cost; a.best_frame = in.best_frame; a.cost_out = in.cost_out;
  gmr::tree_parent_depth(blob_ptr<int32_t>(m->blob, m->h.off_parent), a.nbody, a.parent, a.depth);
  a.tile = (int)gmr::env_int("GMR_AMD_TRANSITIONS_TILE", 1, gmr::kTrMaxTile, gmr::kTrTile);
  unsigned ta = gmr::clip_waves(gmr::kTrTargetWaves, in.n_seq, gmr::mean_clip_slots(in.n_frames, gmr::chain_geom(a.nbody).groups, in.n_seq));
  unsigned tb = gmr::clip_waves(gmr::kTrTargetWaves, in.n_seq, gmr::mean_clip_tiles(in.n_frames, in.n_seq, gmr::kFkWave));
  unsigned tc = gmr::transitions_pair_waves(in.n_sources, a.tile, in.n_dst_clips, gmr::kTrPairWaves);
  if (const long forced = gmr::env_int("GMR_AMD_TRANSITIONS_WAVES", 1, gmr::kGridYMax, 0)) ta = tb = tc = (unsigned)forced;
  const unsigned bytes = (unsigned)gmr::transitions_pair_lds_bytes(a.P, a.tile);
  hipLaunchKernelGGL(gmr::motion_transitions_points_kernel, dim3((unsigned)in.n_seq, ta), dim3(gmr::kFkWave), 0, st, a);
  hipLaunchKernelGGL(gmr::motion_transitions_window_kernel, dim3((unsigned)in.n_seq, tb), dim3(gmr::kFkWave), 0, st, a);
  if (in.window <= 8) hipLaunchKernelGGL(gmr::motion_transitions_pair_kernel<8>, dim3(tc), dim3(gmr::kFkWave), bytes, st, a);
  else hipLaunchKernelGGL(gmr::motion_transitions_pair_kernel<gmr::kTrMaxWindow>, dim3(tc), dim3(gmr::kFkWave), bytes, st, a);
  if (hipGetLastError() != hipSuccess) { set_err(m, "kernel launch failed"); return GMR_EDEVICE; }
  return GMR_OK;
}

int gmr_motion_transitions(gmr_model *m, const gmr_transitions_input *in) {
  if (!m) return GMR_EINVAL;
  m->err.clear();
  if (!in) { set_err(m, "null input"); return GMR_EINVAL; }
  if (in->n_frames < 0 || in->n_seq < 0 || in->n_src_clips < 0 || in->n_dst_clips < 0 || in->n_sources < 0 || in->n_targets < 0) {
    set_err(m, "negative count"); return GMR_EINVAL;
  }
  if (in->window < 1) { set_err(m, "window must be at least 1"); return GMR_EINVAL; }
  if (in->src_stride < 1) { set_err(m, "src_stride must be at least 1"); return GMR_EINVAL; }
  if (in->n_bodies < 1) { set_err(m, "n_bodies must be at least 1"); return GMR_EINVAL; }
  if (in->min_gap < 0) { set_err(m, "min_gap must not be negative"); return GMR_EINVAL; }
  const int nb = m->h.nbody;
  if (nb > gmr::kFkWave) { set_err(m, "a model of %d bodies does not fit the transition search's pose tile", nb); return GMR_EUNSUPPORTED; }
  if (in->n_bodies > gmr::kTrMaxBodies) { set_err(m, "at most %d bodies per call", gmr::kTrMaxBodies); return GMR_EUNSUPPORTED; }
  if (in->window > gmr::kTrMaxWindow) { set_err(m, "a window of at most %d frames", gmr::kTrMaxWindow); return GMR_EUNSUPPORTED; }
  if (in->n_frames == 0 || in->n_seq == 0 || in->n_src_clips == 0 || in->n_dst_clips == 0 || in->n_sources == 0) return GMR_OK;   // (an array of no rows may well be a NULL pointer)
  if (!in->qpos || !in->seq_offsets || !in->body_ids || !in->weights || !in->src_clips || !in->src_offsets || !in->dst_clips ||
      !in->points || !in->moments || !in->best_cost || !in->best_frame) {
    set_err(m, "null argument"); return GMR_EINVAL;
  }
  if (in->cost_out && !in->dst_offsets) { set_err(m, "null argument: cost_out needs dst_offsets"); return GMR_EINVAL; }
  return transitions_run(m, *in, static_cast<hipStream_t>(in->stream));
}

// ------------------------------------------------------------------ retiming to velocity limits (retime_kernel.hip.h)
// The launches of gmr_motion_retime_plan (three) and gmr_motion_retime_apply (one), and nothing else: no allocation, no copy, no
// synchronisation.  The need, ticks and apply kernels take the grid (clips, wavefronts per clip) by the grid rule of clip_launch.h
// over the mean clip's tiles of input (apply: output) rows; the scan kernel takes one wavefront per clip.  GMR_AMD_RETIME_WAVES
// forces the wavefronts per clip (the results do not depend on it).
static unsigned retime_clip_waves(int64_t n_rows, int64_t n_seq) {
  const unsigned rule = gmr::clip_waves(gmr::kRetimeTargetWaves, n_seq, gmr::mean_clip_tiles(n_rows, n_seq, gmr::kRetimeTile));
  return (unsigned)gmr::env_int("GMR_AMD_RETIME_WAVES", 1, gmr::kGridYMax, rule);
}

static int retime_plan_run(gmr_model *m, const gmr_retime_plan_input &in, int nq, hipStream_t st) {
  if (hipSetDevice(m->device) != hipSuccess) { set_err(m, "hipSetDevice failed"); return GMR_EDEVICE; }
  gmr::RetimePlanArgs a{};
  a.qpos = in.qpos; a.seq_offsets = in.seq_offsets; a.vmax = in.vmax; a.need = in.need; a.ticks = in.ticks; a.cum = in.cum;
  a.out_len = in.out_len; a.clip_stats = in.clip_stats; a.need_max = in.need_max;
  a.fps = in.fps; a.max_stretch = in.max_stretch; a.n_frames = in.n_frames; a.n_seq = in.n_seq; a.nq = nq; a.window = in.window;
  if (in.n_frames > 0) {  // (without frames every clip is empty: only the per-clip results are written)
    const unsigned ty = retime_clip_waves(in.n_frames, in.n_seq);
    hipLaunchKernelGGL(gmr::motion_retime_need_kernel, dim3((unsigned)in.n_seq, ty), dim3(gmr::kFkWave), 0, st, a);
    hipLaunchKernelGGL(gmr::motion_retime_ticks_kernel, dim3((unsigned)in.n_seq, ty), dim3(gmr::kFkWave), 0, st, a);
  }
  hipLaunchKernelGGL(gmr::motion_retime_scan_kernel, dim3((unsigned)in.n_seq), dim3(gmr::kFkWave), 0, st, a);
  if (hipGetLastError() != hipSuccess) { set_err(m, "kernel launch failed"); return GMR_EDEVICE; }
  return GMR_OK;
}

int gmr_motion_retime_plan(gmr_model *m, const gmr_retime_plan_input *in) {
  if (!m) return GMR_EINVAL;
  m->err.clear();
  if (!in) { set_err(m, "null input"); return GMR_EINVAL; }
  if (in->n_frames < 0 || in->n_seq < 0) { set_err(m, "negative count"); return GMR_EINVAL; }
  if (in->window < 0 || in->window > gmr::kRetimeMaxWindow) { set_err(m, "window must be 0 .. %d", gmr::kRetimeMaxWindow); return GMR_EINVAL; }
  if (!(in->max_stretch >= 1.0) || !(in->max_stretch <= 64.0)) { set_err(m, "max_stretch must be 1 .. 64"); return GMR_EINVAL; }
  if (!std::isfinite(in->fps) || !(in->fps > 0.0)) { set_err(m, "fps must be finite and > 0"); return GMR_EINVAL; }
  if (m->dm.root_planar) { set_err(m, "retiming needs a free-joint root; a planar base is not supported"); return GMR_EUNSUPPORTED; }
  const int nq = m->fk.ndof + 7;
  if (nq > gmr::kRetimeMaxNq) { set_err(m, "a row of %d columns does not fit one wavefront", nq); return GMR_EUNSUPPORTED; }
  if (in->n_seq == 0) return GMR_OK;   // (an array of no rows may well be a NULL pointer)
  if (!in->seq_offsets || !in->out_len || !in->clip_stats || !in->need_max) { set_err(m, "null argument"); return GMR_EINVAL; }
  if (in->n_frames > 0 && (!in->qpos || !in->need || !in->ticks || !in->cum || (nq > 7 && !in->vmax))) { set_err(m, "null argument"); return GMR_EINVAL; }
  return retime_plan_run(m, *in, nq, static_cast<hipStream_t>(in->stream));
}

static int retime_apply_run(gmr_model *m, const gmr_retime_apply_input &in, int nq, hipStream_t st) {
  if (hipSetDevice(m->device) != hipSuccess) { set_err(m, "hipSetDevice failed"); return GMR_EDEVICE; }
  gmr::RetimeApplyArgs a{};
  a.qpos = in.qpos; a.seq_offsets = in.seq_offsets; a.out_offsets = in.out_offsets; a.ticks = in.ticks; a.cum = in.cum;
  a.out = in.qpos_out; a.src_time = in.src_time;
  a.n_frames = in.n_frames; a.n_out_frames = in.n_out_frames; a.n_seq = in.n_seq; a.nq = nq;
  const unsigned ty = retime_clip_waves(in.n_out_frames, in.n_seq);
  const auto kernel = in.interp == GMR_RETIME_INTERP_CUBIC ? gmr::motion_retime_apply_cubic_kernel : gmr::motion_retime_apply_kernel;
  hipLaunchKernelGGL(kernel, dim3((unsigned)in.n_seq, ty), dim3(gmr::kFkWave), 0, st, a);
  if (hipGetLastError() != hipSuccess) { set_err(m, "kernel launch failed"); return GMR_EDEVICE; }
  return GMR_OK;
}

int gmr_motion_retime_apply(gmr_model *m, const gmr_retime_apply_input *in) {
  if (!m) return GMR_EINVAL;
  m->err.clear();
  if (!in) { set_err(m, "null input"); return GMR_EINVAL; }
  if (in->n_frames < 0 || in->n_seq < 0 || in->n_out_frames < 0) { set_err(m, "negative count"); return GMR_EINVAL; }
  if (in->interp != GMR_RETIME_INTERP_LINEAR && in->interp != GMR_RETIME_INTERP_CUBIC) { set_err(m, "interp must be 0 (linear) or 1 (cubic)"); return GMR_EINVAL; }
  if (m->dm.root_planar) { set_err(m, "retiming needs a free-joint root; a planar base is not supported"); return GMR_EUNSUPPORTED; }
  const int nq = m->fk.ndof + 7;
  if (nq > gmr::kRetimeMaxNq) { set_err(m, "a row of %d columns does not fit one wavefront", nq); return GMR_EUNSUPPORTED; }
  if (in->n_seq == 0 || in->n_frames == 0 || in->n_out_frames == 0) return GMR_OK;   // (an array of no rows may well be a NULL pointer)
  if (!in->qpos || !in->seq_offsets || !in->ticks || !in->cum || !in->out_offsets || !in->qpos_out || !in->src_time) {
    set_err(m, "null argument"); return GMR_EINVAL;
  }
  if (in->qpos_out == in->qpos) { set_err(m, "qpos_out must not be qpos: an output row reads other rows"); return GMR_EINVAL; }
  return retime_apply_run(m, *in, nq, static_cast<hipStream_t>(in->stream));
}

// ------------------------------------------------------------------ retiming to torque limits (retime_torque_kernel.hip.h)
// The launches of gmr_motion_retime_plan_torque and nothing else: the torque need kernel in the place of the velocity one, the
// ticks and scan kernels of the velocity plan as they are, and with align_end the alignment kernel, one wavefront per clip.
static int retime_torque_run(gmr_model *m, const gmr_retime_torque_input &in, int nq, hipStream_t st) {
  if (hipSetDevice(m->device) != hipSuccess) { set_err(m, "hipSetDevice failed"); return GMR_EDEVICE; }
  gmr::RetimeTorqueArgs t{};
  t.tau = in.tau; t.tau_static = in.tau_static; t.seq_offsets = in.seq_offsets; t.torque_limit = in.torque_limit;
  t.need_floor = in.need_floor; t.need = in.need; t.static_over = in.static_over;
  t.limit_scale = in.limit_scale; t.n_frames = in.n_frames; t.n_seq = in.n_seq; t.nh = nq - 7;
  gmr::RetimePlanArgs a{};  // (qpos, vmax and fps are the velocity need kernel's alone)
  a.seq_offsets = in.seq_offsets; a.need = in.need; a.ticks = in.ticks; a.cum = in.cum;
  a.out_len = in.out_len; a.clip_stats = in.clip_stats; a.need_max = in.need_max;
  a.max_stretch = in.max_stretch; a.n_frames = in.n_frames; a.n_seq = in.n_seq; a.nq = nq; a.window = in.window;
  if (in.n_frames > 0) {  // (without frames every clip is empty: only the per-clip results are written)
    const unsigned ty = retime_clip_waves(in.n_frames, in.n_seq);
    hipLaunchKernelGGL(gmr::motion_retime_torque_need_kernel, dim3((unsigned)in.n_seq, ty), dim3(gmr::kFkWave), 0, st, t);
    hipLaunchKernelGGL(gmr::motion_retime_ticks_kernel, dim3((unsigned)in.n_seq, ty), dim3(gmr::kFkWave), 0, st, a);
  }
  hipLaunchKernelGGL(gmr::motion_retime_scan_kernel, dim3((unsigned)in.n_seq), dim3(gmr::kFkWave), 0, st, a);
  if (in.align_end && in.n_frames > 0) {
    gmr::RetimeAlignArgs g{};
    g.seq_offsets = in.seq_offsets; g.ticks = in.ticks; g.cum = in.cum; g.out_len = in.out_len; g.clip_stats = in.clip_stats;
    g.n_frames = in.n_frames; g.n_seq = in.n_seq;
    hipLaunchKernelGGL(gmr::motion_retime_align_kernel, dim3((unsigned)in.n_seq), dim3(gmr::kFkWave), 0, st, g);
  }
  if (hipGetLastError() != hipSuccess) { set_err(m, "kernel launch failed"); return GMR_EDEVICE; }
  return GMR_OK;
}

int gmr_motion_retime_plan_torque(gmr_model *m, const gmr_retime_torque_input *in) {
  if (!m) return GMR_EINVAL;
  m->err.clear();
  if (!in) { set_err(m, "null input"); return GMR_EINVAL; }
  if (in->n_frames < 0 || in->n_seq < 0) { set_err(m, "negative count"); return GMR_EINVAL; }
  if (in->window < 0 || in->window > gmr::kRetimeMaxWindow) { set_err(m, "window must be 0 .. %d", gmr::kRetimeMaxWindow); return GMR_EINVAL; }
  if (!(in->max_stretch >= 1.0) || !(in->max_stretch <= 64.0)) { set_err(m, "max_stretch must be 1 .. 64"); return GMR_EINVAL; }
  if (!(in->limit_scale > 0.0) || !(in->limit_scale <= 1.0)) { set_err(m, "limit_scale must be > 0 and <= 1"); return GMR_EINVAL; }
  if (in->align_end != 0 && in->align_end != 1) { set_err(m, "align_end must be 0 or 1"); return GMR_EINVAL; }
  if (m->dm.root_planar) { set_err(m, "retiming needs a free-joint root; a planar base is not supported"); return GMR_EUNSUPPORTED; }
  const int nq = m->fk.ndof + 7;
  if (nq > gmr::kRetimeMaxNq) { set_err(m, "a row of %d columns does not fit one wavefront", nq); return GMR_EUNSUPPORTED; }
  if (in->n_seq == 0) return GMR_OK;   // (an array of no rows may well be a NULL pointer)
  if (!in->seq_offsets || !in->out_len || !in->clip_stats || !in->need_max) { set_err(m, "null argument"); return GMR_EINVAL; }
  if (in->n_frames > 0 && (!in->need || !in->ticks || !in->cum || (nq > 7 && (!in->tau || !in->tau_static || !in->torque_limit)))) {
    set_err(m, "null argument"); return GMR_EINVAL;
  }
  return retime_torque_run(m, *in, nq, static_cast<hipStream_t>(in->stream));
}

// ------------------------------------------------------------------ clip report (report_kernel.hip.h)
// Validate every member with clips, send the entries, clip offsets, segment prefixes and slot columns in one call block
// ("the call block"; the segments' partial rows are its device-only tail), run pass 1 over all members' segments in
// one grid and pass 2 over all members' clips in a second.
static int report_run(const Members &g, const gmr_clip_report_input *inputs, const gmr_clip_report_params *prm, hipStream_t st) {
  struct Member {
    bool work = false, kp = false;
    gmr::CallBlock::Uploaded<int64_t> offs;
    gmr::CallBlock::Uploaded<int> clip_seg, slot_col;  // slot_col: members with key-points only
    gmr::CallBlock::DeviceOnly<unsigned long long> rows;
  };
  const int n = g.n;
  std::string &err = g.err;
  gmr_clip_report_params p{};
  if (prm) p = *prm; else p.limit_eps = GMR_CLIP_REPORT_LIMIT_EPS;
  if (p.segment_frames < 0) { err = "negative segment_frames"; return GMR_EINVAL; }
  if (!(p.limit_eps >= 0.0)) { err = "limit_eps must be >= 0"; return GMR_EINVAL; }
  const int segment = p.segment_frames ? p.segment_frames : GMR_CLIP_REPORT_SEGMENT;
  gmr::CallBlock blk;
  const auto h_ent = blk.uploaded<gmr::ReportEntry>((size_t)n);
  std::vector<gmr::ReportEntry> ent(n);
  std::vector<Member> mem(n);
  int64_t segs = 0, clips = 0;
  int lds = 0;
  for (int i = 0; i < n; ++i) {
    const gmr_clip_report_input &in = inputs[i];
    const gmr_model *m = g.models[i];
    const std::string who = g.who(i);
    gmr::ReportEntry &e = ent[i];
    e.seg_base = segs; e.clip_base = clips;
    if (in.n_frames < 0 || in.n_seq < 0) { err = who + "negative size"; return GMR_EINVAL; }
    if (in.n_seq == 0 && in.n_frames == 0) continue;  // no work for this member
    if (const char *why = seq_offsets_error(in.seq_offsets, in.n_seq, in.n_frames)) { err = who + why; return GMR_EINVAL; }
    if (in.n_frames > 0 && !in.qpos) { err = who + "null qpos"; return GMR_EINVAL; }
    const bool want_err = in.err_max_out || in.err_sum_out || in.task_pos_max_out || in.task_pos_sum_out || in.task_rot_max_out || in.task_rot_sum_out;
    const bool have_kp = in.n_frames > 0 && (in.human_pos || in.human_quat);  // (no frames: nothing is read, every clip reports 0)
    if (want_err && !have_kp && in.n_frames > 0) { err = who + "the error fields need the human key-points"; return GMR_EINVAL; }
    if (have_kp) {
      if (m->h.nslot == 0) { err = who + "model has no IK config"; return GMR_ENOCONFIG; }
      if (!in.human_pos || !in.human_quat || !in.slot_col || in.n_cols <= 0 || (in.in_dtype != GMR_DTYPE_F32 && in.in_dtype != GMR_DTYPE_F64)) {
        err = who + "the key-points need both arrays, their dtype and slot_col"; return GMR_EINVAL;
      }
      for (int s = 0; s < m->h.nslot; ++s)
        if (in.slot_col[s] < 0 || in.slot_col[s] >= in.n_cols) {
          err = who + "slot_col[" + std::to_string(s) + "]=" + std::to_string(in.slot_col[s]) + " outside [0," + std::to_string(in.n_cols) + ")";
          return GMR_EINVAL;
        }
    }
    Member &mb = mem[i];
    mb.clip_seg = blk.uploaded<int>((size_t)in.n_seq + 1);
    int *cs = blk[mb.clip_seg];  // (filled before the next reservation moves the image)
    int64_t acc = 0;
    for (int s = 0; s < in.n_seq; ++s) {
      acc += (in.seq_offsets[s + 1] - in.seq_offsets[s] + segment - 1) / segment;
      if (acc > 0x7fffffff) { err = who + "too many segments for one launch"; return GMR_EINVAL; }
      cs[s + 1] = (int)acc;
    }
    mb.work = true;
    mb.offs = blk.put(in.seq_offsets, (size_t)in.n_seq + 1);
    e.m = m->dm_eval_dev; e.lay = m->lay_eval;
    e.qpos = in.qpos;
    if (have_kp) {
      e.hpos = in.human_pos; e.hquat = in.human_quat;
      e.in_f64 = in.in_dtype == GMR_DTYPE_F64; e.n_cols = in.n_cols;
      mb.kp = true;
      mb.slot_col = blk.put(in.slot_col, (size_t)m->h.nslot);
    }
    e.hscale = in.height_scale; e.iters = in.iters;
    e.hlo = m->rep_lo; e.hhi = m->rep_hi;
    e.nh = m->h.nq - 7; e.nt = m->h.ntask[0] + m->h.ntask[1];
    mb.rows = blk.device_only<unsigned long long>((size_t)acc * gmr::report_row_words(e.nt, e.nh));
    e.err_max = in.err_max_out; e.err_sum = in.err_sum_out;
    e.task_pos_max = in.task_pos_max_out; e.task_pos_sum = in.task_pos_sum_out;
    e.task_rot_max = in.task_rot_max_out; e.task_rot_sum = in.task_rot_sum_out;
    e.dof_step_max = in.dof_step_max_out; e.root_step_max = in.root_step_max_out; e.root_turn_max = in.root_turn_max_out;
    e.near_lo = in.near_lo_out; e.near_hi = in.near_hi_out; e.solves_max = in.solves_max_out; e.solves_sum = reinterpret_cast<long long *>(in.solves_sum_out);
    e.nonfinite = in.nonfinite_frames_out;
    e.limit_eps = p.limit_eps;
    e.n_seq = in.n_seq; e.offset_to_ground = p.offset_to_ground ? 1 : 0; e.segment = segment;
    lds = std::max(lds, m->lds_bytes_eval + ((m->h.nq + 1) & ~1) * (int)sizeof(double));
    segs += acc; clips += in.n_seq;
  }
  if (clips == 0) return GMR_OK;
  if (segs > 0x7fffffff || clips > 0x7fffffff) { err = "too many clips for one launch"; return GMR_EINVAL; }
  if (hipSetDevice(g.device) != hipSuccess) { err = "hipSetDevice failed"; return GMR_EDEVICE; }
  CallScratch sc;
  const int rc = send_call_block(g, blk, sc, st, [&](const gmr::CallBlock::Device &dev) {
    for (int i = 0; i < n; ++i) {
      const Member &mb = mem[i];
      if (!mb.work) continue;
      gmr::ReportEntry &e = ent[i];
      e.offs = dev(mb.offs); e.clip_seg = dev(mb.clip_seg); e.rows = dev(mb.rows);
      if (mb.kp) e.slot_col = dev(mb.slot_col);
    }
    std::copy(ent.begin(), ent.end(), blk[h_ent]);
    return GMR_OK;
  });
  if (rc != GMR_OK) return rc;
  const gmr::ReportEntry *d_ent = blk.on(sc.p)(h_ent);
  if (segs > 0) hipLaunchKernelGGL(gmr::clip_report_kernel, dim3((unsigned)segs), dim3(64), (unsigned)lds, st, d_ent, n);
  hipLaunchKernelGGL(gmr::clip_report_merge_kernel, dim3((unsigned)clips), dim3(gmr::kReportMergeThreads), 0, st, d_ent, n);
  if (hipGetLastError() != hipSuccess) { err = "kernel launch failed"; return GMR_EDEVICE; }
  return GMR_OK;
}

int gmr_clip_report(gmr_model *m, const gmr_clip_report_input *in, const gmr_clip_report_params *prm, void *stream) {
  return member_call(m, nullptr, in, [&](const Members &g) { return report_run(g, in, prm, static_cast<hipStream_t>(stream)); });
}

int gmr_group_clip_report(gmr_group *g, const gmr_clip_report_input *inputs, const gmr_clip_report_params *prm, void *stream) {
  return member_call(nullptr, g, inputs, [&](const Members &ms) { return report_run(ms, inputs, prm, static_cast<hipStream_t>(stream)); });
}

/* Frames per wavefront of the adapter kernels: runs long enough that a wavefront's setup (plan, tables) is amortised and its
 * consecutive output rows complete each other's cache lines, short enough that a small clip still fills the chip. */
static int adapter_chunk(int64_t n_frames, int groups) {
  int64_t c = (n_frames + 16383) / 16384;  /* ~16 k wavefronts = 16 per SIMD on 256 CUs when there is that much work */
  c = std::max<int64_t>(c, 8);
  c = std::min<int64_t>(c, 64);
  c = (c + groups - 1) / groups * groups;
  return (int)c;
}

/* The skeleton the SMPL-X kernels work on: the joints emitted (out_cols, NULL = all) and their ancestors, renumbered in order
 * (a parent precedes its children, the root stays first).  Fills n_joints, n_out, parent, out_col, src. */
static int smpl_live_skeleton(const int32_t *parents, int n_joints, const int32_t *out_cols, int n_out, gmr::SmplSkeleton &sk) {
  if (parents[0] != -1) return GMR_EINVAL;
  for (int j = 1; j < n_joints; ++j)
    if (parents[j] < 0 || parents[j] >= j) return GMR_EINVAL;
  short col_of[gmr::kSmplMaxJoints];      /* output column of model joint j, -1 = not emitted */
  unsigned char live[gmr::kSmplMaxJoints]; /* emitted, or an ancestor of an emitted joint */
  if (out_cols) {  /* out_cols[c] = joint emitted as column c; ancestors are chained internally */
    if (n_out < 1 || n_out > n_joints) return GMR_EINVAL;
    for (int j = 0; j < n_joints; ++j) { col_of[j] = -1; live[j] = 0; }
    for (int c = 0; c < n_out; ++c) {
      const int j = out_cols[c];
      if (j < 0 || j >= n_joints || col_of[j] >= 0) return GMR_EINVAL;
      col_of[j] = (short)c;
      for (int a = j; a >= 0 && !live[a]; a = parents[a]) live[a] = 1;
    }
    sk.n_out = n_out;
  } else {
    for (int j = 0; j < n_joints; ++j) { col_of[j] = (short)j; live[j] = 1; }
    sk.n_out = n_joints;
  }
  short cidx[gmr::kSmplMaxJoints];
  int nl = 0;
  for (int j = 0; j < n_joints; ++j) {
    cidx[j] = -1;
    if (!live[j]) continue;
    cidx[j] = (short)nl;
    sk.src[nl] = (short)j;
    sk.out_col[nl] = col_of[j];
    sk.parent[nl] = j == 0 ? (short)-1 : cidx[parents[j]];
    ++nl;
  }
  sk.n_joints = nl;
  return GMR_OK;
}

int gmr_smplx_keypoints_cols(const int32_t *parents, int n_joints, int joints_stride, const double *global_orient, const double *full_pose,
                             const double *joints, int64_t n_frames, int64_t n_frames_out, int resample, const int32_t *out_cols, int n_out,
                             double *pos_out, double *quat_out, void *stream) {
  return gmr_smplx_keypoints_in(parents, n_joints, joints_stride, global_orient, full_pose, joints, GMR_DTYPE_F64, n_frames, n_frames_out, resample,
                                out_cols, n_out, pos_out, quat_out, stream);
}

int gmr_smplx_keypoints_in(const int32_t *parents, int n_joints, int joints_stride, const void *global_orient, const void *full_pose,
                           const void *joints, int in_dtype, int64_t n_frames, int64_t n_frames_out, int resample, const int32_t *out_cols, int n_out,
                           double *pos_out, double *quat_out, void *stream) {
  if (!parents || !global_orient || !full_pose || !joints || !pos_out || !quat_out || n_frames < 0 || n_frames_out < 0) return GMR_EINVAL;
  if (in_dtype != GMR_DTYPE_F32 && in_dtype != GMR_DTYPE_F64) return GMR_EINVAL;
  if (n_joints < 1 || n_joints > gmr::kSmplMaxJoints || joints_stride < n_joints) return GMR_EUNSUPPORTED;
  if (!resample && n_frames_out != n_frames) return GMR_EINVAL;
  if (n_frames_out > 0 && n_frames == 0) return GMR_EINVAL;
  gmr::SmplSkeleton sk{};
  sk.joints_stride = joints_stride; sk.pose_stride = n_joints; sk.resample = resample ? 1 : 0;
  if (const int rc = smpl_live_skeleton(parents, n_joints, out_cols, n_out, sk)) return rc;
  const int nl = sk.n_joints;
  if (n_frames_out == 0) return GMR_OK;
  const int chunk = adapter_chunk(n_frames_out, gmr::chain_geom(nl).groups);
  const int64_t nblk = (n_frames_out + chunk - 1) / chunk;
  if (nblk > 0x7fffffff) return GMR_EINVAL;
  if (in_dtype == GMR_DTYPE_F32)
    hipLaunchKernelGGL(gmr::smplx_keypoints_kernel<float>, dim3((unsigned)nblk), dim3(64), 0, static_cast<hipStream_t>(stream), sk,
                       static_cast<const float *>(global_orient), static_cast<const float *>(full_pose), static_cast<const float *>(joints), n_frames,
                       n_frames_out, chunk, pos_out, quat_out);
  else
    hipLaunchKernelGGL(gmr::smplx_keypoints_kernel<double>, dim3((unsigned)nblk), dim3(64), 0, static_cast<hipStream_t>(stream), sk,
                       static_cast<const double *>(global_orient), static_cast<const double *>(full_pose), static_cast<const double *>(joints), n_frames,
                       n_frames_out, chunk, pos_out, quat_out);
  return hipGetLastError() == hipSuccess ? GMR_OK : GMR_EDEVICE;
}

int gmr_smplx_keypoints(const int32_t *parents, int n_joints, int joints_stride, const double *global_orient, const double *full_pose,
                        const double *joints, int64_t n_frames, int64_t n_frames_out, int resample, double *pos_out, double *quat_out,
                        void *stream) {
  return gmr_smplx_keypoints_cols(parents, n_joints, joints_stride, global_orient, full_pose, joints, n_frames, n_frames_out, resample,
                                  nullptr, 0, pos_out, quat_out, stream);
}

int gmr_smplx_body(const int32_t *parents, int n_joints, const gmr_smplx_body_clip *clips, int n_clips, const int32_t *out_cols, int n_out,
                   double *global_orient, double *full_pose, double *joints, double *rest_out, void *stream) {
  if (!parents || n_clips < 0 || (n_clips > 0 && !clips)) return GMR_EINVAL;
  if (n_joints != gmr::kBodyJoints) return GMR_EUNSUPPORTED;
  gmr::SmplSkeleton sk{};
  sk.joints_stride = n_joints; sk.pose_stride = n_joints;
  if (const int rc = smpl_live_skeleton(parents, n_joints, out_cols, n_out, sk)) return rc;
  if (n_clips == 0) return GMR_OK;
  const int groups = gmr::chain_geom(sk.n_joints).groups;
  int64_t total = 0;
  size_t n_betas = 0;
  for (int c = 0; c < n_clips; ++c) {
    const gmr_smplx_body_clip &in = clips[c];
    if (in.n_frames < 0 || in.n_betas < 0 || in.dirs_stride < in.n_betas || !in.j_template || !in.hand_mean) return GMR_EINVAL;
    if (in.n_betas > 0 && (!in.betas || !in.j_dirs)) return GMR_EINVAL;
    if (in.n_frames > 0 && (!in.root_orient || !in.pose_body || !in.trans)) return GMR_EINVAL;
    for (int k = 0; k < 3; ++k)
      if (in.in_dtype[k] != GMR_DTYPE_F32 && in.in_dtype[k] != GMR_DTYPE_F64) return GMR_EINVAL;
    total += in.n_frames;
    n_betas += (size_t)in.n_betas;
  }
  if (total > 0 && (!global_orient || !full_pose || !joints)) return GMR_EINVAL;
  /* the device the outputs live on (the rest skeletons' when there is not a single frame) */
  const void *where = total > 0 ? static_cast<const void *>(full_pose) : static_cast<const void *>(rest_out);
  if (!where) return GMR_OK;
  hipPointerAttribute_t attr{};
  if (hipPointerGetAttributes(&attr, where) != hipSuccess) { (void)hipGetLastError(); return GMR_EINVAL; }
  if (hipSetDevice(attr.device) != hipSuccess) return GMR_EDEVICE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int chunk = adapter_chunk(total, groups);
  const size_t clip_bytes = (sizeof(gmr::BodyClip) * (size_t)n_clips + 15) & ~size_t(15);
  const size_t rest_at = clip_bytes + sizeof(double) * n_betas;
  const size_t rest_doubles = (size_t)gmr::kBodyJoints * 3;
  const size_t bytes = rest_at + (rest_out ? 0 : sizeof(double) * rest_doubles * (size_t)n_clips);
  CallScratch sc;
  sc.st = st;
  hipMemPool_t pool = scratch_pool(attr.device);
  if ((pool ? hipMallocFromPoolAsync(&sc.p, bytes, pool, st) : hipMallocAsync(&sc.p, bytes, st)) != hipSuccess) { (void)hipGetLastError(); return GMR_EDEVICE; }
  uint8_t *ws = static_cast<uint8_t *>(sc.p);
  std::vector<uint8_t> host(rest_at, 0);
  gmr::BodyClip *hc = reinterpret_cast<gmr::BodyClip *>(host.data());
  double *hb = reinterpret_cast<double *>(host.data() + clip_bytes);
  double *rest = rest_out ? rest_out : reinterpret_cast<double *>(ws + rest_at);
  int64_t row = 0, blk = 0;
  size_t b_at = 0;
  for (int c = 0; c < n_clips; ++c) {
    const gmr_smplx_body_clip &in = clips[c];
    gmr::BodyClip &e = hc[c];
    e.root_orient = in.root_orient; e.pose_body = in.pose_body; e.trans = in.trans;
    e.j_template = in.j_template; e.j_dirs = in.j_dirs; e.hand_mean = in.hand_mean;
    e.betas = reinterpret_cast<const double *>(ws + clip_bytes) + b_at;
    if (in.n_betas > 0) memcpy(hb + b_at, in.betas, sizeof(double) * (size_t)in.n_betas);
    b_at += (size_t)in.n_betas;
    e.rest = rest + rest_doubles * (size_t)c;
    e.row0 = row; e.n_frames = in.n_frames; e.blk0 = blk;
    for (int k = 0; k < 3; ++k) e.dt[k] = in.in_dtype[k] == GMR_DTYPE_F64 ? 1 : 0;
    e.n_betas = in.n_betas; e.dirs_stride = in.dirs_stride;
    row += in.n_frames;
    blk += (in.n_frames + chunk - 1) / chunk;
  }
  if (blk > 0x7fffffff) return GMR_EINVAL;
  if (hipMemcpyAsync(ws, host.data(), rest_at, hipMemcpyHostToDevice, st) != hipSuccess) { (void)hipGetLastError(); return GMR_EDEVICE; }
  const auto *d_clips = reinterpret_cast<const gmr::BodyClip *>(ws);
  const int n_rest = n_clips * (int)rest_doubles;
  hipLaunchKernelGGL(gmr::smplx_rest_kernel, dim3((unsigned)((n_rest + 255) / 256)), dim3(256), 0, st, d_clips, n_clips);
  if (blk > 0)
    hipLaunchKernelGGL(gmr::smplx_body_kernel, dim3((unsigned)blk), dim3(64), 0, st, sk, d_clips, n_clips, chunk, global_orient, full_pose, joints);
  return hipGetLastError() == hipSuccess ? GMR_OK : GMR_EDEVICE;
}

int gmr_bvh_parse_header(const char *text, size_t len, int max_joints, char *names_out, size_t names_cap, int32_t *parents_out,
                         double *offsets_out, int32_t *channels_out, int32_t *order_out, int64_t *n_frames_out, double *frame_time_out,
                         size_t *motion_offset_out) {
  if (!text || max_joints <= 0 || !names_out || !parents_out || !offsets_out || !channels_out || !order_out || !n_frames_out ||
      !frame_time_out || !motion_offset_out)
    return -1;
  gmr_bvh::Cursor c{text, text + len};
  gmr_bvh::Header h{};
  h.max_joints = max_joints; h.names = names_out; h.names_cap = names_cap;
  h.parents = parents_out; h.offsets = offsets_out; h.channels = channels_out;
  if (!c.next() || !c.is("HIERARCHY") || !c.next() || !c.is("ROOT")) return -1;
  int rc = gmr_bvh::joint(c, h, -1, 0);
  if (rc) return rc;
  if (h.order[0] < 0) return -1;  // no joint names three rotation channels where the reference looks for the Euler order
  int64_t nf;
  double ft;
  if (!c.next() || !c.is("MOTION") || !c.next() || !c.is("Frames:") || !gmr_bvh::integer(c, nf) || !c.next() || !c.is("Frame") ||
      !c.next() || !c.is("Time:") || !gmr_bvh::number(c, ft))
    return -1;
  const char *p = c.p;  // the motion rows start behind the end of the Frame Time line
  while (p < text + len && *p != '\n') ++p;
  if (p < text + len) ++p;
  for (int i = 0; i < 3; ++i) order_out[i] = h.order[i];
  *n_frames_out = nf; *frame_time_out = ft; *motion_offset_out = (size_t)(p - text);
  return h.n;
}

int64_t gmr_bvh_parse_motion(const char *text, size_t len, int64_t max_lines, double *out, int64_t max_out, int64_t *n_lines,
                             int64_t *n_cols) {
  // Decimal -> double by Clinger's fast path: a mantissa below 2^53 and a power of ten up to 10^22 are both exact doubles, so
  // one multiply / divide gives the correctly rounded result (what Python's float() returns).  Anything else (more than 19
  // digits, huge exponents, inf / nan) goes through strtod.
  static const double p10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16,
                                 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  if (!text || !out || max_lines < 0 || max_out < 0) return -1;
  const char *p = text, *end = text + len;
  int64_t count = 0, lines = 0, cols0 = -1;
  while (p < end && lines < max_lines) {
    int64_t cols = 0;
    for (;;) {  // one line
      while (p < end && (*p == ' ' || *p == '\t' || *p == '\r')) ++p;
      if (p >= end || *p == '\n') break;
      const char *tok = p;
      bool neg = false;
      if (*p == '-' || *p == '+') { neg = *p == '-'; ++p; }
      uint64_t mant = 0;
      int nd = 0, e10 = 0;
      bool digits = false, fast = true;
      while (p < end && *p >= '0' && *p <= '9') {
        digits = true;
        if (nd < 19) { mant = mant * 10 + (uint64_t)(*p - '0'); if (mant) ++nd; } else fast = false;
        ++p;
      }
      if (p < end && *p == '.') {
        ++p;
        while (p < end && *p >= '0' && *p <= '9') {
          digits = true;
          if (nd < 19) { mant = mant * 10 + (uint64_t)(*p - '0'); if (mant) ++nd; --e10; } else fast = false;  // further digits: below 1 ulp of 19 digits, but be exact
          ++p;
        }
      }
      if (digits && p < end && (*p == 'e' || *p == 'E')) {
        const char *q = p + 1;
        bool eneg = false;
        if (q < end && (*q == '-' || *q == '+')) { eneg = *q == '-'; ++q; }
        if (q < end && *q >= '0' && *q <= '9') {
          int ev = 0;
          while (q < end && *q >= '0' && *q <= '9') { if (ev < 10000) ev = ev * 10 + (*q - '0'); ++q; }
          e10 += eneg ? -ev : ev;
          p = q;
        }
      }
      const bool ends = p >= end || *p == ' ' || *p == '\t' || *p == '\r' || *p == '\n';
      double v;
      if (digits && ends && fast && mant < (1ull << 53) && e10 >= -22 && e10 <= 22) {
        v = (double)mant;
        v = e10 < 0 ? v / p10[-e10] : v * p10[e10];
        if (neg) v = -v;
      } else {  // slow path: let strtod decide (also rejects garbage)
        const char *t = tok;
        while (t < end && !(*t == ' ' || *t == '\t' || *t == '\r' || *t == '\n')) ++t;
        std::string buf(tok, t);
        char *stop = nullptr;
        if (!gmr_bvh::float_token(buf.data(), buf.size())) return -1;  // (what strtod would take but Python's float() does not: hex, nan(...))
        v = strtod(buf.c_str(), &stop);
        if (buf.empty() || stop != buf.c_str() + buf.size()) return -1;
        p = t;
      }
      if (count >= max_out) return -1;
      out[count++] = v;
      ++cols;
    }
    if (p < end && *p == '\n') ++p;
    if (cols == 0) continue;  // blank line
    if (cols0 < 0) cols0 = cols;
    else if (cols != cols0) return -1;
    ++lines;
  }
  if (n_lines) *n_lines = lines;
  if (n_cols) *n_cols = cols0 < 0 ? 0 : cols0;
  return count;
}

int gmr_bvh_parse_motion_device(const char *text, int64_t text_bytes, int n_files, const int64_t *seg_begin, const int64_t *seg_end,
                                const int64_t *n_lines, int64_t n_cols, const int64_t *row_begin, double *rows_out, int32_t *status_out,
                                int64_t *n_tokens_out, int64_t *slow_out, int64_t max_slow, int64_t *n_slow, void *stream) {
  if (!text || !seg_begin || !seg_end || !n_lines || !row_begin || !rows_out || !status_out || !n_slow || n_files < 0 || n_cols < 1 ||
      max_slow < 0 || (max_slow > 0 && !slow_out))
    return GMR_EINVAL;
  *n_slow = 0;
  if (n_files == 0) return GMR_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  std::vector<gmr::TxtFile> files((size_t)n_files);
  int64_t nchunk = 0;
  for (int f = 0; f < n_files; ++f) {
    if (seg_begin[f] < 0 || seg_end[f] < seg_begin[f] || seg_end[f] > text_bytes || n_lines[f] < 0 || row_begin[f] < 0) return GMR_EINVAL;
    gmr::TxtFile &t = files[(size_t)f];
    t.seg_begin = seg_begin[f]; t.seg_end = seg_end[f]; t.chunk0 = nchunk;
    t.tok_limit = n_lines[f] * n_cols; t.out_base = row_begin[f] * n_cols; t.n_tokens = 0; t.status = 0; t.pad = 0;
    nchunk += std::max<int64_t>(1, (seg_end[f] - seg_begin[f] + gmr::kTxtChunk - 1) / gmr::kTxtChunk);  // (an empty block still owns a chunk: chunk -> file stays a search)
  }
  if (nchunk > 0x7fffffff) return GMR_EUNSUPPORTED;
  // one stream-ordered scratch block: file table | per-chunk counts | per-chunk bases | slow list | slow counter
  const size_t o_files = 0, o_counts = (sizeof(gmr::TxtFile) * (size_t)n_files + 15) & ~(size_t)15;
  const size_t o_bases = (o_counts + sizeof(int) * (size_t)nchunk + 15) & ~(size_t)15;
  const size_t o_slow = o_bases + sizeof(int64_t) * (size_t)nchunk;
  const size_t o_cnt = o_slow + sizeof(int64_t) * 3 * (size_t)max_slow;
  const size_t total = o_cnt + 16;
  char *scr = nullptr;
  if (hipMallocAsync((void **)&scr, total, st) != hipSuccess) return GMR_EDEVICE;
  int rc = GMR_OK;
  unsigned long long cnt = 0;
  do {
    if (hipMemcpyAsync(scr + o_files, files.data(), sizeof(gmr::TxtFile) * (size_t)n_files, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(scr + o_cnt, 0, 16, st) != hipSuccess) { rc = GMR_EDEVICE; break; }
    gmr::TxtFile *dfiles = reinterpret_cast<gmr::TxtFile *>(scr + o_files);
    int *counts = reinterpret_cast<int *>(scr + o_counts);
    int64_t *bases = reinterpret_cast<int64_t *>(scr + o_bases);
    const unsigned char *utext = reinterpret_cast<const unsigned char *>(text);
    hipLaunchKernelGGL(gmr::bvh_txt_count_kernel, dim3((unsigned)nchunk), dim3(64), 0, st, utext, dfiles, n_files, counts);
    hipLaunchKernelGGL(gmr::bvh_txt_scan_kernel, dim3((unsigned)n_files), dim3(64), 0, st, dfiles, counts, bases);
    hipLaunchKernelGGL(gmr::bvh_txt_parse_kernel, dim3((unsigned)nchunk), dim3(64), 0, st, utext, dfiles, n_files, bases, n_cols, rows_out,
                       reinterpret_cast<int64_t *>(scr + o_slow), max_slow, reinterpret_cast<unsigned long long *>(scr + o_cnt));
    if (hipGetLastError() != hipSuccess) { rc = GMR_EDEVICE; break; }
    if (hipMemcpyAsync(files.data(), dfiles, sizeof(gmr::TxtFile) * (size_t)n_files, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(&cnt, scr + o_cnt, sizeof(cnt), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) { rc = GMR_EDEVICE; break; }
    const int64_t keep = std::min<int64_t>((int64_t)cnt, max_slow);
    if (keep > 0 && (hipMemcpyAsync(slow_out, scr + o_slow, sizeof(int64_t) * 3 * (size_t)keep, hipMemcpyDeviceToHost, st) != hipSuccess ||
                     hipStreamSynchronize(st) != hipSuccess)) { rc = GMR_EDEVICE; break; }
    *n_slow = (int64_t)cnt;
    for (int f = 0; f < n_files; ++f) {
      const gmr::TxtFile &t = files[(size_t)f];
      status_out[f] = (t.status & 1) | (t.n_tokens < t.tok_limit ? 2 : 0);
      if (n_tokens_out) n_tokens_out[f] = t.n_tokens;
    }
  } while (0);
  (void)hipFreeAsync(scr, st);
  return rc;
}

static int bvh_fk_launch(const int32_t *parents, int n_joints, const int32_t *euler_order, const int32_t *extra_pos_src,
                         const int32_t *extra_rot_src, int n_extra, int layout, const double *pbase, const double *rbase,
                         const double *offsets, int64_t pstride, int64_t rstride, double ang_scale, int64_t n_frames, double scale,
                         const int32_t *out_cols, int n_out, double *pos_out, double *quat_out, void *stream) {
  if (!parents || !euler_order || !pbase || !rbase || !pos_out || !quat_out || n_frames < 0) return GMR_EINVAL;
  if (n_joints < 1 || n_joints > gmr::kBvhMaxJoints || n_extra < 0 || n_extra > gmr::kBvhMaxExtra) return GMR_EUNSUPPORTED;
  if (n_extra > 0 && (!extra_pos_src || !extra_rot_src)) return GMR_EINVAL;
  gmr::BvhSkeleton sk{};
  sk.n_joints = n_joints; sk.n_extra = n_extra; sk.layout = layout;
  for (int i = 0; i < 3; ++i) {
    if (euler_order[i] < 0 || euler_order[i] > 2) return GMR_EINVAL;
    sk.order[i] = euler_order[i];
  }
  if (parents[0] != -1) return GMR_EINVAL;
  for (int j = 0; j < n_joints; ++j) {
    if (j > 0 && (parents[j] < 0 || parents[j] >= j)) return GMR_EINVAL;  // hierarchy order
    sk.parent[j] = (short)parents[j];
  }
  for (int k = 0; k < n_extra; ++k) {
    if (extra_pos_src[k] < 0 || extra_pos_src[k] >= n_joints || extra_rot_src[k] < 0 || extra_rot_src[k] >= n_joints) return GMR_EINVAL;
    sk.extra_pos_src[k] = (short)extra_pos_src[k]; sk.extra_rot_src[k] = (short)extra_rot_src[k];
  }
  const int nb = n_joints + n_extra;
  if (out_cols) {  /* out_cols[c] = entry (joint, or n_joints + extra) emitted as column c */
    if (n_out < 1 || n_out > nb) return GMR_EINVAL;
    for (int j = 0; j < n_joints; ++j) sk.out_col[j] = -1;
    for (int k = 0; k < n_extra; ++k) sk.extra_col[k] = -1;
    for (int c = 0; c < n_out; ++c) {
      const int e = out_cols[c];
      if (e < 0 || e >= nb) return GMR_EINVAL;
      short &slot = e < n_joints ? sk.out_col[e] : sk.extra_col[e - n_joints];
      if (slot >= 0) return GMR_EINVAL;
      slot = (short)c;
    }
    sk.n_out = n_out;
  } else {
    for (int j = 0; j < n_joints; ++j) sk.out_col[j] = (short)j;
    for (int k = 0; k < n_extra; ++k) sk.extra_col[k] = (short)(n_joints + k);
    sk.n_out = nb;
  }
  if (n_frames == 0) return GMR_OK;
  const gmr::ChainGeom geo = gmr::chain_geom(n_joints);
  const int chunk = adapter_chunk(n_frames, geo.groups);
  const int64_t nblk = (n_frames + chunk - 1) / chunk;
  if (nblk > 0x7fffffff) return GMR_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int K = geo.jp <= 64 ? 1 : geo.jp / 64;
#define GMR_BVH_LAUNCH(KK, SS)                                                                                                              \
  hipLaunchKernelGGL((gmr::bvh_fk_kernel<KK, SS>), dim3((unsigned)nblk), dim3(64), lds_bytes, st, sk, pbase, rbase, offsets, (int)pstride, (int)rstride, ang_scale, \
                     n_frames, chunk, scale, pos_out, quat_out)
  const bool s9 = layout == gmr::BVH_ROWS9;
  const int per_frame = (int)(pbase != rbase ? pstride + rstride : pstride);
  const size_t lds_bytes = 2 * (size_t)gmr::bvh_batch(per_frame, geo.groups).doubles * sizeof(double);  // two stage buffers
  if (K == 1) { if (s9) GMR_BVH_LAUNCH(1, true); else GMR_BVH_LAUNCH(1, false); }
  else if (K == 2) { if (s9) GMR_BVH_LAUNCH(2, true); else GMR_BVH_LAUNCH(2, false); }
  else { if (s9) GMR_BVH_LAUNCH(3, true); else GMR_BVH_LAUNCH(3, false); }
#undef GMR_BVH_LAUNCH
  return hipGetLastError() == hipSuccess ? GMR_OK : GMR_EDEVICE;
}

int gmr_bvh_fk(const int32_t *parents, int n_joints, const int32_t *euler_order, const int32_t *extra_pos_src,
               const int32_t *extra_rot_src, int n_extra, const double *local_pos, const double *euler_rad, int64_t n_frames,
               double scale, double *pos_out, double *quat_out, void *stream) {
  return bvh_fk_launch(parents, n_joints, euler_order, extra_pos_src, extra_rot_src, n_extra, gmr::BVH_SPLIT, local_pos, euler_rad, nullptr,
                       3 * (int64_t)n_joints, 3 * (int64_t)n_joints, 1.0, n_frames, scale, nullptr, 0, pos_out, quat_out, stream);
}

int gmr_bvh_fk_rows(const int32_t *parents, int n_joints, const int32_t *euler_order, const int32_t *extra_pos_src,
                    const int32_t *extra_rot_src, int n_extra, int channels, const double *offsets, const double *rows, int64_t n_cols,
                    int64_t n_frames, double scale, const int32_t *out_cols, int n_out, double *pos_out, double *quat_out, void *stream) {
  if (!offsets || n_joints < 1) return GMR_EINVAL;
  int64_t want;
  if (channels == 3) want = 3 + 3 * (int64_t)n_joints;
  else if (channels == 6) want = 6 * (int64_t)n_joints;
  else if (channels == 9) want = 3 + 9 * (int64_t)(n_joints - 1);
  else return GMR_EUNSUPPORTED;
  if (n_cols != want) return GMR_EINVAL;
  return bvh_fk_launch(parents, n_joints, euler_order, extra_pos_src, extra_rot_src, n_extra, channels, rows, rows, offsets, n_cols, n_cols,
                       3.14159265358979323846 / 180.0, n_frames, scale, out_cols, n_out, pos_out, quat_out, stream);
}

#ifdef GMR_IK_STAMPS
/* diagnostic builds only: read and clear the per-phase cycle sums */
int gmr_debug_read_stamps(gmr_model *m, unsigned long long *out16) {
  if (!m || !m->dbg) return GMR_EINVAL;
  HIP_TRY(m, hipDeviceSynchronize());
  HIP_TRY(m, hipMemcpy(out16, m->dbg, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  HIP_TRY(m, hipMemset(m->dbg, 0, 16 * sizeof(unsigned long long)));
  return GMR_OK;
}
#endif

}  // extern "C"

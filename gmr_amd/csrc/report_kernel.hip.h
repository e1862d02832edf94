// report_kernel.hip.h -- the per-clip retarget quality report: solved qpos and the human key-points in, a few hundred bytes
// per clip out, for several models in one grid.
//
// What the reference's workflow gathers by hand -- error1() / error2() per frame (motion_retarget.py:188-200), the pelvis /
// hand position errors of its fork tooling, mink.check_limits' joints at their limits, the curated hard-motion lists -- as
// one fused pass: qpos and key-points are read once, nothing per frame is written.
//
// Pass 1 (clip_report_kernel): one wavefront per *segment*, a run of at most `segment` consecutive frames of one clip (never
// across a clip boundary), found through the members' segment bases and the clip's own prefix of segments.  The wavefront walks
// its frames in order with eval_kernel's device functions: q into LDS, fk_phase<false>, the target preparation of eval_kernel
// (offset_to_ground and a per-clip height scale included), task_residual per table.  Running statistics stay in registers:
//   lane = task (per table)   position / rotation error of the task: max and sum
//   lane = hinge (+64 k)      frames near the lower / upper limit, largest step between consecutive frames
//   wave-uniform              stage errors (max, sum), root step and turn, solves, non-finite frames
// The previous frame's q stays in LDS (two buffers that swap roles); a segment that does not start its clip loads frame a-1 as
// its "previous", so the step across a segment boundary is counted exactly once, by the later segment.  A frame whose qpos or
// consumed key-points hold a non-finite value is counted and otherwise skipped, and so are the steps into and out of it.
// Each segment writes one row of 8-byte words (doubles, counts as int64) to stream-ordered scratch.
//
// Pass 2 (clip_report_merge_kernel): one workgroup per clip folds the clip's rows in segment order, one lane per word, and
// writes the typed outputs.  No floating-point atomics anywhere: a report is bit-reproducible for a given segment length, and
// the maxima and counts are the same for every segment length.  A clip without frames has no rows and reports zeros.
//
// Segment length (GMR_CLIP_REPORT_SEGMENT = 32): measured, not derived (tools/clip_report_bench.py, profiles/clip_report_bench.json;
// unitree_g1, 2048 clips x 300 frames, the native call on preallocated outputs, medians of 10 alternated rounds): 1 frame per
// wavefront 2.97 ms, 4: 2.02, 8: 1.90, 16: 1.84, 32: 1.94, 64: 1.99, 128: 2.24, 300 (one wavefront per clip): 2.34.  Short
// segments pay the per-wavefront set-up (entry and clip look-up, hinge limits, the previous frame) per frame and write a row of
// 9 + 4 ntask + 3 nhinge words (unitree_g1: 1.6 KB) per frame; long ones leave the tail of the grid to a few wavefronts.  The
// curve is flat from 8 to 64 (within 8 %); 32 is 5 % off its best point at this shape, writes half the rows of 16 (55 bytes per
// frame) and still cuts a 10 s clip at 30 fps into ten wavefronts.  Not everything is paid once per segment: fk_phase<false>
// re-reads the body constants from the (L2-resident) model every frame, as in eval_kernel.  LDS is no limit (the eval layout plus
// one more q: ~3.5 KB per wavefront for G1); registers are: the accumulators of both tables, the frame's key-points and
// task_residual's working set want 178 VGPRs; the launch bounds ask for 3 wavefronts per SIMD (168 registers, no scratch -- at
// 4 per SIMD, 128 registers, 60 of them spill).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ik_kernel.hip.h"
#include "member_launch.hip.h"

namespace gmr {

constexpr int kReportHingeRounds = (GMR_MAX_BODIES + 63) / 64;  // hinges per lane: a model has at most GMR_MAX_BODIES - 1
constexpr int kReportHead = 9;  // words of a row before the task block
constexpr int kReportMergeThreads = 64;

// Words of a segment row: [err_max 2 | err_sum 2 | root_step | root_turn | nonfinite | solves_max | solves_sum |
//   task_pos_max nt | task_pos_sum nt | task_rot_max nt | task_rot_sum nt | dof_step_max nh | near_lo nh | near_hi nh]
__host__ __device__ inline int report_row_words(int nt, int nh) { return kReportHead + 4 * nt + 3 * nh; }

// One member's arguments of a launch, read through the constant address space.
struct ReportEntry {
  const DevModel *m;  // the evaluation model (full body tree)
  LdsLayout lay;      // its eval layout; the second q buffer follows at lay.total_doubles
  const double *qpos;
  const void *hpos, *hquat;  // NULL: no key-points, no error fields
  const int *slot_col;
  const double *hscale;  // [n_seq] or NULL
  const int *iters;      // [n] or NULL
  const int64_t *offs;   // device [n_seq + 1]
  const int *clip_seg;   // device [n_seq + 1]: segments of the clips before clip s
  const double *hlo, *hhi;  // device [nh]: hinge limits, -inf / +inf for an unlimited hinge
  unsigned long long *rows;  // [segments of this member][row words]
  double *err_max, *err_sum, *task_pos_max, *task_pos_sum, *task_rot_max, *task_rot_sum, *dof_step_max, *root_step_max, *root_turn_max;
  int *near_lo, *near_hi, *solves_max, *nonfinite;
  long long *solves_sum;
  double limit_eps;
  int64_t seg_base;   // first pass-1 workgroup of this member
  int64_t clip_base;  // first pass-2 workgroup of this member
  int n_seq, in_f64, n_cols, offset_to_ground, segment, nh, nt, pad;
};

__device__ __forceinline__ bool report_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }  // false for NaN and inf

__global__ void __launch_bounds__(64, 3) clip_report_kernel(const ReportEntry *__restrict__ entries, int n_entries) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int ei = launch_member<ReportEntry, &ReportEntry::seg_base>(entries, n_entries, (int64_t)blockIdx.x);
  const ReportEntry *ep = entries + ei;
  DevModelG &m = *(DevModelG *)motion_const(&ep->m);
  const int o_q = motion_const(&ep->lay.q), o_tp = motion_const(&ep->lay.tp), o_tq = motion_const(&ep->lay.tq);
  const int o_xpos = motion_const(&ep->lay.xpos), o_xquat = motion_const(&ep->lay.xquat), o_q2 = motion_const(&ep->lay.total_doubles);
  double *xpos = lds + o_xpos, *xquat = lds + o_xquat, *tp = lds + o_tp, *tq = lds + o_tq;
  const double *__restrict__ qpos = motion_const(&ep->qpos);
  const void *hpos = motion_const(&ep->hpos), *hquat = motion_const(&ep->hquat);
  const double *hscale = motion_const(&ep->hscale);
  const int *iters = motion_const(&ep->iters);
  const int64_t *offs = motion_const(&ep->offs);
  const int *clip_seg = motion_const(&ep->clip_seg);
  const int n_seq = motion_const(&ep->n_seq), in_f64 = motion_const(&ep->in_f64), n_cols = motion_const(&ep->n_cols);
  const int segment = motion_const(&ep->segment), nh = motion_const(&ep->nh), nt = motion_const(&ep->nt);
  const int offset_to_ground = motion_const(&ep->offset_to_ground);
  const double limit_eps = motion_const(&ep->limit_eps);
  const int nq = m.nq, nbody = m.nbody, nslot = m.nslot, root_slot = m.root_slot, planar = m.root_planar;
  const bool have_kp = hpos != nullptr;
  // ---- this wavefront's segment: the last clip whose prefix of segments is <= the member-local index (wave-uniform)
  const int sl = (int)((int64_t)blockIdx.x - motion_const(&ep->seg_base));
  int s = 0;
  {
    int hi = n_seq;
    while (hi - s > 1) {
      const int mid = (s + hi) >> 1;
      if (motion_const(clip_seg + mid) <= sl) s = mid; else hi = mid;
    }
  }
  const int64_t a = motion_const(offs + s), b = motion_const(offs + s + 1);
  const int64_t fa = a + (int64_t)(sl - motion_const(clip_seg + s)) * segment;
  const int64_t fb = fa + segment < b ? fa + segment : b;
  const double hs = hscale ? hscale[s] : 1.0;
  // ---- per-lane constants: slot columns, hinge limits
  const bool is_slot = lane < nslot;
  int s_col = 0, root_col = 0;
  if (have_kp) {
    const int *slot_col = motion_const(&ep->slot_col);
    s_col = slot_col[is_slot ? lane : 0];
    root_col = slot_col[root_slot];
  }
  double lo[kReportHingeRounds], hi_[kReportHingeRounds], step_max[kReportHingeRounds];
  long long n_lo[kReportHingeRounds], n_hi[kReportHingeRounds];
  {
    const double *hlo = motion_const(&ep->hlo), *hhi = motion_const(&ep->hhi);
#pragma unroll
    for (int r = 0; r < kReportHingeRounds; ++r) {
      const int j = lane + 64 * r;
      lo[r] = j < nh ? hlo[j] : -INFINITY;
      hi_[r] = j < nh ? hhi[j] : INFINITY;
      step_max[r] = 0.0; n_lo[r] = 0; n_hi[r] = 0;
    }
  }
  double pos_max[2] = {0, 0}, pos_sum[2] = {0, 0}, rot_max[2] = {0, 0}, rot_sum[2] = {0, 0};
  double err_max[2] = {0, 0}, err_sum[2] = {0, 0}, root_step = 0.0, root_turn = 0.0;
  long long nonfinite = 0, solves_max = 0, solves_sum = 0;

  // Frame f's q into `dst`; key-points of the frame into registers.  Returns whether everything consumed is finite (wave-uniform).
  double hp[3], hq[4], rp[3];
  auto load_frame = [&](int64_t f, double *dst) -> bool {
    bool ok = true;
    for (int i = lane; i < nq; i += 64) {
      const double v = qpos[(size_t)f * nq + i];
      dst[i] = v;
      ok = ok && report_finite(v);
    }
    hp[0] = hp[1] = hp[2] = 0.0; rp[0] = rp[1] = rp[2] = 0.0;
    hq[0] = 1.0; hq[1] = hq[2] = hq[3] = 0.0;
    if (have_kp) {
      const long long base = f * n_cols;
      if (in_f64) {
        const double *P = (const double *)hpos, *Q = (const double *)hquat;
        for (int i = 0; i < 3; i++) { rp[i] = P[(base + root_col) * 3 + i]; hp[i] = P[(base + s_col) * 3 + i]; }
        for (int i = 0; i < 4; i++) hq[i] = Q[(base + s_col) * 4 + i];
      } else {
        const float *P = (const float *)hpos, *Q = (const float *)hquat;
        for (int i = 0; i < 3; i++) { rp[i] = (double)P[(base + root_col) * 3 + i]; hp[i] = (double)P[(base + s_col) * 3 + i]; }
        for (int i = 0; i < 4; i++) hq[i] = (double)Q[(base + s_col) * 4 + i];
      }
      for (int i = 0; i < 3; i++) ok = ok && report_finite(rp[i]) && report_finite(hp[i]);
      for (int i = 0; i < 4; i++) ok = ok && report_finite(hq[i]);
    }
    return __all(ok) != 0;
  };

  double *qc = lds + o_q, *qp = lds + o_q2;  // current / previous frame
  bool prev_ok = false;
  if (fa > a) prev_ok = load_frame(fa - 1, qp);
  for (int64_t f = fa; f < fb; ++f) {
    __syncthreads();  // the previous iteration's readers of qc / qp are done
    const bool ok = load_frame(f, qc);
    __syncthreads();
    if (!ok) {
      ++nonfinite;
      prev_ok = false;
      continue;
    }
    if (iters) {
      const long long it = iters[f] & 0x3FFFFFFF;  // (bits 30 and 31 of iters_out are flags, gmr_amd.h)
      solves_max = it > solves_max ? it : solves_max;
      solves_sum += it;
    }
    // ---- joints: lane = hinge
#pragma unroll
    for (int r = 0; r < kReportHingeRounds; ++r) {
      const int j = lane + 64 * r;
      if (j < nh) {
        const double th = qc[7 + j];
        if (th - lo[r] <= limit_eps) ++n_lo[r];
        if (hi_[r] - th <= limit_eps) ++n_hi[r];
        if (prev_ok) step_max[r] = fmax(step_max[r], fabs(th - qp[7 + j]));
      }
    }
    // ---- root step and turn (every lane computes the same values)
    if (prev_ok) {
#pragma clang fp contract(off)  // plain differences, squares and sums in this order: what float64 numpy gives
      const double dx = qc[0] - qp[0], dy = qc[1] - qp[1], dz = qc[2] - qp[2];
      const double d2 = planar ? dx * dx + dy * dy : dx * dx + dy * dy + dz * dz;
      root_step = fmax(root_step, __builtin_sqrt(d2));
      double w, n;
      if (planar) {  // heading 2 atan2(z, w) of each: the wrapped difference, sign-blind
        w = qp[3] * qc[3] + qp[6] * qc[6];
        n = fabs(qp[3] * qc[6] - qp[6] * qc[3]);
      } else {  // conj(q_prev) (x) q_cur; a common scale of the two cancels in the atan2
        const double pc[4] = {qp[3], -qp[4], -qp[5], -qp[6]}, cq[4] = {qc[3], qc[4], qc[5], qc[6]};
        double qr[4];
        qmul(pc, cq, qr);
        w = qr[0];
        n = __builtin_sqrt(qr[1] * qr[1] + qr[2] * qr[2] + qr[3] * qr[3]);
      }
      root_turn = fmax(root_turn, 2.0 * atan2(n, fabs(w)));
    }
    prev_ok = true;
    if (have_kp) {
      fk_phase<false>(m, nullptr, nbody, m.fkrounds, lane, qc, xpos, xquat);
      {  // target preparation, as in eval_kernel
        double pz = INFINITY, p[3] = {0, 0, 0}, qo[4] = {1, 0, 0, 0}, R[9], g[3];
        if (is_slot) {
          const double s_scale = hs * m.sscale[lane], root_scale = hs * m.sscale[root_slot];
          const double s_poff[3] = {m.spoff[3 * lane], m.spoff[3 * lane + 1], m.spoff[3 * lane + 2]};
          const double s_roff[4] = {m.sroff[4 * lane], m.sroff[4 * lane + 1], m.sroff[4 * lane + 2], m.sroff[4 * lane + 3]};
          for (int i = 0; i < 3; i++) p[i] = (lane == root_slot) ? root_scale * rp[i] : (hp[i] - rp[i]) * s_scale + root_scale * rp[i];
          qnormalize(hq);
          qmul(hq, s_roff, qo);
          qrenorm(qo);
          q2mat(qo, R);
          mv(R, s_poff, g);
          for (int i = 0; i < 3; i++) p[i] += g[i];
          if (m.sfoot[lane]) pz = p[2];
        }
        if (offset_to_ground) p[2] = p[2] - wave_min(pz) + 0.1;
        if (is_slot) {
          for (int i = 0; i < 3; i++) tp[3 * lane + i] = p[i];
          for (int i = 0; i < 4; i++) tq[4 * lane + i] = qo[i];
        }
      }
      __syncthreads();
#pragma unroll
      for (int tab = 0; tab < 2; ++tab) {
        if (m.use_table[tab]) {
          const bool is_task = lane < m.ntask[tab];
          const int trow = tab * GMR_MAX_TASKS + (is_task ? lane : 0);
          const int body = m.tbody[trow], slot = m.tslot[trow];
          double e[6], kap, bet;
          const double err = fast_sqrt(wave_sum(is_task ? task_residual(body, slot, xpos, xquat, tp, tq, e, kap, bet) : 0.0));
          err_max[tab] = fmax(err_max[tab], err);
          err_sum[tab] += err;
          if (is_task) {
            const double d0 = tp[3 * slot] - xpos[3 * body], d1 = tp[3 * slot + 1] - xpos[3 * body + 1], d2 = tp[3 * slot + 2] - xpos[3 * body + 2];
            const double dp = __builtin_sqrt(d0 * d0 + d1 * d1 + d2 * d2), dr = __builtin_sqrt(e[3] * e[3] + e[4] * e[4] + e[5] * e[5]);
            pos_max[tab] = fmax(pos_max[tab], dp); pos_sum[tab] += dp;
            rot_max[tab] = fmax(rot_max[tab], dr); rot_sum[tab] += dr;
          }
        }
      }
    }
    double *t = qc; qc = qp; qp = t;  // this frame is the next one's "previous"
  }
  // ---- the segment's row
  unsigned long long *row = motion_const(&ep->rows) + (size_t)sl * report_row_words(nt, nh);
  auto put_d = [&](int w, double v) { row[w] = (unsigned long long)__double_as_longlong(v); };
  if (lane == 0) {
    put_d(0, err_max[0]); put_d(1, err_max[1]); put_d(2, err_sum[0]); put_d(3, err_sum[1]);
    put_d(4, root_step); put_d(5, root_turn);
    row[6] = (unsigned long long)nonfinite; row[7] = (unsigned long long)solves_max; row[8] = (unsigned long long)solves_sum;
  }
#pragma unroll
  for (int tab = 0; tab < 2; ++tab) {
    const int nt_tab = m.ntask[tab];
    if (lane < nt_tab) {
      const int w = kReportHead + (tab ? m.ntask[0] : 0) + lane;
      put_d(w, pos_max[tab]); put_d(w + nt, pos_sum[tab]); put_d(w + 2 * nt, rot_max[tab]); put_d(w + 3 * nt, rot_sum[tab]);
    }
  }
#pragma unroll
  for (int r = 0; r < kReportHingeRounds; ++r) {
    const int j = lane + 64 * r;
    if (j < nh) {
      const int w = kReportHead + 4 * nt + j;
      put_d(w, step_max[r]);
      row[w + nh] = (unsigned long long)n_lo[r];
      row[w + 2 * nh] = (unsigned long long)n_hi[r];
    }
  }
}

// One workgroup per clip: word w of the clip's rows folded in segment order by lane w (+ 64 k), then stored in its output's type.
__global__ void __launch_bounds__(kReportMergeThreads) clip_report_merge_kernel(const ReportEntry *__restrict__ entries, int n_entries) {
  const int ei = launch_member<ReportEntry, &ReportEntry::clip_base>(entries, n_entries, (int64_t)blockIdx.x);
  const ReportEntry *ep = entries + ei;
  const int s = (int)((int64_t)blockIdx.x - motion_const(&ep->clip_base));
  const int nh = motion_const(&ep->nh), nt = motion_const(&ep->nt), W = report_row_words(nt, nh);
  const int *clip_seg = motion_const(&ep->clip_seg);
  const int k0 = motion_const(clip_seg + s), k1 = motion_const(clip_seg + s + 1);
  const unsigned long long *rows = motion_const(&ep->rows);
  const bool want_solves = motion_const(&ep->iters) != nullptr;
  for (int w = threadIdx.x; w < W; w += kReportMergeThreads) {
    // kind of the word: 0 max of doubles, 1 sum of doubles, 2 max of counts, 3 sum of counts
    int kind, idx = 0;
    void *out = nullptr;
    if (w < 2) { kind = 0; out = motion_const(&ep->err_max); idx = w; }
    else if (w < 4) { kind = 1; out = motion_const(&ep->err_sum); idx = w - 2; }
    else if (w == 4) { kind = 0; out = motion_const(&ep->root_step_max); }
    else if (w == 5) { kind = 0; out = motion_const(&ep->root_turn_max); }
    else if (w == 6) { kind = 3; out = motion_const(&ep->nonfinite); }
    else if (w == 7) { kind = 2; out = want_solves ? motion_const(&ep->solves_max) : nullptr; }
    else if (w == 8) { kind = 3; out = want_solves ? (void *)motion_const(&ep->solves_sum) : nullptr; }
    else if (w < kReportHead + 4 * nt) {
      const int k = (w - kReportHead) / nt;
      idx = (w - kReportHead) - k * nt;
      kind = k & 1;
      out = k == 0 ? motion_const(&ep->task_pos_max) : k == 1 ? motion_const(&ep->task_pos_sum)
          : k == 2 ? motion_const(&ep->task_rot_max) : motion_const(&ep->task_rot_sum);
    } else {
      const int k = (w - kReportHead - 4 * nt) / nh;
      idx = (w - kReportHead - 4 * nt) - k * nh;
      kind = k == 0 ? 0 : 3;
      out = k == 0 ? (void *)motion_const(&ep->dof_step_max) : k == 1 ? (void *)motion_const(&ep->near_lo) : (void *)motion_const(&ep->near_hi);
    }
    if (!out) continue;
    double d = 0.0;
    long long c = 0;
    for (int k = k0; k < k1; ++k) {
      const unsigned long long v = rows[(size_t)k * W + w];
      if (kind == 0) d = fmax(d, __longlong_as_double((long long)v));
      else if (kind == 1) d += __longlong_as_double((long long)v);
      else if (kind == 2) c = (long long)v > c ? (long long)v : c;
      else c += (long long)v;
    }
    const int per = w < kReportHead ? (w < 4 ? 2 : 1) : (w < kReportHead + 4 * nt ? nt : nh);
    const size_t at = (size_t)s * per + idx;
    if (kind < 2) static_cast<double *>(out)[at] = d;
    else if (w == 8) static_cast<long long *>(out)[at] = c;
    else static_cast<int *>(out)[at] = (int)c;
  }
}

}  // namespace gmr

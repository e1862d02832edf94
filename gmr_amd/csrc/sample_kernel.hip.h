// sample_kernel.hip.h -- the motion library's random access: (clip id, time) queries against stored qpos, one launch
// (gmr_motion_sample; the definition is the contract in include/gmr_amd.h).
//
// What a tracking / AMP trainer asks at every simulation step -- for environment e the reference state of clip id[e] at time t[e],
// and usually at K future times -- answered from the qpos the retarget wrote (288 B per G1 frame), not from a pre-exported track
// (2.7 KB per frame, one rate): per query the tracking export's lerp / shortest-arc slerp of two source rows, the generalized
// velocity as the lerp of the two rows' central differences (continuous in t), the FK chain of fk_kernel.hip.h on the float32
// casts (bit for bit gmr_fk), and the bodies' twists carried down the same chain.  track_lerp / track_slerp / track_ang_vel are
// the tracking export's own functions (track_kernel.hip.h), shared and not copied.
//
// One wavefront per 64 consecutive queries, lane = query; motion_track_kernel's four stages without its halo lanes:
//
//   1  per lane: the query's clip and time -> four source rows r0 .. r3 = i0-1, i0, i1, i1+1 clamped to the clip, the weight a,
//      the steps h0, h1 of the two stencils, and the flags (valid; i1 > i0) -> the plan arrays in LDS.  An invalid query (and a
//      dead lane of the last wavefront) gets no rows: nothing of qpos is read for it
//   2  per element: one (query, column) per lane and load group of four rows, kSampleBatch groups in flight (consecutive lanes read
//      consecutive doubles of a row); positions and joints are lerped into the pose row image, their two central differences into
//      the velocity row image, the four quaternions parked.  Invalid queries get NaN rows
//   3  per lane: slerp and the two angular stencils, then the FK chain with the twist beside the pose (branch slots of 13 floats);
//      every body that is asked for is stored as it is produced, 12 / 16 bytes per lane and array -- there is no body image in
//      LDS (the export needs one for its differences; here the full images would be 64 x nbody x 52 B = 126 KB for G1)
//   4  per element: the six generalized outputs of the 64 queries leave linearly (track_emit), as float64 or rounded once to float32
//
// The arguments travel as the kernel argument (the kernarg segment: scalar loads), so a call enqueues this kernel and nothing else.
// The body-id list is turned into per-body chains of output columns in LDS once per wavefront (first[body] -> column -> next
// column), read back wave-uniformly: the walk costs nbody + n_sel steps where a scan of the list per body would cost their product.
// LDS per wavefront (sample_lds): pose rows [64][nq | 1] f64 | velocity rows [64][nq | 1] f64 | parked quaternions [64][17] f64 |
// plan: src [4][64] i64, a, h0, h1 [64] f64, flags [64] i32 | branch slots [nslots][13][64] f32 | first [nbody], next [n_sel] i32.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "track_kernel.hip.h"

namespace gmr {

constexpr int kSampleBatch = 4;    // (query, column) elements in flight per lane in stage 2: 4 x 4 rows = 16 loads
constexpr int kSampleQuatPitch = 17;  // doubles per lane of the quaternion park (odd: conflict-free)
constexpr int kSampleSlot = 13;    // floats per branch slot: position 3, rotation 4, linear 3 and angular 3 velocity

struct SampleArgs {
  const FkBody *body;
  const int *save_slot;
  int nbody, ndof, nslots, n_seq;
  const double *qpos;
  int64_t n_frames;
  const int64_t *seq_offsets;
  const double *fps;
  const int64_t *ids;
  const void *times;
  int64_t n_queries;
  const int *body_ids;
  int n_sel, k_per_id, time_f64, out_f64;
  void *root_pos, *root_rot, *joint_pos, *root_lin_vel, *root_ang_vel, *joint_vel;
  float *body_pos, *body_quat, *body_lin_vel, *body_ang_vel;
};

// Byte offsets of the LDS arrays of one wavefront, and their sum (host and device agree on this layout).
struct SampleLds { int rows, vels, quats, src, a, h0, h1, flags, slots, first; int64_t next, bytes; };  // (all but n_sel's share is < 160 KB)
__host__ __device__ inline SampleLds sample_lds(int nbody, int ndof, int nslots, int n_sel) {
  SampleLds l{};
  int at = 0;
  l.rows = at;  at += motion_qpitch(ndof + 7) * kFkWave * 8;
  l.vels = at;  at += motion_qpitch(ndof + 7) * kFkWave * 8;
  l.quats = at; at += kSampleQuatPitch * kFkWave * 8;
  l.src = at;   at += 4 * kFkWave * 8;
  l.a = at;     at += kFkWave * 8;
  l.h0 = at;    at += kFkWave * 8;
  l.h1 = at;    at += kFkWave * 8;
  l.flags = at; at += kFkWave * 4;
  l.slots = at; at += (nslots > 1 ? nslots : 1) * kSampleSlot * kFkWave * 4;
  l.first = at; at += nbody * 4;
  l.next = at;
  l.bytes = ((int64_t)at + (int64_t)n_sel * 4 + 15) & ~(int64_t)15;
  return l;
}

constexpr int kSampleValid = 1, kSampleStep = 2;  // plan flags: the query reads rows; i1 > i0

__global__ void __launch_bounds__(kFkWave) motion_sample_kernel(const SampleArgs A) {
#pragma clang fp contract(off)  // gmr_fk's arithmetic exactly; the float64 part as the contract writes it
  extern __shared__ __attribute__((aligned(16))) unsigned char sample_smem[];
  const int lane = threadIdx.x;
  FkTree t{};  // the fields the chain reads (fk_body, fk_const)
  t.body = A.body;
  t.save_slot = A.save_slot;
  t.nbody = A.nbody;
  t.ndof = A.ndof;
  t.nslots = A.nslots;
  const double *__restrict__ qpos = A.qpos;
  const int nbody = A.nbody, ndof = A.ndof, nq = ndof + 7, qp = motion_qpitch(nq);
  const int *const body_ids = A.body_ids;
  const int n_sel = body_ids ? A.n_sel : 0, ncol = body_ids ? A.n_sel : nbody;  // ncol: body columns of one query in the outputs
  float *const o_bpos = A.body_pos, *const o_bquat = A.body_quat, *const o_blin = A.body_lin_vel, *const o_bang = A.body_ang_vel;
  const int want = (o_bpos ? 1 : 0) | (o_bquat ? 2 : 0) | (o_blin ? 4 : 0) | (o_bang ? 8 : 0);  // the body outputs asked for
  const bool want_fk = want != 0 && ncol > 0;
  const SampleLds L = sample_lds(nbody, ndof, A.nslots, n_sel);
  double *rows = reinterpret_cast<double *>(sample_smem + L.rows);    // [64][qp]: x y z | qx qy qz qw | joints
  double *vels = reinterpret_cast<double *>(sample_smem + L.vels);    // [64][qp]: v | w, one spare | joint velocities
  double *quats = reinterpret_cast<double *>(sample_smem + L.quats);  // [64][17]: the quaternions (wxyz) of rows r0 .. r3
  int64_t *src = reinterpret_cast<int64_t *>(sample_smem + L.src);    // [4][64]: global source rows r0 .. r3
  double *wa = reinterpret_cast<double *>(sample_smem + L.a), *wh0 = reinterpret_cast<double *>(sample_smem + L.h0);
  double *wh1 = reinterpret_cast<double *>(sample_smem + L.h1);
  int *flags = reinterpret_cast<int *>(sample_smem + L.flags);
  float *slots = reinterpret_cast<float *>(sample_smem + L.slots);
  int *first = reinterpret_cast<int *>(sample_smem + L.first), *next = reinterpret_cast<int *>(sample_smem + L.next);
  const int64_t q = (int64_t)blockIdx.x * kFkWave + lane;  // this lane's query; the wavefront's rows 0 .. nfb-1 are its live ones
  const bool live = q < A.n_queries;
  const double nan = __builtin_nan("");
  // ---- 1: this lane's plan.  Dead lanes and invalid queries read no row of qpos; they take part in everything else
  double a = 0.0, h0 = 0.0, h1 = 0.0;
  int fl = 0;
  if (want_fk && body_ids)
    for (int j = lane; j < nbody; j += kFkWave) first[j] = -1;
  if (live) {
    const int64_t id = A.ids[A.k_per_id == 1 ? q : q / A.k_per_id];
    const double tq = A.time_f64 ? static_cast<const double *>(A.times)[q] : (double)static_cast<const float *>(A.times)[q];
    bool ok = id >= 0 && id < (int64_t)A.n_seq && fabs(tq) < __builtin_inf();  // (false for a NaN time)
    int64_t sb = 0, T = 0;
    double f = 1.0;
    if (ok) {
      sb = A.seq_offsets[id];
      T = A.seq_offsets[id + 1] - sb;
      f = A.fps[id];
      ok = T > 0 && sb >= 0 && T <= A.n_frames - sb;  // (a clip table that leaves qpos is not followed)
    }
    const double u = tq * f;
    ok = ok && u == u;  // (a NaN fps)
    if (ok) {
      int64_t i0;
      if (u <= 0.0) i0 = 0;
      else if (u >= (double)(T - 1)) i0 = T - 1;
      else i0 = (int64_t)floor(u);
      const int64_t i1 = i0 + 1 < T ? i0 + 1 : T - 1;
      a = (i1 > i0 && 0.0 < u) ? u - (double)i0 : 0.0;
      const int64_t km0 = i0 > 0 ? i0 - 1 : 0, kp1 = i1 + 1 < T ? i1 + 1 : T - 1;  // kp0 = i1; km1 = i0 when i1 > i0, else km0
      const int64_t km1 = i1 > 0 ? i1 - 1 : 0;
      const double dt = 1.0 / f;
      h0 = (double)(i1 - km0) * dt;
      h1 = (double)(kp1 - km1) * dt;
      fl = kSampleValid | (i1 > i0 ? kSampleStep : 0);
      src[0 * kFkWave + lane] = sb + km0;
      src[1 * kFkWave + lane] = sb + i0;
      src[2 * kFkWave + lane] = sb + i1;
      src[3 * kFkWave + lane] = sb + kp1;
    }
  }
  wa[lane] = a;
  wh0[lane] = h0;
  wh1[lane] = h1;
  flags[lane] = fl;
  __syncthreads();
  if (want_fk && body_ids)  // chains of output columns per body (any order within a chain: each column is stored once)
    for (int k = lane; k < n_sel; k += kFkWave) next[k] = atomicExch(&first[body_ids[k]], k);
  // ---- 2: the four source rows of all 64 queries, one (query, column) per lane and load group
  {
    const int n = kFkWave * nq;
    const float inv_nq = 1.0f / (float)nq;
    for (int base = 0; base < n; base += kSampleBatch * kFkWave) {
      double xa[kSampleBatch], xb[kSampleBatch], xc[kSampleBatch], xd[kSampleBatch];  // rows r0 .. r3 (separate arrays: registers)
#pragma unroll
      for (int b = 0; b < kSampleBatch; ++b) {
        const int i = base + b * kFkWave + lane;
        xa[b] = xb[b] = xc[b] = xd[b] = 0.0;
        if (i < n) {
          const int fr = motion_div(i, inv_nq), c = i - fr * nq;
          if (flags[fr] & kSampleValid) {
            xa[b] = qpos[src[0 * kFkWave + fr] * nq + c];
            xb[b] = qpos[src[1 * kFkWave + fr] * nq + c];
            xc[b] = qpos[src[2 * kFkWave + fr] * nq + c];
            xd[b] = qpos[src[3 * kFkWave + fr] * nq + c];
          }
        }
      }
#pragma unroll
      for (int b = 0; b < kSampleBatch; ++b) {
        const int i = base + b * kFkWave + lane;
        if (i < n) {
          const int fr = motion_div(i, inv_nq), c = i - fr * nq;
          const int ff = flags[fr];
          if (c >= 3 && c < 7) {
            double *qd = quats + fr * kSampleQuatPitch + c - 3;
            qd[0] = xa[b]; qd[4] = xb[b]; qd[8] = xc[b]; qd[12] = xd[b];
          } else if (!(ff & kSampleValid)) {
            rows[fr * qp + c] = nan;
            vels[fr * qp + c] = nan;
          } else {
            const double aa = wa[fr], hh0 = wh0[fr], hh1 = wh1[fr];
            const double xm = (ff & kSampleStep) ? xb[b] : xa[b];  // row km1: i0 when i1 > i0, else km0
            const double v0 = hh0 != 0.0 ? (xc[b] - xa[b]) / hh0 : 0.0;
            const double v1 = hh1 != 0.0 ? (xd[b] - xm) / hh1 : 0.0;
            rows[fr * qp + c] = track_lerp(xb[b], xc[b], aa);
            vels[fr * qp + c] = track_lerp(v0, v1, aa);
          }
        }
      }
    }
  }
  __syncthreads();
  // ---- 3: slerp and the two angular stencils (wxyz in, xyzw out), then the chain on the float32 casts of the query's row
  {
    double qr[4] = {nan, nan, nan, nan}, wr[3] = {nan, nan, nan};
    if (fl & kSampleValid) {
      double qa[4], qb[4], qc[4], qd[4], qm[4];  // rows r0 .. r3 as xyzw, and row km1: i0 when i1 > i0, else km0
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const double *qq = quats + lane * kSampleQuatPitch + ((i + 1) & 3);
        qa[i] = qq[0]; qb[i] = qq[4]; qc[i] = qq[8]; qd[i] = qq[12];
        qm[i] = (fl & kSampleStep) ? qb[i] : qa[i];
      }
      // a = 0 is a copy; so are two identical source rows (the tracking export's rule)
      if (a == 0.0 || (qb[0] == qc[0] && qb[1] == qc[1] && qb[2] == qc[2] && qb[3] == qc[3])) {
#pragma unroll
        for (int i = 0; i < 4; i++) qr[i] = qb[i];
      } else {
        track_slerp(qb, qc, a, qr);
      }
      double w0[3] = {0.0, 0.0, 0.0}, w1[3] = {0.0, 0.0, 0.0};
      if (h0 != 0.0) track_ang_vel(qc, qa, h0, w0);
      if (h1 != 0.0) track_ang_vel(qd, qm, h1, w1);
#pragma unroll
      for (int i = 0; i < 3; i++) wr[i] = track_lerp(w0[i], w1[i], a);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) rows[lane * qp + 3 + i] = qr[i];
#pragma unroll
    for (int i = 0; i < 3; i++) vels[lane * qp + 3 + i] = wr[i];
  }
  if (want_fk) {  // (wave-uniform) fk_kernel's chain, with the twist: cv / cw are the body's world linear / angular velocity
    struct F3 { float x, y, z; };     // 12 bytes, 4-byte aligned
    struct F4 { float x, y, z, w; };  // 16 bytes, 4-byte aligned
    const double *my = rows + lane * qp, *myv = vels + lane * qp;
    const bool good = (fl & kSampleValid) != 0;
    const float nanf = __builtin_nanf("");
    float cp[3], cr[4], cv[3], cw[3];
#pragma unroll
    for (int i = 0; i < 3; i++) { cp[i] = (float)my[i]; cv[i] = (float)myv[i]; cw[i] = (float)myv[3 + i]; }
#pragma unroll
    for (int i = 0; i < 4; i++) cr[i] = (float)my[3 + i];
    auto save = [&](int sv) {
      float *sl = slots + (size_t)sv * kSampleSlot * kFkWave + lane;
#pragma unroll
      for (int i = 0; i < 3; i++) { sl[i * kFkWave] = cp[i]; sl[(7 + i) * kFkWave] = cv[i]; sl[(10 + i) * kFkWave] = cw[i]; }
#pragma unroll
      for (int i = 0; i < 4; i++) sl[(3 + i) * kFkWave] = cr[i];
    };
    auto put = [&](int col) {  // the current body into output column `col` of this lane's query
      if (!live) return;
      const int64_t o = q * ncol + col;
      if (want & 1) *reinterpret_cast<F3 *>(o_bpos + o * 3) = good ? F3{cp[0], cp[1], cp[2]} : F3{nanf, nanf, nanf};
      if (want & 2) *reinterpret_cast<F4 *>(o_bquat + o * 4) = good ? F4{cr[0], cr[1], cr[2], cr[3]} : F4{nanf, nanf, nanf, nanf};
      if (want & 4) *reinterpret_cast<F3 *>(o_blin + o * 3) = good ? F3{cv[0], cv[1], cv[2]} : F3{nanf, nanf, nanf};
      if (want & 8) *reinterpret_cast<F3 *>(o_bang + o * 3) = good ? F3{cw[0], cw[1], cw[2]} : F3{nanf, nanf, nanf};
    };
    auto keep = [&](int j) {
      if (!body_ids) { put(j); return; }
      int k = __builtin_amdgcn_readfirstlane(first[j]);
      while (k >= 0) {
        put(k);
        k = __builtin_amdgcn_readfirstlane(next[k]);
      }
    };
    if (fk_const(t.save_slot, 0) >= 0) save(fk_const(t.save_slot, 0));
    keep(0);
    FkBody nxt = fk_body(t, nbody > 1 ? 1 : 0);
    for (int j = 1; j < nbody; ++j) {
      const FkBody rec = nxt;
      nxt = fk_body(t, j + 1 < nbody ? j + 1 : j);  // one body ahead
      float pp[3], pr[4], pv[3], pw[3];
      const int sidx = rec.src_slot;
      if (sidx < 0) {
#pragma unroll
        for (int i = 0; i < 3; i++) { pp[i] = cp[i]; pv[i] = cv[i]; pw[i] = cw[i]; }
#pragma unroll
        for (int i = 0; i < 4; i++) pr[i] = cr[i];
      } else {
        const float *sl = slots + (size_t)sidx * kSampleSlot * kFkWave + lane;
#pragma unroll
        for (int i = 0; i < 3; i++) { pp[i] = sl[i * kFkWave]; pv[i] = sl[(7 + i) * kFkWave]; pw[i] = sl[(10 + i) * kFkWave]; }
#pragma unroll
        for (int i = 0; i < 4; i++) pr[i] = sl[(3 + i) * kFkWave];
      }
      float jq[4] = {0.f, 0.f, 0.f, 1.f};
      if (rec.dofidx >= 0) fk_hinge_quat(rec.axis, (float)my[7 + rec.dofidx], jq);
      const float lt[3] = {rec.lpos[0], rec.lpos[1], rec.lpos[2]};
      const float lr[4] = {rec.lrot[0], rec.lrot[1], rec.lrot[2], rec.lrot[3]};
      float wt[3], tmp[4];
      fk_quat_rotate(pr, lt, wt);
#pragma unroll
      for (int i = 0; i < 3; i++) cp[i] = pp[i] + wt[i];
      fk_quat_mul(lr, jq, tmp);
      fk_quat_mul(pr, tmp, cr);
      // the twist (the contract's operand order): v = v_p + w_p x (x - x_p), w = w_p + (R axis) thetadot
      const float d[3] = {cp[0] - pp[0], cp[1] - pp[1], cp[2] - pp[2]};
      cv[0] = pv[0] + (pw[1] * d[2] - pw[2] * d[1]);
      cv[1] = pv[1] + (pw[2] * d[0] - pw[0] * d[2]);
      cv[2] = pv[2] + (pw[0] * d[1] - pw[1] * d[0]);
#pragma unroll
      for (int i = 0; i < 3; i++) cw[i] = pw[i];
      if (rec.dofidx >= 0) {
        const float ax[3] = {(float)rec.axis[0], (float)rec.axis[1], (float)rec.axis[2]};
        const float td = (float)myv[7 + rec.dofidx];
        float aw[3];
        fk_quat_rotate(cr, ax, aw);
#pragma unroll
        for (int i = 0; i < 3; i++) cw[i] = pw[i] + aw[i] * td;
      }
      keep(j);
      if (rec.save_slot >= 0) save(rec.save_slot);
    }
  }
  __syncthreads();
  // ---- 4: the generalized outputs of queries q0 .. q0 + nfb - 1
  // (the six pointers are read from the argument here, not at the kernel's entry: held in SGPRs across the chain they would not fit)
  const auto *late = (const SampleArgs __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr();
  const int out_f64 = late->out_f64;
  unsigned wg = blockIdx.x;
  asm volatile("" : "+s"(wg));  // (computed again here: carried from the entry, the 64-bit base is what no longer fits in SGPRs)
  const int64_t q0 = (int64_t)wg * kFkWave;
  const int64_t left = late->n_queries - q0;
  const int nout = (int)(left < kFkWave ? left : kFkWave);  // (nfb again)
  auto emit = [&](void *dst, int width, auto f) {  // dst [Q][width] of the output type
    if (!dst) return;
    if (out_f64) track_emit(static_cast<double *>(dst) + q0 * width, nout * width, lane, f);
    else track_emit(static_cast<float *>(dst) + q0 * width, nout * width, lane, [&](int i) { return (float)f(i); });
  };
  emit(late->root_pos, 3, [&](int i) { const int fr = motion_div(i, 1.0f / 3.0f); return rows[fr * qp + i - fr * 3]; });
  emit(late->root_rot, 4, [&](int i) { return rows[(i >> 2) * qp + 3 + (i & 3)]; });
  emit(late->root_lin_vel, 3, [&](int i) { const int fr = motion_div(i, 1.0f / 3.0f); return vels[fr * qp + i - fr * 3]; });
  emit(late->root_ang_vel, 3, [&](int i) { const int fr = motion_div(i, 1.0f / 3.0f); return vels[fr * qp + 3 + i - fr * 3]; });
  if (ndof > 0) {
    const float inv_ndof = 1.0f / (float)ndof;
    emit(late->joint_pos, ndof, [&](int i) { const int fr = motion_div(i, inv_ndof); return rows[fr * qp + 7 + i - fr * ndof]; });
    emit(late->joint_vel, ndof, [&](int i) { const int fr = motion_div(i, inv_ndof); return vels[fr * qp + 7 + i - fr * ndof]; });
  }
}

}  // namespace gmr

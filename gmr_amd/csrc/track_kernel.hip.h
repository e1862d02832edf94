// track_kernel.hip.h -- the tracking export: solved qpos in, resampled world body states and velocities out, for several models
// in one grid (gmr_motion_track / gmr_group_motion_track; the definition is the contract in include/gmr_amd.h).
//
// What a consumer of a retargeted dataset does before it trains a tracking policy -- resample every clip to the controller's
// rate, FK with the real root, differentiate -- as one launch: per output frame the lerp / shortest-arc slerp of two source
// rows (float64), the FK chain of fk_kernel.hip.h on the float32 casts of the result (bit for bit gmr_fk), and central
// differences of the resampled rows and of the float32 body poses.
//
// One wavefront per tile, lane = output frame.  A tile is kTrackTile = 62 consecutive output frames of one member (clips
// concatenated) plus one halo frame on each side, so every central difference finds both of its frames inside the wavefront.  A
// frame at the edge of its clip differences against itself on that side (one-sided difference; nothing crosses a clip), so a halo
// lane only matters when it lies in the clip of its neighbour; a halo that falls off the member repeats the member's edge frame.
// Lane l holds output frame g0 + l - 1 in LDS row (l + 63) & 63: the 62 central lanes own rows 0 .. 61, which makes the tile's
// part of every output one contiguous run that starts at the base of its LDS image.
//
//   1  per lane: clip (wave-uniform binary search for the tile's first frame, then forward per lane), source rows i0 / i1 and
//      weight a, neighbours km / kp and step h -> the plan arrays in LDS
//   2  per element: the two source rows of all 64 frames, one (frame, column) per lane and load pair, kMotionBatch pairs in flight
//      (consecutive lanes read consecutive doubles of a row, and consecutive rows where the ratio is <= 1); positions and joints
//      are lerped into the row image, the two quaternions parked
//   3  per lane: slerp, then the FK chain with the real root; positions and rotations go into the two tile images
//   4  per element: every output leaves linearly, 16 bytes per lane and store where the destination is 16-byte aligned; the
//      angular velocities of the bodies, one (frame, body) item per lane, leave as 12 contiguous bytes per lane
//
// Staging the tile's whole source span in LDS (as the epilogue stages its 64 rows) would bound the ratio fps_in / fps_out by the
// LDS left over; reading each frame's two rows with row-coalesced loads has no such limit and one code path, and the second read of
// a row shared by two output frames comes out of the cache.
// LDS per wavefront (track_lds): row image [64][nq | 1] f64 | parked quaternions [64][8] f64 | plan: src0, src1 i64, a, h f64,
// rowm, rowp i32, [64] each | position image [64][3 nbody] f32 | rotation image [64][4 nbody] f32 | branch slots [nslots][7][64] f32.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "member_launch.hip.h"
#include "motion_kernel.hip.h"

namespace gmr {

constexpr int kTrackTile = kFkWave - 2;  // output frames per wavefront (one halo lane on each side)

// One member's arguments of a launch, read by the kernel through the constant address space.
struct TrackEntry {
  FkTree fk;
  const double *qpos;
  const int64_t *seq_offsets, *out_offsets;  // device copies, [n_seq + 1]
  const double *ratio;                       // device copy, [n_seq]
  double *root_pos, *root_rot, *joint_pos, *root_lin_vel, *root_ang_vel, *joint_vel;
  float *body_pos, *body_quat, *body_lin_vel, *body_ang_vel;
  double dt;          // 1 / fps_out
  int64_t n_out;      // output frames of this member (out_offsets[n_seq])
  int64_t tile_base;  // first workgroup of this member
  int n_seq, pad;
};

// Byte offsets of the LDS arrays of one wavefront, and their sum (host and device agree on this layout).
struct TrackLds { int64_t rows, quats, src0, src1, a, h, rowm, rowp, pos, rot, slots, bytes; };
__host__ __device__ inline TrackLds track_lds(int nbody, int ndof, int nslots) {
  TrackLds l{};
  int64_t at = 0;
  l.rows = at;  at += (int64_t)motion_qpitch(ndof + 7) * kFkWave * 8;
  l.quats = at; at += (int64_t)8 * kFkWave * 8;
  l.src0 = at;  at += kFkWave * 8;
  l.src1 = at;  at += kFkWave * 8;
  l.a = at;     at += kFkWave * 8;
  l.h = at;     at += kFkWave * 8;
  l.rowm = at;  at += kFkWave * 4;
  l.rowp = at;  at += kFkWave * 4;
  l.pos = at;   at += (int64_t)3 * nbody * kFkWave * 4;  // (every offset so far is a multiple of 16)
  l.rot = at;   at += (int64_t)4 * nbody * kFkWave * 4;
  l.slots = at; at += (int64_t)(nslots > 1 ? nslots : 1) * 7 * kFkWave * 4;
  l.bytes = at;
  return l;
}
__host__ __device__ inline int64_t track_lds_bytes(int nbody, int ndof, int nslots) { return track_lds(nbody, ndof, nslots).bytes; }

__device__ __forceinline__ double track_lerp(double x0, double x1, double a) {
#pragma clang fp contract(off)
  return a == 0.0 ? x0 : x0 + a * (x1 - x0);  // (a = 0 is a copy, also of -0.0 and beside a non-finite x1)
}

// shortest-arc slerp of two xyzw quaternions, 0 < a < 1, normalised
__device__ __forceinline__ void track_slerp(const double q0[4], const double q1in[4], double a, double o[4]) {
#pragma clang fp contract(off)
  double q1[4] = {q1in[0], q1in[1], q1in[2], q1in[3]};
  double d = q0[0] * q1[0] + q0[1] * q1[1] + q0[2] * q1[2] + q0[3] * q1[3];
  if (d < 0.0) {
#pragma unroll
    for (int i = 0; i < 4; i++) q1[i] = -q1[i];
    d = -d;
  }
  const double om = acos(fmin(d, 1.0));
  double w0 = 1.0 - a, w1 = a;
  if (!(om < 1e-8)) {
    const double s = sin(om);
    w0 = sin((1.0 - a) * om) / s;
    w1 = sin(a * om) / s;
  }
  double r[4];
#pragma unroll
  for (int i = 0; i < 4; i++) r[i] = w0 * q0[i] + w1 * q1[i];
  const double n = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]);
#pragma unroll
  for (int i = 0; i < 4; i++) o[i] = r[i] / n;
}

// rotvec(p (x) conj(q)) / h for xyzw quaternions: the world-frame angular velocity that turns q into p in time h
__device__ __forceinline__ void track_ang_vel(const double p[4], const double q[4], double h, double o[3]) {
#pragma clang fp contract(off)
  double w = p[3] * q[3] + (p[0] * q[0] + p[1] * q[1] + p[2] * q[2]);
  double v[3] = {q[3] * p[0] - p[3] * q[0] - (p[1] * q[2] - p[2] * q[1]),
                 q[3] * p[1] - p[3] * q[1] - (p[2] * q[0] - p[0] * q[2]),
                 q[3] * p[2] - p[3] * q[2] - (p[0] * q[1] - p[1] * q[0])};
  if (w < 0.0) {
    w = -w;
#pragma unroll
    for (int i = 0; i < 3; i++) v[i] = -v[i];
  }
  const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  const double f = n > 1e-12 ? 2.0 * atan2(n, w) / n : 2.0;
#pragma unroll
  for (int i = 0; i < 3; i++) o[i] = v[i] * f / h;
}

// dst[i] = f(i) for i < n, consecutive lanes -> consecutive elements: 16 bytes per lane and store where dst allows it
template <class T, class F>
__device__ __forceinline__ void track_emit(T *dst, int n, int lane, F f) {
  constexpr int V = 16 / (int)sizeof(T);
  struct alignas(16) Vec { T v[V]; };
  int done = 0;
  if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    const int nv = n / V;
    for (int i = lane; i < nv; i += kFkWave) {
      Vec x;
#pragma unroll
      for (int u = 0; u < V; ++u) x.v[u] = f(V * i + u);
      *reinterpret_cast<Vec *>(dst + V * i) = x;
    }
    done = nv * V;
  }
  for (int i = done + lane; i < n; i += kFkWave) dst[i] = f(i);
}

__global__ void __launch_bounds__(kFkWave) motion_track_kernel(const TrackEntry *__restrict__ entries, int n_entries) {
#pragma clang fp contract(off)  // gmr_fk's arithmetic exactly; the float64 part as the contract writes it
  extern __shared__ __attribute__((aligned(16))) unsigned char track_smem[];
  const int lane = threadIdx.x;
  const int ei = launch_member<TrackEntry, &TrackEntry::tile_base>(entries, n_entries, (int64_t)blockIdx.x);
  const TrackEntry *ep = entries + ei;
  FkTree t{};  // the fields the chain reads (fk_body, fk_const)
  t.body = motion_const(&ep->fk.body);
  t.save_slot = motion_const(&ep->fk.save_slot);
  t.nbody = motion_const(&ep->fk.nbody);
  t.ndof = motion_const(&ep->fk.ndof);
  t.nslots = motion_const(&ep->fk.nslots);
  const double *__restrict__ qpos = motion_const(&ep->qpos);
  const int64_t n_out = motion_const(&ep->n_out);
  const int n_seq = motion_const(&ep->n_seq);
  const int64_t *soffs = motion_const(&ep->seq_offsets), *ooffs = motion_const(&ep->out_offsets);
  const double *ratios = motion_const(&ep->ratio);
  const double dt = motion_const(&ep->dt);
  float *const o_bpos = motion_const(&ep->body_pos), *const o_bquat = motion_const(&ep->body_quat);
  float *const o_blin = motion_const(&ep->body_lin_vel), *const o_bang = motion_const(&ep->body_ang_vel);
  const bool want_fk = o_bpos || o_bquat || o_blin || o_bang;
  const int nbody = t.nbody, ndof = t.ndof, nq = ndof + 7, qp = motion_qpitch(nq), row3 = 3 * nbody, row4 = 4 * nbody;
  const TrackLds L = track_lds(nbody, ndof, t.nslots);
  double *rows = reinterpret_cast<double *>(track_smem + L.rows);    // [64][qp]: x y z | qx qy qz qw | joints
  double *quats = reinterpret_cast<double *>(track_smem + L.quats);  // [64][8]: the two source quaternions (wxyz), later root_ang_vel
  int64_t *src0 = reinterpret_cast<int64_t *>(track_smem + L.src0), *src1 = reinterpret_cast<int64_t *>(track_smem + L.src1);
  double *wa = reinterpret_cast<double *>(track_smem + L.a), *wh = reinterpret_cast<double *>(track_smem + L.h);
  int *rowm = reinterpret_cast<int *>(track_smem + L.rowm), *rowp = reinterpret_cast<int *>(track_smem + L.rowp);
  float *ipos = reinterpret_cast<float *>(track_smem + L.pos), *irot = reinterpret_cast<float *>(track_smem + L.rot);
  float *slots = reinterpret_cast<float *>(track_smem + L.slots);
  const int64_t g0 = ((int64_t)blockIdx.x - motion_const(&ep->tile_base)) * kTrackTile;
  const int nfb = (int)(n_out - g0 < kTrackTile ? n_out - g0 : kTrackTile);  // output frames of this tile: rows 0 .. nfb-1
  const int row = (lane + kFkWave - 1) & (kFkWave - 1);
  // ---- 1: this lane's frame.  Halo lanes off the member, and the dead lanes of the last tile, repeat the nearest frame of the
  // member: they take part in everything and store nothing
  int64_t g = g0 + lane - 1;
  g = g < 0 ? 0 : g;
  g = g > n_out - 1 ? n_out - 1 : g;
  int s = 0;
  {
    const int64_t gmin = g0 > 0 ? g0 - 1 : 0;
    int hi = n_seq;
    while (hi - s > 1) {  // wave-uniform: scalar loads
      const int mid = (s + hi) >> 1;
      if (motion_const(ooffs + mid) <= gmin) s = mid; else hi = mid;
    }
    while (s + 1 < n_seq && ooffs[s + 1] <= g) ++s;  // (clips without output frames share their offset with the next and are skipped)
  }
  double a;
  {
    const int64_t ob = ooffs[s], Ms = ooffs[s + 1] - ob, sb = soffs[s], T = soffs[s + 1] - sb;  // T >= 1: the host refuses Ms > 0 with T = 0
    const int64_t k = g - ob;
    const double u = (double)k * ratios[s];
    const double fl = floor(u);
    int64_t i0 = fl >= (double)(T - 1) ? T - 1 : (int64_t)fl;  // the clamp, taken before the conversion
    i0 = i0 < 0 ? 0 : i0;
    const int64_t i1 = i0 + 1 < T ? i0 + 1 : T - 1;
    a = i1 > i0 ? u - (double)i0 : 0.0;
    const int64_t km = k > 0 ? k - 1 : 0, kp = k + 1 < Ms ? k + 1 : Ms - 1;
    src0[row] = sb + i0;
    src1[row] = sb + i1;
    wa[row] = a;
    wh[row] = (double)(kp - km) * dt;
    rowm[row] = (row - (int)(k - km)) & (kFkWave - 1);  // the neighbour's lane is this lane -1 / +1, and so is its row
    rowp[row] = (row + (int)(kp - k)) & (kFkWave - 1);
  }
  __syncthreads();
  // ---- 2: both source rows of all 64 frames, one (frame, column) per lane and load pair
  {
    const int n = kFkWave * nq;
    const float inv_nq = 1.0f / (float)nq;
    for (int base = 0; base < n; base += kMotionBatch * kFkWave) {
      double v0[kMotionBatch], v1[kMotionBatch];
#pragma unroll
      for (int b = 0; b < kMotionBatch; ++b) {
        const int i = base + b * kFkWave + lane;
        v0[b] = v1[b] = 0.0;
        if (i < n) {
          const int fr = motion_div(i, inv_nq), c = i - fr * nq;
          v0[b] = qpos[src0[fr] * nq + c];
          v1[b] = qpos[src1[fr] * nq + c];
        }
      }
#pragma unroll
      for (int b = 0; b < kMotionBatch; ++b) {
        const int i = base + b * kFkWave + lane;
        if (i < n) {
          const int fr = motion_div(i, inv_nq), c = i - fr * nq;
          if (c >= 3 && c < 7) {
            quats[fr * 8 + c - 3] = v0[b];
            quats[fr * 8 + c + 1] = v1[b];
          } else {
            rows[fr * qp + c] = track_lerp(v0[b], v1[b], wa[fr]);
          }
        }
      }
    }
  }
  __syncthreads();
  // ---- 3: slerp (wxyz in, xyzw out), then the chain on the float32 casts of the resampled row
  {
    double q0[4], q1[4], qr[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      q0[i] = quats[row * 8 + ((i + 1) & 3)];
      q1[i] = quats[row * 8 + 4 + ((i + 1) & 3)];
    }
    // a = 0 is a copy; so are two identical source rows (a standing robot): the slerp of q with itself would give q / |q|, an ulp
    // beside the copied rows of the same clip, and a velocity that is not zero
    if (a == 0.0 || (q0[0] == q1[0] && q0[1] == q1[1] && q0[2] == q1[2] && q0[3] == q1[3])) {
#pragma unroll
      for (int i = 0; i < 4; i++) qr[i] = q0[i];
    } else {
      track_slerp(q0, q1, a, qr);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) rows[row * qp + 3 + i] = qr[i];
  }
  if (want_fk) {  // (wave-uniform) fk_pos_kernel's chain, the dof angles read out of the row image, rotations kept too
    const double *my = rows + row * qp;
    float cp[3], cr[4];
#pragma unroll
    for (int i = 0; i < 3; i++) cp[i] = (float)my[i];
#pragma unroll
    for (int i = 0; i < 4; i++) cr[i] = (float)my[3 + i];
    auto save = [&](int sv) {
      float *sl = slots + (size_t)sv * 7 * kFkWave + lane;
#pragma unroll
      for (int i = 0; i < 3; i++) sl[i * kFkWave] = cp[i];
#pragma unroll
      for (int i = 0; i < 4; i++) sl[(3 + i) * kFkWave] = cr[i];
    };
    auto keep = [&](int j) {
#pragma unroll
      for (int i = 0; i < 3; i++) ipos[row * row3 + 3 * j + i] = cp[i];
#pragma unroll
      for (int i = 0; i < 4; i++) irot[row * row4 + 4 * j + i] = cr[i];
    };
    if (fk_const(t.save_slot, 0) >= 0) save(fk_const(t.save_slot, 0));
    keep(0);
    FkBody nxt = fk_body(t, nbody > 1 ? 1 : 0);
    for (int j = 1; j < nbody; ++j) {
      const FkBody rec = nxt;
      nxt = fk_body(t, j + 1 < nbody ? j + 1 : j);  // one body ahead
      float pp[3], pr[4];
      const int src = rec.src_slot;
      if (src < 0) {
#pragma unroll
        for (int i = 0; i < 3; i++) pp[i] = cp[i];
#pragma unroll
        for (int i = 0; i < 4; i++) pr[i] = cr[i];
      } else {
        const float *sl = slots + (size_t)src * 7 * kFkWave + lane;
#pragma unroll
        for (int i = 0; i < 3; i++) pp[i] = sl[i * kFkWave];
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
      keep(j);
      if (rec.save_slot >= 0) save(rec.save_slot);
    }
  }
  __syncthreads();
  // ---- 4: the outputs of rows 0 .. nfb-1
  const int rm = rowm[row], rp = rowp[row];
  const double h = wh[row];
  double *const o_rav = motion_const(&ep->root_ang_vel);
  if (o_rav) {  // per lane, handed to the linear store below through the (now dead) quaternion park
    double w[3] = {0.0, 0.0, 0.0};
    if (h != 0.0) track_ang_vel(rows + rp * qp + 3, rows + rm * qp + 3, h, w);
#pragma unroll
    for (int i = 0; i < 3; i++) quats[row * 8 + i] = w[i];
    __syncthreads();
    track_emit(o_rav + g0 * 3, nfb * 3, lane, [&](int i) {
      const int fr = motion_div(i, 1.0f / 3.0f);
      return quats[fr * 8 + i - fr * 3];
    });
  }
  auto diff = [&](int fr, int c) {  // central difference of column c of the row image
    const double hh = wh[fr];
    return hh != 0.0 ? (rows[rowp[fr] * qp + c] - rows[rowm[fr] * qp + c]) / hh : 0.0;
  };
  if (double *o = motion_const(&ep->root_pos))
    track_emit(o + g0 * 3, nfb * 3, lane, [&](int i) { const int fr = motion_div(i, 1.0f / 3.0f); return rows[fr * qp + i - fr * 3]; });
  if (double *o = motion_const(&ep->root_rot))
    track_emit(o + g0 * 4, nfb * 4, lane, [&](int i) { return rows[(i >> 2) * qp + 3 + (i & 3)]; });
  if (double *o = motion_const(&ep->root_lin_vel))
    track_emit(o + g0 * 3, nfb * 3, lane, [&](int i) { const int fr = motion_div(i, 1.0f / 3.0f); return diff(fr, i - fr * 3); });
  if (ndof > 0) {
    const float inv_ndof = 1.0f / (float)ndof;
    if (double *o = motion_const(&ep->joint_pos))
      track_emit(o + g0 * ndof, nfb * ndof, lane, [&](int i) { const int fr = motion_div(i, inv_ndof); return rows[fr * qp + 7 + i - fr * ndof]; });
    if (double *o = motion_const(&ep->joint_vel))
      track_emit(o + g0 * ndof, nfb * ndof, lane, [&](int i) { const int fr = motion_div(i, inv_ndof); return diff(fr, 7 + i - fr * ndof); });
  }
  if (!want_fk) return;
  if (o_bpos) track_emit(o_bpos + g0 * row3, nfb * row3, lane, [&](int i) { return ipos[i]; });
  if (o_bquat) track_emit(o_bquat + g0 * row4, nfb * row4, lane, [&](int i) { return irot[i]; });
  if (o_blin) {
    const float inv_row3 = 1.0f / (float)row3;
    track_emit(o_blin + g0 * row3, nfb * row3, lane, [&](int i) {
      const int fr = motion_div(i, inv_row3), c = i - fr * row3;
      const double hh = wh[fr];
      return hh != 0.0 ? (float)(((double)ipos[rowp[fr] * row3 + c] - (double)ipos[rowm[fr] * row3 + c]) / hh) : 0.f;
    });
  }
  if (o_bang) {  // one (frame, body) item per lane
    struct F3 { float x, y, z; };  // 12 bytes, 4-byte aligned
    const float inv_nb = 1.0f / (float)nbody;
    float *dst = o_bang + g0 * row3;
    for (int i = lane; i < nfb * nbody; i += kFkWave) {
      const int fr = motion_div(i, inv_nb), b = i - fr * nbody;
      const double hh = wh[fr];
      double w[3] = {0.0, 0.0, 0.0};
      if (hh != 0.0) {
        const float *fp = irot + rowp[fr] * row4 + 4 * b, *fm = irot + rowm[fr] * row4 + 4 * b;
        const double p[4] = {(double)fp[0], (double)fp[1], (double)fp[2], (double)fp[3]};
        const double q[4] = {(double)fm[0], (double)fm[1], (double)fm[2], (double)fm[3]};
        track_ang_vel(p, q, hh, w);
      }
      *reinterpret_cast<F3 *>(dst + 3 * i) = F3{(float)w[0], (float)w[1], (float)w[2]};
    }
  }
}

}  // namespace gmr

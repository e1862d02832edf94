// self_collision_repair_kernel.hip.h -- push colliding capsule pairs apart in float64, two launches
// (gmr_motion_self_collision_repair; the definition is the contract above gmr_self_collision_repair_input in include/gmr_amd.h).
//
//   a  self_collision_repair_kernel        grid (clip, wavefronts per clip: each strides over its clip's frames), one wavefront per
//                                          workgroup, ONE frame per wavefront at a time.  The row is staged in LDS (coalesced, with
//                                          the finite check); then up to I + 1 evaluations, each
//                                            1  LANE = BODY: the pose sweep of self_collision_kernel.hip.h, level by level, 7
//                                               doubles per body left in LDS; the lane keeps its own pose, and a hinge's lane its
//                                               angle, its start angle and its world axis in registers -- LANE = HINGE is the same
//                                               lane, so the Jacobian needs no second sweep;
//                                            2  LANE = CAPSULE in ceil(C / 64) passes: the world ends, 6 doubles per capsule, to LDS;
//                                            3  LANE = PAIR in passes of 64, ascending: closest points, clearance (running minimum
//                                               and NaN flag for clearance_before / clearance_after), violation v.  One ballot of
//                                               the lanes with v > 0 and a moving set; those park a, b, n, v and their two ancestor
//                                               masks in LDS.  For every set bit from the lowest up all lanes read that pair's ten
//                                               doubles and two masks at one address (an LDS broadcast), a hinge's lane forms its
//                                               gradient entry, one wave_sum gives sum g^2, and the lane adds v rho g to its own
//                                               accumulator: the active pairs arrive in ascending index without a list in memory;
//                                            4  LANE = HINGE: divide by V, wave_max for the step cap, clamp to the widened limits.
//                                          A frame without a violation costs one evaluation and leaves the loop wave-uniformly.
//                                          The ancestor masks are bit sets over BODIES (bit b: body b is a hinge on the path), made
//                                          on the host with the caller's hinge mask already applied (api.hip), staged per capsule.
//   b  self_collision_repair_stats_kernel  one wavefront per clip, lane = frame in tiles of 64: counts by ballot, maximum and minimum
//                                          by one wave reduction.  Reads clearance_after and move of a.
//
// Weaknesses, not engineered away: one frame per wavefront leaves 64 - nbody lanes idle in phases 1 and 4 and in the gradient (26
// of 64 on G1), where the report packs two frames side by side; phase 1 costs one LDS round trip per tree level; the pairs of a
// passive frame are still evaluated once; sum g^2 is a full 64-lane reduction per active pair whatever the moving set's size
// (DESIGN.md 4.21).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dynamics_kernel.hip.h"  // dyn_clamp, dyn_qmul, dyn_rot, dyn_cross
#include "fk_kernel.hip.h"        // kFkWave
#include "ik_kernel.hip.h"        // DevModel, wave_min / wave_max / wave_sum
#include "tree_chain.hip.h"       // wave_lds_sync

namespace gmr {

constexpr int kScrMaxCaps = 256;        // capsules of one call
constexpr int kScrMaxPairs = 32768;     // pairs of one call
constexpr int kScrCapPasses = kScrMaxCaps / kFkWave;
constexpr int kScrPairsLdsMax = 4096;   // pair tables up to this size are staged in LDS as 16-bit words
constexpr int kScrTargetWaves = 8192;   // wavefronts of one launch of kernel a that the host aims for
constexpr int kScrMaxIters = 32;
constexpr int kScrPose = 7;             // doubles a body leaves in LDS: x(3) r(4)
constexpr int kScrPark = 10;            // doubles an active pair parks: a(3) b(3) n(3) v
constexpr int kScrRow = 72;             // doubles of the staged row: nq <= 7 + 63

struct SelfCollisionRepairArgs {
  const DevModel *dm;            // the full body tree (gmr_evaluate's)
  const double *lo, *hi;         // [nq - 7] hinge limits in qpos order, -inf / +inf where unlimited
  const double *qpos;
  const int64_t *seq_offsets;
  int64_t n_frames;
  int n_seq, nbody, nq, n_caps, n_pairs, iters;
  const int32_t *cap_body;
  const double *cap_p0, *cap_p1, *cap_radius;
  const int32_t *pairs;
  double margin, damping, step_cap, resolve_tol;
  double *qpos_out, *before, *after, *move;
  int32_t *repaired, *unresolved;
  double *move_max, *clearance_min_after;
  int32_t *nonfinite;
  uint64_t movable;              // bit b: body b is a hinge the caller lets move
  uint64_t anc[kFkWave];         // per body: the movable hinge bodies on its path from the root, itself included
  uint8_t parent[kFkWave], depth[kFkWave];   // the tree, from the blob (parent of the root: 0xff)
};

// bytes of dynamic LDS of kernel a: poses | ends and radii | parked pairs | row | capsule masks | parked masks | packed pairs
__host__ __device__ inline int self_collision_repair_lds_bytes(int n_caps, int n_pairs, bool pairs_in_lds) {
  return (kScrPose * kFkWave + 7 * n_caps + kScrPark * kFkWave + kScrRow + n_caps + 2 * kFkWave) * 8 + (pairs_in_lds ? 2 * n_pairs : 0);
}

__device__ __forceinline__ int scr_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ double scr_clamp01(double x) { return x > 0.0 ? (x < 1.0 ? x : 1.0) : 0.0; }   // 0 for a NaN
__device__ __forceinline__ double scr_dot(const double u[3], const double v[3]) {
#pragma clang fp contract(off)
  return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2];
}

// The closest points of the segments p1 .. q1 and p2 .. q2: the report's clamped formula in its operation order, with the points.
__device__ __forceinline__ void scr_closest(const double p1[3], const double q1[3], const double p2[3], const double q2[3], double pa[3], double pb[3]) {
#pragma clang fp contract(off)
  const double d1[3] = {q1[0] - p1[0], q1[1] - p1[1], q1[2] - p1[2]};
  const double d2[3] = {q2[0] - p2[0], q2[1] - p2[1], q2[2] - p2[2]};
  const double r[3] = {p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2]};
  const double a = scr_dot(d1, d1), e = scr_dot(d2, d2), f = scr_dot(d2, r), c = scr_dot(d1, r), b = scr_dot(d1, d2);
  const double den = a * e - b * b;
  double s = den > 0.0 ? scr_clamp01((b * f - c * e) / den) : 0.0;
  double t = e > 0.0 ? (b * s + f) / e : 0.0;
  if (!(e > 0.0) || t < 0.0) {
    t = 0.0;
    s = a > 0.0 ? scr_clamp01(-c / a) : 0.0;
  } else if (t > 1.0) {
    t = 1.0;
    s = a > 0.0 ? scr_clamp01((b - c) / a) : 0.0;
  }
  for (int k = 0; k < 3; ++k) { pa[k] = p1[k] + s * d1[k]; pb[k] = p2[k] + t * d2[k]; }
}

// ------------------------------------------------------------------ a: per frame
// grid (n_seq, wavefronts per clip); dynamic LDS: self_collision_repair_lds_bytes
template <bool kPairsLds>
__global__ void __launch_bounds__(kFkWave) self_collision_repair_kernel(const SelfCollisionRepairArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double scr_lds[];
  const int lane = threadIdx.x;
  const int nb = a.nbody, nq = a.nq, C = a.n_caps, P = a.n_pairs, I = a.iters;
  double *const pose = scr_lds;                      // [kScrPose][64]
  double *const ends = pose + kScrPose * kFkWave;    // [6][C]
  double *const rad = ends + 6 * C;                  // [C]
  double *const park = rad + C;                      // [kScrPark][64]
  double *const row = park + kScrPark * kFkWave;     // [kScrRow]
  uint64_t *const capanc = reinterpret_cast<uint64_t *>(row + kScrRow);   // [C]
  uint64_t *const pmask = capanc + C;                // [2][64]: the moving set, the first capsule's ancestors
  uint16_t *const packed = reinterpret_cast<uint16_t *>(pmask + 2 * kFkWave);   // [P], <true> only
  const bool active = lane < nb;
  const int bj = active ? lane : 0;   // (idle lanes read body 0's constants and never write)
  const DevModel *dm = a.dm;

  // the lane's body, once per launch
  const int par = bj > 0 ? scr_clampi((int)a.parent[bj], nb - 1) : 0;
  const int depth = a.depth[bj];
  int maxd = active ? depth : 0;
  for (int off = 32; off; off >>= 1) { const int o = __shfl_xor(maxd, off); maxd = o > maxd ? o : maxd; }
  const bool hinge = active && bj > 0 && dm->jtype[bj] == GMR_JNT_HINGE;
  const bool root = active && bj == 0;
  const int qadr = hinge ? 7 + scr_clampi(dm->qadr[bj] - 7, nq - 8) : 7;   // (a hinge's column, 7 .. nq - 1)
  const bool movable = hinge && ((a.movable >> bj) & 1ull);
  const double bpos[3] = {dm->bpos[3 * bj], dm->bpos[3 * bj + 1], dm->bpos[3 * bj + 2]};
  const double bquat[4] = {dm->bquat[4 * bj], dm->bquat[4 * bj + 1], dm->bquat[4 * bj + 2], dm->bquat[4 * bj + 3]};
  const double axis[3] = {dm->axis[3 * bj], dm->axis[3 * bj + 1], dm->axis[3 * bj + 2]};
  const double lim_lo = hinge ? a.lo[qadr - 7] : 0.0, lim_hi = hinge ? a.hi[qadr - 7] : 0.0;
  const uint64_t mybit = 1ull << bj;

  // the lane's capsules, once per launch; radii, ancestor masks (and the pair table) go to LDS
  double cp0[kScrCapPasses][3], cp1[kScrCapPasses][3];
  int cbody[kScrCapPasses];
#pragma unroll
  for (int kk = 0; kk < kScrCapPasses; ++kk) {
    const int ci = kFkWave * kk + lane;
    const int cc = ci < C ? ci : 0;
    cbody[kk] = scr_clampi(a.cap_body[cc], nb - 1);
    for (int c = 0; c < 3; ++c) { cp0[kk][c] = a.cap_p0[3 * cc + c]; cp1[kk][c] = a.cap_p1[3 * cc + c]; }
    if (ci < C) { rad[ci] = a.cap_radius[ci]; capanc[ci] = a.anc[cbody[kk]]; }
  }
  if (kPairsLds) {
    for (int p = lane; p < P; p += kFkWave)
      packed[p] = (uint16_t)(scr_clampi(a.pairs[2 * p], C - 1) | (scr_clampi(a.pairs[2 * p + 1], C - 1) << 8));
  }
  wave_lds_sync();

  const int64_t r0 = dyn_clamp(a.seq_offsets[blockIdx.x], 0, a.n_frames);
  const int64_t r1 = dyn_clamp(a.seq_offsets[blockIdx.x + 1], r0, a.n_frames);
  const int64_t T = r1 - r0;
  const double inf = __longlong_as_double(0x7ff0000000000000ll), nan = __longlong_as_double(0x7ff8000000000000ll);

  for (int64_t k = blockIdx.y; k < T; k += gridDim.y) {
    const int64_t g = r0 + k;
    // ---- the row: staged, checked
    wave_lds_sync();   // (the previous frame no longer reads the buffers)
    bool fin = true;
    for (int i = lane; i < nq; i += kFkWave) {
      const double v = a.qpos[g * nq + i];
      row[i] = v;
      fin = fin && __builtin_isfinite(v);
    }
    const bool valid = __ballot(!fin) == 0;
    wave_lds_sync();
    const double q0 = hinge ? row[qadr] : 0.0;
    double th = q0;
    double x[3] = {0.0, 0.0, 0.0}, r[4] = {1.0, 0.0, 0.0, 0.0};
    if (root) {
      const double qn = sqrt(row[3] * row[3] + row[4] * row[4] + row[5] * row[5] + row[6] * row[6]);
      x[0] = row[0]; x[1] = row[1]; x[2] = row[2];
      r[0] = row[3] / qn; r[1] = row[4] / qn; r[2] = row[5] / qn; r[3] = row[6] / qn;
    }
    double cl_before = nan, cl_after = nan;
    for (int pass = 0; valid; ++pass) {   // (valid is wave-uniform: an invalid frame is copied through)
      // ---- 1: poses, LANE = BODY
      for (int d = 0; d <= maxd; ++d) {
        if (active && depth == d) {
          if (d > 0) {
            const double xp[3] = {pose[0 * kFkWave + par], pose[1 * kFkWave + par], pose[2 * kFkWave + par]};
            const double rp[4] = {pose[3 * kFkWave + par], pose[4 * kFkWave + par], pose[5 * kFkWave + par], pose[6 * kFkWave + par]};
            double dd[3], t[4];
            dyn_rot(rp, bpos, dd);
            x[0] = xp[0] + dd[0]; x[1] = xp[1] + dd[1]; x[2] = xp[2] + dd[2];
            dyn_qmul(rp, bquat, t);
            if (hinge) {
              const double hh = 0.5 * th;
              const double sn = sin(hh), cs = cos(hh);
              const double jq[4] = {cs, sn * axis[0], sn * axis[1], sn * axis[2]};
              dyn_qmul(t, jq, r);
            } else {
              r[0] = t[0]; r[1] = t[1]; r[2] = t[2]; r[3] = t[3];
            }
          }
          pose[0 * kFkWave + lane] = x[0]; pose[1 * kFkWave + lane] = x[1]; pose[2 * kFkWave + lane] = x[2];
          pose[3 * kFkWave + lane] = r[0]; pose[4 * kFkWave + lane] = r[1]; pose[5 * kFkWave + lane] = r[2]; pose[6 * kFkWave + lane] = r[3];
        }
        wave_lds_sync();
      }
      double u[3];
      dyn_rot(r, axis, u);   // the hinge's world axis (unused off a hinge's lane)

      // ---- 2: world ends, LANE = CAPSULE
#pragma unroll
      for (int kk = 0; kk < kScrCapPasses; ++kk) {
        const int ci = kFkWave * kk + lane;
        if (ci < C) {
          const int sl = cbody[kk];
          const double xb[3] = {pose[0 * kFkWave + sl], pose[1 * kFkWave + sl], pose[2 * kFkWave + sl]};
          const double rb[4] = {pose[3 * kFkWave + sl], pose[4 * kFkWave + sl], pose[5 * kFkWave + sl], pose[6 * kFkWave + sl]};
          double e0[3], e1[3];
          dyn_rot(rb, cp0[kk], e0);
          dyn_rot(rb, cp1[kk], e1);
          ends[0 * C + ci] = xb[0] + e0[0]; ends[1 * C + ci] = xb[1] + e0[1]; ends[2 * C + ci] = xb[2] + e0[2];
          ends[3 * C + ci] = xb[0] + e1[0]; ends[4 * C + ci] = xb[1] + e1[1]; ends[5 * C + ci] = xb[2] + e1[2];
        }
      }
      wave_lds_sync();

      // ---- 3: pairs in passes of 64, ascending; the active ones one by one, LANE = HINGE
      const bool step = pass < I;   // (the evaluation after the last pass only measures)
      double best = inf, acc = 0.0, V = 0.0;
      bool bad = false;
      for (int p0 = 0; p0 < P; p0 += kFkWave) {
        const int p = p0 + lane;
        const bool in = p < P;
        const int pp = in ? p : 0;
        int ia, ib;
        if (kPairsLds) {
          const unsigned w = packed[pp];
          ia = (int)(w & 0xffu); ib = (int)(w >> 8);
        } else {
          ia = scr_clampi(a.pairs[2 * pp], C - 1); ib = scr_clampi(a.pairs[2 * pp + 1], C - 1);
        }
        const double p1[3] = {ends[0 * C + ia], ends[1 * C + ia], ends[2 * C + ia]}, q1[3] = {ends[3 * C + ia], ends[4 * C + ia], ends[5 * C + ia]};
        const double p2[3] = {ends[0 * C + ib], ends[1 * C + ib], ends[2 * C + ib]}, q2[3] = {ends[3 * C + ib], ends[4 * C + ib], ends[5 * C + ib]};
        double pa[3], pb[3];
        scr_closest(p1, q1, p2, q2, pa, pb);
        const double w[3] = {pa[0] - pb[0], pa[1] - pb[1], pa[2] - pb[2]};
        const double nw = sqrt(scr_dot(w, w));
        const double cl = nw - (rad[ia] + rad[ib]);
        if (in) {
          bad = bad || cl != cl;
          best = cl < best ? cl : best;
        }
        if (!step) continue;   // (wave-uniform)
        const uint64_t ax = capanc[ia], mv = ax ^ capanc[ib];
        const double vv = a.margin - cl;
        const bool act = in && vv > 0.0 && mv != 0ull;   // (a NaN is not > 0)
        u64 todo = __ballot(act);
        if (!todo) continue;   // (wave-uniform)
        if (act) {
          const bool sep = nw > 0.0;
          park[0 * kFkWave + lane] = pa[0]; park[1 * kFkWave + lane] = pa[1]; park[2 * kFkWave + lane] = pa[2];
          park[3 * kFkWave + lane] = pb[0]; park[4 * kFkWave + lane] = pb[1]; park[5 * kFkWave + lane] = pb[2];
          park[6 * kFkWave + lane] = sep ? w[0] / nw : 0.0; park[7 * kFkWave + lane] = sep ? w[1] / nw : 0.0;
          park[8 * kFkWave + lane] = sep ? w[2] / nw : 0.0; park[9 * kFkWave + lane] = vv;
          pmask[lane] = mv; pmask[kFkWave + lane] = ax;
        }
        wave_lds_sync();
        while (todo) {
          const int b = (int)__builtin_ctzll(todo);
          todo &= todo - 1;
          const uint64_t mset = pmask[b], xset = pmask[kFkWave + b];
          const double n[3] = {park[6 * kFkWave + b], park[7 * kFkWave + b], park[8 * kFkWave + b]};
          const double v = park[9 * kFkWave + b];
          double gi = 0.0;
          if (hinge && (mset & mybit)) {
            const bool on_x = (xset & mybit) != 0ull;   // the hinge carries the pair's first capsule, else its second
            const int o = on_x ? 0 : 3;
            const double arm[3] = {park[(o + 0) * kFkWave + b] - x[0], park[(o + 1) * kFkWave + b] - x[1], park[(o + 2) * kFkWave + b] - x[2]};
            double cr[3];
            dyn_cross(u, arm, cr);
            const double d = scr_dot(n, cr);
            gi = on_x ? d : -d;
          }
          const double s2 = wave_sum(gi * gi);
          const double rho = v / (s2 + a.damping);
          acc = acc + (v * rho) * gi;
          V = V + v;
        }
        wave_lds_sync();   // (the next pass of pairs parks over these)
      }
      const bool any_bad = __ballot(bad) != 0;
      const double amin = wave_min(best);   // (no lane holds a NaN: those were flagged apart)
      cl_after = any_bad ? nan : amin;
      if (pass == 0) cl_before = cl_after;
      if (!step || __ballot(V > 0.0) == 0) break;   // (V is the same in every lane)

      // ---- 4: the step, LANE = HINGE
      const double dq = acc / V;
      const double m = wave_max(fabs(dq));
      const double scale = m > a.step_cap ? a.step_cap / m : 1.0;
      if (movable && dq != 0.0) {
        const double lw = lim_lo < q0 ? lim_lo : q0, hw = lim_hi > q0 ? lim_hi : q0;
        const double qn = th + scale * dq;
        th = qn < lw ? lw : (qn > hw ? hw : qn);
      }
      wave_lds_sync();   // (the next evaluation overwrites poses and ends)
    }

    // ---- outputs: the row with the hinges' final angles, element-wise and coalesced
    const double mv = wave_max(hinge && valid ? fabs(th - q0) : 0.0);
    if (hinge && valid) row[qadr] = th;   // (an untouched hinge puts its own bits back)
    wave_lds_sync();
    for (int i = lane; i < nq; i += kFkWave) a.qpos_out[g * nq + i] = row[i];
    if (lane == 0) {
      if (a.before) a.before[g] = cl_before;
      if (a.after) a.after[g] = cl_after;
      if (a.move) a.move[g] = mv;
    }
  }
}

// ------------------------------------------------------------------ b: per clip
// grid (n_seq); lane = frame, tiles of 64
__global__ void __launch_bounds__(kFkWave) self_collision_repair_stats_kernel(const SelfCollisionRepairArgs a) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int64_t r0 = dyn_clamp(a.seq_offsets[s], 0, a.n_frames);
  const int64_t r1 = dyn_clamp(a.seq_offsets[s + 1], r0, a.n_frames);
  const int64_t T = r1 - r0;
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  const double thr = a.margin - a.resolve_tol;
  double cmin = inf, mmax = 0.0;
  int repaired = 0, unresolved = 0, nonfinite = 0;
  for (int64_t k0 = 0; k0 < T; k0 += kFkWave) {
    const bool in = k0 + lane < T;
    const int64_t g = r0 + k0 + lane;
    const double cl = in ? a.after[g] : 0.0;
    const double mv = in ? a.move[g] : 0.0;
    const bool isn = in && cl != cl;
    const bool ok = in && !isn;
    repaired += __popcll(__ballot(ok && mv > 0.0));
    unresolved += __popcll(__ballot(ok && cl < thr));
    nonfinite += __popcll(__ballot(isn));
    if (ok) {
      cmin = cl < cmin ? cl : cmin;
      mmax = mv > mmax ? mv : mmax;
    }
  }
  const double wmin = wave_min(cmin), wmax = wave_max(mmax);
  if (lane == 0) {
    if (a.repaired) a.repaired[s] = repaired;
    if (a.unresolved) a.unresolved[s] = unresolved;
    if (a.move_max) a.move_max[s] = wmax;
    if (a.clearance_min_after) a.clearance_min_after[s] = wmin;
    if (a.nonfinite) a.nonfinite[s] = nonfinite;
  }
}

}  // namespace gmr

// self_collision_kernel.hip.h -- capsule clearance of retargeted qpos in float64, two launches (gmr_motion_self_collision; the
// definition is the contract above gmr_self_collision_input in include/gmr_amd.h).
//
//   a  motion_self_collision_kernel        grid (clip, wavefronts per clip: each strides over its clip's frame slots), one wavefront
//                                          per workgroup, three phases per pass:
//                                            1  LANE = BODY with tree_chain's geometry (chain_geom: skeletons of up to 32 bodies put
//                                               64 / jp frames side by side): the pose sweep of dynamics_kernel.hip.h, level by
//                                               level, 7 doubles per body left in LDS;
//                                          then per frame of the pass
//                                            2  LANE = CAPSULE in ceil(C / 64) passes: the world ends, 6 doubles per capsule, to LDS;
//                                            3  lane l takes the pairs l, l + 64, ...: both capsules' ends and radii from LDS, a
//                                               running (clearance, index) minimum that keeps the lower index on equality, a NaN
//                                               flag and a hit count; one wavefront reduction (wave_min of the clearance, wave_min
//                                               of the index over the lanes that hold it, wave_sum of the hits) and lane 0 stores.
//                                          A lane keeps its body's and its capsules' constants in registers for the whole launch; the
//                                          radii and, in the <true> instance, the pair indices (one 16-bit word per pair: n_caps <=
//                                          256) are staged in LDS once per wavefront.  The <false> instance re-reads the pair table
//                                          (8 bytes per pair, consecutive across the lanes) from L2 in every frame; the host picks
//                                          (api.hip, self_collision_run).
//   b  motion_self_collision_stats_kernel  one wavefront per clip, lane = frame in tiles of 64: the minimum with its earliest frame,
//                                          the counts, and the longest run of colliding frames from one ballot per tile (a lane's
//                                          run length is its distance to the highest clear bit at or below it; what crosses a tile
//                                          edge is the run that ends in lane 63).  Reads the three per-frame outputs of a.
//
// The minimum of a frame and its index are properties of the pair table, not of the schedule: a lane's pairs come in ascending order
// and `<` keeps the first, the index reduction takes the lowest index among the lanes at the minimum, so neither the number of pairs
// per lane nor the number of wavefronts per clip can change a byte.
//
// Weaknesses, not engineered away: phase 1 costs one LDS round trip per tree level with most lanes idle (as in the dynamics kernel),
// phase 2 leaves 64 - C % 64 lanes idle in its last pass, and the reads of phase 3 are indexed ds_read_b64 with whatever bank
// conflicts the pair table implies.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dynamics_kernel.hip.h"  // dyn_clamp, dyn_qmul, dyn_rot
#include "fk_kernel.hip.h"        // kFkWave
#include "ik_kernel.hip.h"        // DevModel, wave_min / wave_max / wave_sum
#include "tree_chain.hip.h"       // chain_geom, wave_lds_sync

namespace gmr {

constexpr int kColMaxCaps = 256;        // capsules of one call: an index fits a byte
constexpr int kColMaxPairs = 32768;     // pairs of one call
constexpr int kColCapPasses = kColMaxCaps / kFkWave;   // capsules a lane owns at most
constexpr int kColPairsLdsMax = 4096;   // pair tables up to this size may be staged in LDS (8 KiB: the tile stays below 28 KiB)
constexpr int kColTargetWaves = 8192;   // wavefronts of one launch of kernel a that the host aims for (api.hip, self_collision_run)
constexpr int kColPose = 7;             // doubles a body leaves in LDS: x(3) r(4)

struct SelfCollisionArgs {
  const DevModel *dm;            // the full body tree (gmr_evaluate's)
  const double *qpos;
  const int64_t *seq_offsets;
  int64_t n_frames;
  int n_seq, nbody, nq, n_caps, n_pairs;
  const int32_t *cap_body;
  const double *cap_p0, *cap_p1, *cap_radius;
  const int32_t *pairs;
  double margin;
  double *clearance;
  int32_t *pair, *hits;
  double *clearance_min;
  int32_t *worst_frame, *worst_pair, *colliding, *longest_run;
  int64_t *hits_sum;
  int32_t *nonfinite;
  uint8_t parent[kFkWave], depth[kFkWave];   // the tree, from the blob (parent of the root: 0xff)
};

// bytes of dynamic LDS of kernel a: poses, ends and radii, then the packed pairs
__host__ __device__ inline int self_collision_lds_bytes(int n_caps, int n_pairs, bool pairs_in_lds) {
  return (kColPose * kFkWave + 7 * n_caps) * 8 + (pairs_in_lds ? 2 * n_pairs : 0);
}

__device__ __forceinline__ int col_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ double col_clamp01(double x) { return x > 0.0 ? (x < 1.0 ? x : 1.0) : 0.0; }   // 0 for a NaN
__device__ __forceinline__ double col_dot(const double u[3], const double v[3]) {
#pragma clang fp contract(off)
  return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2];
}

// The distance of the segments p1 .. q1 and p2 .. q2: the contract's clamped closest points, in its operation order.
__device__ __forceinline__ double col_segment_distance(const double p1[3], const double q1[3], const double p2[3], const double q2[3]) {
#pragma clang fp contract(off)
  const double d1[3] = {q1[0] - p1[0], q1[1] - p1[1], q1[2] - p1[2]};
  const double d2[3] = {q2[0] - p2[0], q2[1] - p2[1], q2[2] - p2[2]};
  const double r[3] = {p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2]};
  const double a = col_dot(d1, d1), e = col_dot(d2, d2), f = col_dot(d2, r), c = col_dot(d1, r), b = col_dot(d1, d2);
  const double den = a * e - b * b;
  double s = den > 0.0 ? col_clamp01((b * f - c * e) / den) : 0.0;
  double t = e > 0.0 ? (b * s + f) / e : 0.0;
  if (!(e > 0.0) || t < 0.0) {   // (a second segment without length: the point of the first nearest to it)
    t = 0.0;
    s = a > 0.0 ? col_clamp01(-c / a) : 0.0;
  } else if (t > 1.0) {
    t = 1.0;
    s = a > 0.0 ? col_clamp01((b - c) / a) : 0.0;
  }
  const double w[3] = {(p1[0] + s * d1[0]) - (p2[0] + t * d2[0]), (p1[1] + s * d1[1]) - (p2[1] + t * d2[1]),
                       (p1[2] + s * d1[2]) - (p2[2] + t * d2[2])};
  return sqrt(col_dot(w, w));
}

// ------------------------------------------------------------------ a: per frame
// grid (n_seq, wavefronts per clip); dynamic LDS: self_collision_lds_bytes
template <bool kPairsLds>
__global__ void __launch_bounds__(kFkWave) motion_self_collision_kernel(const SelfCollisionArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double col_lds[];
  const int lane = threadIdx.x;
  const int nb = a.nbody, nq = a.nq, C = a.n_caps, P = a.n_pairs;
  double *const pose = col_lds;                      // [kColPose][64]
  double *const ends = pose + kColPose * kFkWave;    // [6][C]
  double *const rad = ends + 6 * C;                  // [C]
  uint16_t *const packed = reinterpret_cast<uint16_t *>(rad + C);   // [P], <true> only
  const ChainGeom geom = chain_geom(nb);   // nb <= 64: jp <= 64
  const int jp = geom.jp, groups = geom.groups;
  const int grp = lane / jp, body = lane - grp * jp;
  const bool active = body < nb;
  const int bj = active ? body : 0;   // (idle lanes read body 0's constants and never write)
  const DevModel *dm = a.dm;

  // the lane's body, once per launch
  const int par = bj > 0 ? col_clampi((int)a.parent[bj], nb - 1) : 0;
  const int depth = a.depth[bj];
  int maxd = active ? depth : 0;
  for (int off = 32; off; off >>= 1) { const int o = __shfl_xor(maxd, off); maxd = o > maxd ? o : maxd; }
  const bool hinge = active && bj > 0 && dm->jtype[bj] == GMR_JNT_HINGE;
  const bool root = active && bj == 0;
  const int qadr = hinge ? dm->qadr[bj] : 7;
  const double bpos[3] = {dm->bpos[3 * bj], dm->bpos[3 * bj + 1], dm->bpos[3 * bj + 2]};
  const double bquat[4] = {dm->bquat[4 * bj], dm->bquat[4 * bj + 1], dm->bquat[4 * bj + 2], dm->bquat[4 * bj + 3]};
  const double axis[3] = {dm->axis[3 * bj], dm->axis[3 * bj + 1], dm->axis[3 * bj + 2]};

  // the lane's capsules, once per launch; the radii (and the pair table) go to LDS
  double cp0[kColCapPasses][3], cp1[kColCapPasses][3];
  int cbody[kColCapPasses];
#pragma unroll
  for (int kk = 0; kk < kColCapPasses; ++kk) {
    const int ci = kFkWave * kk + lane;
    const int cc = ci < C ? ci : 0;
    cbody[kk] = col_clampi(a.cap_body[cc], nb - 1);
    for (int c = 0; c < 3; ++c) { cp0[kk][c] = a.cap_p0[3 * cc + c]; cp1[kk][c] = a.cap_p1[3 * cc + c]; }
    if (ci < C) rad[ci] = a.cap_radius[ci];
  }
  if (kPairsLds) {
    for (int p = lane; p < P; p += kFkWave)
      packed[p] = (uint16_t)(col_clampi(a.pairs[2 * p], C - 1) | (col_clampi(a.pairs[2 * p + 1], C - 1) << 8));
  }
  wave_lds_sync();

  const int64_t r0 = dyn_clamp(a.seq_offsets[blockIdx.x], 0, a.n_frames);
  const int64_t r1 = dyn_clamp(a.seq_offsets[blockIdx.x + 1], r0, a.n_frames);
  const int64_t T = r1 - r0;
  const int slot0 = grp * jp;   // the root's slot of this lane's frame
  const double inf = __longlong_as_double(0x7ff0000000000000ll), nan = __longlong_as_double(0x7ff8000000000000ll);

  for (int64_t k0 = (int64_t)blockIdx.y * groups; k0 < T; k0 += (int64_t)gridDim.y * groups) {
    // ---- 1: poses, LANE = BODY
    const int64_t k = k0 + grp;
    const bool live = active && k < T;
    const int64_t g = r0 + k;
    double th = 0.0, x[3] = {0.0, 0.0, 0.0}, r[4] = {1.0, 0.0, 0.0, 0.0};
    if (live && hinge) th = a.qpos[g * nq + qadr];
    if (live && root) {
      const double *row = a.qpos + g * nq;
      const double qn = sqrt(row[3] * row[3] + row[4] * row[4] + row[5] * row[5] + row[6] * row[6]);
      x[0] = row[0]; x[1] = row[1]; x[2] = row[2];
      r[0] = row[3] / qn; r[1] = row[4] / qn; r[2] = row[5] / qn; r[3] = row[6] / qn;
    }
    wave_lds_sync();   // (the previous pass no longer reads the buffers)
    for (int d = 0; d <= maxd; ++d) {
      if (live && depth == d) {
        if (d > 0) {
          const int ps = slot0 + par;
          const double xp[3] = {pose[0 * kFkWave + ps], pose[1 * kFkWave + ps], pose[2 * kFkWave + ps]};
          const double rp[4] = {pose[3 * kFkWave + ps], pose[4 * kFkWave + ps], pose[5 * kFkWave + ps], pose[6 * kFkWave + ps]};
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

    for (int gi = 0; gi < groups; ++gi) {
      const int64_t kf = k0 + gi;
      if (kf >= T) break;   // (wave-uniform)
      const int base = gi * jp;
      // ---- 2: world ends, LANE = CAPSULE
#pragma unroll
      for (int kk = 0; kk < kColCapPasses; ++kk) {
        const int ci = kFkWave * kk + lane;
        if (ci < C) {
          const int sl = base + cbody[kk];
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

      // ---- 3: the lane's pairs
      double best = inf;
      int bi = lane < P ? lane : 0x7fffffff, hits = 0;
      bool bad = false;
      for (int p = lane; p < P; p += kFkWave) {
        int ia, ib;
        if (kPairsLds) {
          const unsigned w = packed[p];
          ia = (int)(w & 0xffu); ib = (int)(w >> 8);
        } else {
          ia = col_clampi(a.pairs[2 * p], C - 1); ib = col_clampi(a.pairs[2 * p + 1], C - 1);
        }
        const double p1[3] = {ends[0 * C + ia], ends[1 * C + ia], ends[2 * C + ia]}, q1[3] = {ends[3 * C + ia], ends[4 * C + ia], ends[5 * C + ia]};
        const double p2[3] = {ends[0 * C + ib], ends[1 * C + ib], ends[2 * C + ib]}, q2[3] = {ends[3 * C + ib], ends[4 * C + ib], ends[5 * C + ib]};
        const double cl = col_segment_distance(p1, q1, p2, q2) - (rad[ia] + rad[ib]);
        bad = bad || cl != cl;
        if (cl < best) { best = cl; bi = p; }   // (ascending p: the first of equals stays)
        hits += cl < a.margin;
      }
      const bool any_bad = __ballot(bad) != 0;
      const double amin = wave_min(best);   // (no lane holds a NaN: those were flagged apart)
      const double imin = wave_min(best == amin ? (double)bi : 2147483647.0);
      const double hsum = wave_sum((double)hits);
      if (lane == 0) {
        const int64_t go = r0 + kf;
        if (a.clearance) a.clearance[go] = any_bad ? nan : amin;
        if (a.pair) a.pair[go] = any_bad ? -1 : (int32_t)imin;
        if (a.hits) a.hits[go] = any_bad ? 0 : (int32_t)hsum;
      }
      wave_lds_sync();   // (the next frame's ends overwrite these)
    }
  }
}

// ------------------------------------------------------------------ b: per clip
// grid (n_seq); lane = frame, tiles of 64
__global__ void __launch_bounds__(kFkWave) motion_self_collision_stats_kernel(const SelfCollisionArgs a) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int64_t r0 = dyn_clamp(a.seq_offsets[s], 0, a.n_frames);
  const int64_t r1 = dyn_clamp(a.seq_offsets[s + 1], r0, a.n_frames);
  const int64_t T = r1 - r0;
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  const u64 at_or_below = ~0ull >> (63 - lane);
  double best = inf;
  int bframe = 0x7fffffff, bpair = -1;
  int colliding = 0, nonfinite = 0, longest = 0, carry = 0;
  long long hsum = 0;
  for (int64_t k0 = 0; k0 < T; k0 += kFkWave) {
    const bool valid = k0 + lane < T;
    const int64_t g = r0 + k0 + lane;
    const double cl = valid ? a.clearance[g] : 0.0;
    const int h = valid ? a.hits[g] : 0;
    const int pr = valid ? a.pair[g] : -1;
    const bool isn = valid && cl != cl;
    if (valid && !isn && cl < best) { best = cl; bframe = (int)(k0 + lane); bpair = pr; }   // (ascending frames: the earliest of equals stays)
    const bool hit = valid && !isn && h > 0;
    const u64 m = __ballot(hit);
    colliding += __popcll(m);
    nonfinite += __popcll(__ballot(isn));
    hsum += h;
    // the run that ends in this lane: back to the highest clear bit at or below it, or through the tile's edge into the carry
    const u64 zeros = ~m & at_or_below;
    const int len = hit ? (zeros ? lane - (63 - __builtin_clzll(zeros)) : lane + 1 + carry) : 0;
    const int tmax = (int)wave_max((double)len);
    longest = tmax > longest ? tmax : longest;
    carry = __builtin_amdgcn_readlane(len, 63);
  }
  const double amin = wave_min(best);
  const double fmin_ = wave_min(best == amin ? (double)bframe : 2147483647.0);
  const u64 who = __ballot(best == amin && bframe != 0x7fffffff && (double)bframe == fmin_);
  const int wpair = __shfl(bpair, who ? (int)__builtin_ctzll(who) : 0);
  const double htot = wave_sum((double)hsum);
  if (lane == 0) {
    if (a.clearance_min) a.clearance_min[s] = who ? amin : inf;
    if (a.worst_frame) a.worst_frame[s] = who ? (int32_t)fmin_ : -1;
    if (a.worst_pair) a.worst_pair[s] = who ? wpair : -1;
    if (a.colliding) a.colliding[s] = colliding;
    if (a.longest_run) a.longest_run[s] = longest;
    if (a.hits_sum) a.hits_sum[s] = (int64_t)htot;
    if (a.nonfinite) a.nonfinite[s] = nonfinite;
  }
}

}  // namespace gmr

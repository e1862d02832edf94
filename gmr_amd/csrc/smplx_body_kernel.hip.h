// smplx_body_kernel.hip.h -- the joints of the SMPL-X body model, straight from AMASS parameters (float64).
//
// What load_smplx_file (reference general_motion_retargeting/utils/smpl.py:12-41) obtains from the `smplx` package for the first 55
// joints, without the 10 475 vertices the retargeter never reads: the rest joints are a linear function of the clip's betas
// (smplx_rest_kernel: J = J_template + J_dirs betas, the vertex sums folded away on the host once per model file), the posed joints
// a rigid chain over them (smplx_body_kernel: R_0 = exp(root_orient), p_0 = J_0, R_i = R_parent exp(pose_i),
// p_i = p_parent + R_parent (J_i - J_parent), then + trans).  Pose-corrective blend shapes move vertices only.
//
// One launch takes every clip of a batch: a wavefront owns a run of frames of ONE clip (found by a search over the clip table), lane =
// joint as in smplx_kernel.hip.h, with the same live-joint skeleton, the same exponential map (sincos_n / rotvec_to_quat_xyzw) and
// the same pointer-jumping products, so the rotation a joint's position was built with is bit for bit the orientation the adapter
// kernel later derives from full_pose.  Jaw, eyes and the 30 hand joints have the same local rotation in every frame (zero, and
// the model's mean hand pose): their quaternions are formed once per wavefront, before the frame loop.
#pragma once

#include "smplx_kernel.hip.h"

namespace gmr {

constexpr int kBodyJoints = 55;      // SMPL-X: pelvis + 21 body joints, jaw, two eyes, 2 x 15 hand joints
constexpr int kBodyPosed = 22;       // joints 0..21 read a rotation vector per frame (root_orient, pose_body)
constexpr int kBodyFirstHand = 25;   // joints 25..54: hands_meanl, hands_meanr

struct BodyClip {
  const void *root_orient, *pose_body, *trans;  // [n_frames][3], [n_frames][63], [n_frames][3], element types per dt[]
  const double *j_template, *j_dirs;            // the clip's model: [55][3], [55][3][dirs_stride]
  const double *hand_mean;                      // [90]: hands_meanl, hands_meanr
  const double *betas;                          // [n_betas] (in the launch's scratch block)
  double *rest;                                 // [55][3]: this clip's rest joints, written by smplx_rest_kernel
  int64_t row0, n_frames;                       // the clip's first row in the outputs
  int64_t blk0;                                 // its first workgroup
  int dt[3];                                    // 0: float32, 1: float64 (root_orient, pose_body, trans)
  int n_betas, dirs_stride, pad;
};

// rest[c][j][k] = j_template[j][k] + sum_l j_dirs[j][k][l] betas[l], one thread per coordinate, summed in the order of l
__global__ void __launch_bounds__(256) smplx_rest_kernel(const BodyClip *__restrict__ clips, int n_clips) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_clips * kBodyJoints * 3) return;
  const int c = i / (kBodyJoints * 3), e = i - c * (kBodyJoints * 3);
  const BodyClip &cl = clips[c];
  const double *d = cl.j_dirs + (size_t)e * cl.dirs_stride;
  double s = 0.0;
  for (int l = 0; l < cl.n_betas; ++l) s = fma(d[l], cl.betas[l], s);
  cl.rest[e] = cl.j_template[e] + s;
}

__device__ __forceinline__ double body_load(const void *p, int64_t i, int f64) {
  return f64 ? static_cast<const double *>(p)[i] : (double)static_cast<const float *>(p)[i];
}

// global_orient [N][3], full_pose [N][55][3], joints [N][55][3] (N = all clips' frames, clip c at rows row0_c ...): only the live
// joints of `sk` are written (sk.src, sk.parent; out_col is not used here -- every live joint's rows are what the adapter reads).
// A wavefront handles frames [chunk * (blockIdx.x - blk0), ...) of its clip, 64 / jp of them per iteration.
__global__ void __launch_bounds__(64) smplx_body_kernel(SmplSkeleton sk, const BodyClip *__restrict__ clips, int n_clips, int chunk,
                                                       double *__restrict__ global_orient, double *__restrict__ full_pose,
                                                       double *__restrict__ joints_out) {
  __shared__ double xb[7][64];
  __shared__ int xi[64];
  const int lane = threadIdx.x;
  const int J = sk.n_joints;
  const ChainGeom geo = chain_geom(J);
  const int jp = geo.jp, G = geo.groups;
  const int j = G > 1 ? (lane & (jp - 1)) : lane;
  const int grp = G > 1 ? lane / jp : 0;
  const bool has = j < J;
  const int par = has ? (int)sk.parent[j] : -1;
  const int jo = has ? (int)sk.src[j] : 0;
  int pslot[1] = {par >= 0 ? lane - j + par : -1};
  unsigned long long plan[1];
  const int rounds = chain_plan<1>(pslot, lane, xi, plan);

  // the clip of this workgroup: the last one whose first workgroup is not behind blockIdx.x (empty clips own no workgroup and
  // share their successor's blk0, so they are never the last of their equals ... unless they end the table, beyond every blockIdx)
  int lo = 0, hi = n_clips;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (clips[mid].blk0 <= (int64_t)blockIdx.x) lo = mid; else hi = mid;
  }
  const BodyClip cl = clips[lo];
  const int64_t f_begin = ((int64_t)blockIdx.x - cl.blk0) * chunk;
  const int64_t f_end = f_begin + chunk < cl.n_frames ? f_begin + chunk : cl.n_frames;

  // per lane, once: the offset from the parent's rest joint (the root: its own rest joint), and the local rotation of a joint no
  // frame changes
  const bool posed = jo < kBodyPosed;
  double d[3] = {0.0, 0.0, 0.0}, fixed_rv[3] = {0.0, 0.0, 0.0}, qf[4] = {0.0, 0.0, 0.0, 1.0};
  if (has) {
    const int pj = par >= 0 ? (int)sk.src[par] : -1;
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = cl.rest[jo * 3 + c] - (pj >= 0 ? cl.rest[pj * 3 + c] : 0.0);
    if (jo >= kBodyFirstHand) {
#pragma unroll
      for (int c = 0; c < 3; ++c) fixed_rv[c] = cl.hand_mean[(jo - kBodyFirstHand) * 3 + c];
    }
  }
  {
    const double a2 = fixed_rv[0] * fixed_rv[0] + fixed_rv[1] * fixed_rv[1] + fixed_rv[2] * fixed_rv[2], a = fast_sqrt(a2);
    const double h[1] = {0.5 * a};
    double sn[1], cs[1];
    sincos_n<1>(h, sn, cs);
    rotvec_to_quat_xyzw(fixed_rv, a2, a, sn[0], cs[0], qf);
  }

  struct Row { double rv[3], tr[3]; };
  auto load = [&](int64_t fb, Row &w) {
    const int64_t k = fb + grp;
#pragma unroll
    for (int c = 0; c < 3; ++c) { w.rv[c] = fixed_rv[c]; w.tr[c] = 0.0; }
    if (has && k < f_end) {
      if (posed) {
        const void *src = jo == 0 ? cl.root_orient : cl.pose_body;
        const int64_t at = jo == 0 ? k * 3 : k * 63 + (jo - 1) * 3;
        const int f64 = jo == 0 ? cl.dt[0] : cl.dt[1];
#pragma unroll
        for (int c = 0; c < 3; ++c) w.rv[c] = body_load(src, at + c, f64);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) w.tr[c] = body_load(cl.trans, k * 3 + c, cl.dt[2]);
    }
  };
  Row cur;
  load(f_begin, cur);
  for (int64_t fb = f_begin; fb < f_end; fb += G) {
    Row nxt;  // the next iteration's rows, requested before this one's arithmetic
    load(fb + G, nxt);

    double q[4] = {qf[0], qf[1], qf[2], qf[3]};  // xyzw
    if (__ballot(posed) != 0) {                   // (a live set without posed joints does not exist: the root is one; kept uniform)
      const double a2 = cur.rv[0] * cur.rv[0] + cur.rv[1] * cur.rv[1] + cur.rv[2] * cur.rv[2], a = fast_sqrt(a2);
      const double h[1] = {posed ? 0.5 * a : 0.0};  // lanes of fixed joints ride along on the short kernel's zero
      double sn[1], cs[1], qp[4];
      sincos_n<1>(h, sn, cs);
      rotvec_to_quat_xyzw(cur.rv, a2, a, sn[0], cs[0], qp);
      if (posed) { q[0] = qp[0]; q[1] = qp[1]; q[2] = qp[2]; q[3] = qp[3]; }
    }
    double p[3] = {d[0], d[1], d[2]};
    // pose relative to an ancestor, folded by pointer jumping: (q_a, p_a) o (q, p) = (q_a q, p_a + R(q_a) p)
    bool dirty = true;
#pragma unroll
    for (int r = 0; r < kChainMaxRounds; ++r) {
      if (r >= rounds) break;
      if (dirty) {
        xb[0][lane] = q[0]; xb[1][lane] = q[1]; xb[2][lane] = q[2]; xb[3][lane] = q[3];
        xb[4][lane] = p[0]; xb[5][lane] = p[1]; xb[6][lane] = p[2];
      }
      wave_lds_sync();
      const unsigned a = chain_anc(plan[0], r);
      dirty = a != kNoAnc;
      if (dirty) {
        const double aq[4] = {xb[0][a], xb[1][a], xb[2][a], xb[3][a]};
        const double aw[4] = {aq[3], aq[0], aq[1], aq[2]};
        double o[4], t[3];
        qrot(aw, p, t);
        quat_mul_xyzw(aq, q, o);
        p[0] = xb[4][a] + t[0]; p[1] = xb[5][a] + t[1]; p[2] = xb[6][a] + t[2];
        q[0] = o[0]; q[1] = o[1]; q[2] = o[2]; q[3] = o[3];
      }
      wave_lds_sync();
    }
    const int64_t k = fb + grp;
    if (has && k < f_end) {
      const int64_t row = cl.row0 + k;
      double *fp = full_pose + (row * kBodyJoints + jo) * 3, *jt = joints_out + (row * kBodyJoints + jo) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) { fp[c] = cur.rv[c]; jt[c] = p[c] + cur.tr[c]; }
      if (jo == 0) {
        double *go = global_orient + row * 3;
        go[0] = cur.rv[0]; go[1] = cur.rv[1]; go[2] = cur.rv[2];
      }
    }
    cur = nxt;
  }
}

}  // namespace gmr

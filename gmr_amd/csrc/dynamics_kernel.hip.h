// dynamics_kernel.hip.h -- floating-base inverse dynamics of retargeted qpos in float64, two launches (gmr_motion_dynamics; the
// definition is the contract above gmr_dynamics_input in include/gmr_amd.h).
//
//   a  motion_dynamics_kernel        grid (clip, wavefronts per clip: each strides over its clip's frame slots), one wavefront per
//                                    workgroup, LANE = BODY with tree_chain's geometry
//                                    (chain_geom): skeletons of up to 32 bodies put 64 / jp frames side by side, larger ones take one
//                                    frame per pass.  A lane keeps its body's constants in registers for the whole launch and reads
//                                    its own joint's coordinate at the frames of its stencil, so the differences are lane-local.
//                                    Down the tree level by level: pose, angular velocity and acceleration, linear acceleration of
//                                    the body origin, the parent's state read from the wavefront's exchange buffer in LDS.  Then every
//                                    lane leaves its body's wrench about the root's position (and m c for the centre of mass) in
//                                    LDS, and the lanes that own a joint add up their subtree.  The bodies are in depth-first
//                                    order (mjcf.py), so subtree(j) is the index range [j, end_j) and the sum runs over it in
//                                    ascending order: a fixed order, no recursion shared with the sweep down, no atomics.
//   b  motion_dynamics_stats_kernel  one wavefront per clip, lane = hinge, the clip's frames in order: maxima, counts, and the sum of
//                                    squares added frame by frame from 0.0.  Reads tau_out and root_wrench_out.
//
// Weaknesses, not engineered away: the sweep down costs one LDS round trip per tree level with most lanes idle (G1: 12 levels), the
// subtree sums leave every lane but the root's idle for most of their length, and stage b walks a clip serially.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fk_kernel.hip.h"   // kFkWave
#include "ik_kernel.hip.h"   // DevModel
#include "tree_chain.hip.h"  // chain_geom, wave_lds_sync

namespace gmr {

constexpr int kDynState = 16;   // doubles a body hands to its children: x(3) r(4) w(3) wd(3) a(3)
constexpr int kDynWrench = 9;   // doubles a body hands to its ancestors: F(3) N(3) m c(3)
constexpr int kDynLdsBytes = (kDynState + kDynWrench) * kFkWave * 8;
constexpr int kDynTargetWaves = 8192;   // wavefronts of one launch of kernel a that the host aims for (api.hip, dynamics_run)

struct DynamicsArgs {
  const DevModel *dm;            // the full body tree (gmr_evaluate's)
  const double *qpos, *qvel, *qacc;
  const int64_t *seq_offsets;
  int64_t n_frames;
  int n_seq, nbody, nq, nh;
  double dt, gx, gy, gz, gnorm, ground_z, fz_min;
  const int32_t *parent;
  const double *mass, *com, *inertia, *armature, *limit;
  double *tau, *wrench, *comw, *zmp, *qvel_out, *qacc_out;
  double *tau_abs_max, *tau_rms, *tau_ratio_max;
  int32_t *frames_over, *any_over;
  double *fz_max, *fz_min_out;
  int32_t *unloaded, *nonfinite;
};

__device__ __forceinline__ int64_t dyn_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// wxyz quaternion product, rotation of a vector and rotation by the conjugate, the contract's operation order (footlock's)
__device__ __forceinline__ void dyn_qmul(const double a[4], const double b[4], double o[4]) {
#pragma clang fp contract(off)
  o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}
__device__ __forceinline__ void dyn_rot_w(double qw, double qx, double qy, double qz, const double v[3], double o[3]) {
#pragma clang fp contract(off)
  const double tx = 2.0 * (qy * v[2] - qz * v[1]), ty = 2.0 * (qz * v[0] - qx * v[2]), tz = 2.0 * (qx * v[1] - qy * v[0]);
  o[0] = v[0] + qw * tx + (qy * tz - qz * ty);
  o[1] = v[1] + qw * ty + (qz * tx - qx * tz);
  o[2] = v[2] + qw * tz + (qx * ty - qy * tx);
}
__device__ __forceinline__ void dyn_rot(const double q[4], const double v[3], double o[3]) { dyn_rot_w(q[0], q[1], q[2], q[3], v, o); }
__device__ __forceinline__ void dyn_rot_inv(const double q[4], const double v[3], double o[3]) { dyn_rot_w(q[0], -q[1], -q[2], -q[3], v, o); }
__device__ __forceinline__ void dyn_cross(const double a[3], const double b[3], double o[3]) {
#pragma clang fp contract(off)
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// rotvec(p (x) conj(q)) / h for wxyz quaternions, the tracking export's formula: the world-frame angular velocity from q to p
__device__ __forceinline__ void dyn_ang_vel(const double p[4], const double q[4], double h, double o[3]) {
#pragma clang fp contract(off)
  double w = p[0] * q[0] + (p[1] * q[1] + p[2] * q[2] + p[3] * q[3]);
  double v[3] = {q[0] * p[1] - p[0] * q[1] - (p[2] * q[3] - p[3] * q[2]),
                 q[0] * p[2] - p[0] * q[2] - (p[3] * q[1] - p[1] * q[3]),
                 q[0] * p[3] - p[0] * q[3] - (p[1] * q[2] - p[2] * q[1])};
  if (w < 0.0) {
    w = -w;
    v[0] = -v[0]; v[1] = -v[1]; v[2] = -v[2];
  }
  const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  const double f = n > 1e-12 ? 2.0 * atan2(n, w) / n : 2.0;
  o[0] = v[0] * f / h; o[1] = v[1] * f / h; o[2] = v[2] * f / h;
}

// The stencils of frame k of a clip of T frames (rows `row0` .. of `q`, pitch nq): velocity over km .. kp, acceleration centred at kc.
struct DynStencil {
  const double *q;
  int64_t km, kp, kc;   // row indices (already offset by the clip's first row)
  double hv, dt;        // (kp - km) dt, 0 for a clip of one frame; dt
  bool acc;             // T >= 3
};
__device__ __forceinline__ DynStencil dyn_stencil(const double *qpos, int nq, int64_t r0, int64_t k, int64_t T, double dt) {
#pragma clang fp contract(off)
  DynStencil s;
  const int64_t km = k > 0 ? k - 1 : 0, kp = k + 1 < T ? k + 1 : T - 1;
  s.q = qpos;
  s.km = (r0 + km) * nq; s.kp = (r0 + kp) * nq;
  s.hv = (double)(kp - km) * dt; s.dt = dt;
  s.acc = T >= 3;
  const int64_t kc = k < 1 ? 1 : (k > T - 2 ? T - 2 : k);
  s.kc = (r0 + kc) * nq;   // read only when acc
  return s;
}
__device__ __forceinline__ void dyn_diff(const DynStencil &s, int col, int nq, double *v, double *a) {
#pragma clang fp contract(off)
  *v = s.hv > 0.0 ? (s.q[s.kp + col] - s.q[s.km + col]) / s.hv : 0.0;
  *a = s.acc ? ((s.q[s.kc + nq + col] - 2.0 * s.q[s.kc + col]) + s.q[s.kc - nq + col]) / (s.dt * s.dt) : 0.0;
}

// The sum of the masses in body order, the same in both kernels (the unloaded threshold must be)
__device__ __forceinline__ double dyn_total_mass(const double *mass, int nb) {
#pragma clang fp contract(off)
  double s = 0.0;
  for (int i = 0; i < nb; ++i) s = s + mass[i];
  return s;
}

// ------------------------------------------------------------------ a: per frame
// grid (n_seq, wavefronts per clip); static LDS: kDynLdsBytes + 64 bytes of parked arguments
__global__ void __launch_bounds__(kFkWave) motion_dynamics_kernel(const DynamicsArgs a) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double dyn_x[kDynState * kFkWave];
  __shared__ __attribute__((aligned(16))) double dyn_w[kDynWrench * kFkWave];
  // What a lane needs once per frame -- five output pointers and the three scalars of the root's lane -- waits in LDS instead of in
  // SGPRs that would stay live across the whole frame loop (the argument's 40 words do not all fit beside the loop's own state).
  __shared__ unsigned long long dyn_u[8];
  const int lane = threadIdx.x;
  const int nb = a.nbody, nq = a.nq, nv = a.nq - 1, nh = a.nh;
  const ChainGeom geom = chain_geom(nb);   // nb <= 64: jp <= 64
  const int jp = geom.jp, groups = geom.groups;
  const int grp = lane / jp, body = lane - grp * jp;
  const bool active = body < nb;
  const int bj = active ? body : 0;   // (idle lanes read body 0's constants and never write)
  const DevModel *dm = a.dm;

  // the lane's body, once per launch
  int par = a.parent[bj];
  par = par >= bj ? bj - 1 : (par < -1 ? -1 : par);   // depth-first order: a parent precedes its child (the host checked the model's)
  int depth = 0;
  for (int j = par; j >= 0; ) {
    ++depth;
    int pj = a.parent[j];
    j = pj >= j ? j - 1 : (pj < -1 ? -1 : pj);
  }
  int end = bj + 1;   // subtree(bj) = [bj, end): the run of later bodies whose parent is not in front of bj
  while (end < nb && a.parent[end] >= bj) ++end;
  int maxd = active ? depth : 0;
  for (int off = 32; off; off >>= 1) { const int o = __shfl_xor(maxd, off); maxd = o > maxd ? o : maxd; }
  const bool hinge = active && bj > 0 && dm->jtype[bj] == GMR_JNT_HINGE;
  const bool root = active && bj == 0;
  const int qadr = hinge ? dm->qadr[bj] : 7;
  const double bpos[3] = {dm->bpos[3 * bj], dm->bpos[3 * bj + 1], dm->bpos[3 * bj + 2]};
  const double bquat[4] = {dm->bquat[4 * bj], dm->bquat[4 * bj + 1], dm->bquat[4 * bj + 2], dm->bquat[4 * bj + 3]};
  const double axis[3] = {dm->axis[3 * bj], dm->axis[3 * bj + 1], dm->axis[3 * bj + 2]};
  const double mass = a.mass[bj];
  const double ipos[3] = {a.com[3 * bj], a.com[3 * bj + 1], a.com[3 * bj + 2]};
  const double Ixx = a.inertia[6 * bj], Iyy = a.inertia[6 * bj + 1], Izz = a.inertia[6 * bj + 2];
  const double Ixy = a.inertia[6 * bj + 3], Ixz = a.inertia[6 * bj + 4], Iyz = a.inertia[6 * bj + 5];
  const double arm = hinge ? a.armature[qadr - 7] : 0.0;
  const double mtot = dyn_total_mass(a.mass, nb);
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  if (lane == 0) {
    dyn_u[0] = (unsigned long long)a.wrench; dyn_u[1] = (unsigned long long)a.comw; dyn_u[2] = (unsigned long long)a.zmp;
    dyn_u[3] = (unsigned long long)__double_as_longlong(a.fz_min * (mtot * a.gnorm));
    dyn_u[4] = (unsigned long long)__double_as_longlong(mtot);
    dyn_u[5] = (unsigned long long)__double_as_longlong(a.ground_z);
    dyn_u[6] = (unsigned long long)a.qvel_out; dyn_u[7] = (unsigned long long)a.qacc_out;
  }
  wave_lds_sync();

  const int64_t r0 = dyn_clamp(a.seq_offsets[blockIdx.x], 0, a.n_frames);
  const int64_t r1 = dyn_clamp(a.seq_offsets[blockIdx.x + 1], r0, a.n_frames);
  const int64_t T = r1 - r0;
  const int slot0 = grp * jp;   // the root's slot of this lane's frame

  for (int64_t k0 = (int64_t)blockIdx.y * groups; k0 < T; k0 += (int64_t)gridDim.y * groups) {
    const int64_t k = k0 + grp;
    const bool live = active && k < T;
    const int64_t g = r0 + k;

    // the lane's own joint: coordinate, velocity, acceleration
    double th = 0.0, thd = 0.0, thdd = 0.0;
    double x[3] = {0.0, 0.0, 0.0}, r[4] = {1.0, 0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0}, wd[3] = {0.0, 0.0, 0.0}, acc[3] = {0.0, 0.0, 0.0};
    double v0[3] = {0.0, 0.0, 0.0};
    double *const o_qvel = (double *)dyn_u[6], *const o_qacc = (double *)dyn_u[7];
    if (live && hinge) {
      th = a.qpos[g * nq + qadr];
      if (a.qvel) thd = a.qvel[g * nv + qadr - 1];
      if (a.qacc) thdd = a.qacc[g * nv + qadr - 1];
      if (!a.qvel || !a.qacc) {
        const DynStencil s = dyn_stencil(a.qpos, nq, r0, k, T, a.dt);
        double dv, da;
        dyn_diff(s, qadr, nq, &dv, &da);
        if (!a.qvel) thd = dv;
        if (!a.qacc) thdd = da;
      }
      if (o_qvel) o_qvel[g * nv + qadr - 1] = thd;
      if (o_qacc) o_qacc[g * nv + qadr - 1] = thdd;
    }
    if (live && root) {
      const double *row = a.qpos + g * nq;
      const double qn = sqrt(row[3] * row[3] + row[4] * row[4] + row[5] * row[5] + row[6] * row[6]);
      x[0] = row[0]; x[1] = row[1]; x[2] = row[2];
      r[0] = row[3] / qn; r[1] = row[4] / qn; r[2] = row[5] / qn; r[3] = row[6] / qn;
      if (a.qvel) {
        const double *p = a.qvel + g * nv;
        v0[0] = p[0]; v0[1] = p[1]; v0[2] = p[2]; w[0] = p[3]; w[1] = p[4]; w[2] = p[5];
      }
      if (a.qacc) {
        const double *p = a.qacc + g * nv;
        acc[0] = p[0]; acc[1] = p[1]; acc[2] = p[2]; wd[0] = p[3]; wd[1] = p[4]; wd[2] = p[5];
      }
      if (!a.qvel || !a.qacc) {
        const DynStencil s = dyn_stencil(a.qpos, nq, r0, k, T, a.dt);
        for (int c = 0; c < 3; ++c) {
          double dv, da;
          dyn_diff(s, c, nq, &dv, &da);
          if (!a.qvel) v0[c] = dv;
          if (!a.qacc) acc[c] = da;
        }
        if (!a.qvel && s.hv > 0.0) {
          const double p[4] = {s.q[s.kp + 3], s.q[s.kp + 4], s.q[s.kp + 5], s.q[s.kp + 6]};
          const double q[4] = {s.q[s.km + 3], s.q[s.km + 4], s.q[s.km + 5], s.q[s.km + 6]};
          dyn_ang_vel(p, q, s.hv, w);
        }
        if (!a.qacc && s.acc) {
          const double qm[4] = {s.q[s.kc - nq + 3], s.q[s.kc - nq + 4], s.q[s.kc - nq + 5], s.q[s.kc - nq + 6]};
          const double qc[4] = {s.q[s.kc + 3], s.q[s.kc + 4], s.q[s.kc + 5], s.q[s.kc + 6]};
          const double qp[4] = {s.q[s.kc + nq + 3], s.q[s.kc + nq + 4], s.q[s.kc + nq + 5], s.q[s.kc + nq + 6]};
          double wp[3], wm[3];
          dyn_ang_vel(qp, qc, s.dt, wp);
          dyn_ang_vel(qc, qm, s.dt, wm);
          wd[0] = (wp[0] - wm[0]) / s.dt; wd[1] = (wp[1] - wm[1]) / s.dt; wd[2] = (wp[2] - wm[2]) / s.dt;
        }
      }
      if (o_qvel) {
        double *o = o_qvel + g * nv;
        o[0] = v0[0]; o[1] = v0[1]; o[2] = v0[2]; o[3] = w[0]; o[4] = w[1]; o[5] = w[2];
      }
      if (o_qacc) {
        double *o = o_qacc + g * nv;
        o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2]; o[3] = wd[0]; o[4] = wd[1]; o[5] = wd[2];
      }
    }

    // down the tree, level by level
    double ax_w[3] = {0.0, 0.0, 0.0};   // the hinge axis in the world
    wave_lds_sync();   // (the previous pass no longer reads the buffers)
    for (int d = 0; d <= maxd; ++d) {
      if (live && depth == d) {
        if (d > 0) {
          const int ps = slot0 + par;
          const double xp[3] = {dyn_x[0 * kFkWave + ps], dyn_x[1 * kFkWave + ps], dyn_x[2 * kFkWave + ps]};
          const double rp[4] = {dyn_x[3 * kFkWave + ps], dyn_x[4 * kFkWave + ps], dyn_x[5 * kFkWave + ps], dyn_x[6 * kFkWave + ps]};
          const double wp[3] = {dyn_x[7 * kFkWave + ps], dyn_x[8 * kFkWave + ps], dyn_x[9 * kFkWave + ps]};
          const double wdp[3] = {dyn_x[10 * kFkWave + ps], dyn_x[11 * kFkWave + ps], dyn_x[12 * kFkWave + ps]};
          const double ap[3] = {dyn_x[13 * kFkWave + ps], dyn_x[14 * kFkWave + ps], dyn_x[15 * kFkWave + ps]};
          double dd[3], t[4];
          dyn_rot(rp, bpos, dd);
          x[0] = xp[0] + dd[0]; x[1] = xp[1] + dd[1]; x[2] = xp[2] + dd[2];
          dyn_qmul(rp, bquat, t);
          w[0] = wp[0]; w[1] = wp[1]; w[2] = wp[2];
          wd[0] = wdp[0]; wd[1] = wdp[1]; wd[2] = wdp[2];
          if (hinge) {
            const double hh = 0.5 * th;
            const double sn = sin(hh), cs = cos(hh);
            const double jq[4] = {cs, sn * axis[0], sn * axis[1], sn * axis[2]};
            dyn_qmul(t, jq, r);
            dyn_rot(r, axis, ax_w);
            double wxa[3];
            dyn_cross(wp, ax_w, wxa);
            for (int c = 0; c < 3; ++c) {
              w[c] = wp[c] + ax_w[c] * thd;
              wd[c] = wdp[c] + ax_w[c] * thdd + wxa[c] * thd;
            }
          } else {
            r[0] = t[0]; r[1] = t[1]; r[2] = t[2]; r[3] = t[3];
          }
          double wdxd[3], wxd[3], wxwxd[3];
          dyn_cross(wdp, dd, wdxd);
          dyn_cross(wp, dd, wxd);
          dyn_cross(wp, wxd, wxwxd);
          acc[0] = ap[0] + wdxd[0] + wxwxd[0]; acc[1] = ap[1] + wdxd[1] + wxwxd[1]; acc[2] = ap[2] + wdxd[2] + wxwxd[2];
        }
        dyn_x[0 * kFkWave + lane] = x[0]; dyn_x[1 * kFkWave + lane] = x[1]; dyn_x[2 * kFkWave + lane] = x[2];
        dyn_x[3 * kFkWave + lane] = r[0]; dyn_x[4 * kFkWave + lane] = r[1]; dyn_x[5 * kFkWave + lane] = r[2]; dyn_x[6 * kFkWave + lane] = r[3];
        dyn_x[7 * kFkWave + lane] = w[0]; dyn_x[8 * kFkWave + lane] = w[1]; dyn_x[9 * kFkWave + lane] = w[2];
        dyn_x[10 * kFkWave + lane] = wd[0]; dyn_x[11 * kFkWave + lane] = wd[1]; dyn_x[12 * kFkWave + lane] = wd[2];
        dyn_x[13 * kFkWave + lane] = acc[0]; dyn_x[14 * kFkWave + lane] = acc[1]; dyn_x[15 * kFkWave + lane] = acc[2];
      }
      wave_lds_sync();
    }

    // the body's own wrench about the root's position, and m c
    const double x0[3] = {dyn_x[0 * kFkWave + slot0], dyn_x[1 * kFkWave + slot0], dyn_x[2 * kFkWave + slot0]};
    if (live) {
      double s[3], wds[3], ws[3], wws[3];
      dyn_rot(r, ipos, s);
      dyn_cross(wd, s, wds);
      dyn_cross(w, s, ws);
      dyn_cross(w, ws, wws);
      const double c[3] = {x[0] + s[0], x[1] + s[1], x[2] + s[2]};
      const double f[3] = {mass * ((acc[0] + wds[0] + wws[0]) - a.gx), mass * ((acc[1] + wds[1] + wws[1]) - a.gy),
                           mass * ((acc[2] + wds[2] + wws[2]) - a.gz)};
      double wb[3], wdb[3];
      dyn_rot_inv(r, w, wb);
      dyn_rot_inv(r, wd, wdb);
      const double Iw[3] = {Ixx * wb[0] + Ixy * wb[1] + Ixz * wb[2], Ixy * wb[0] + Iyy * wb[1] + Iyz * wb[2], Ixz * wb[0] + Iyz * wb[1] + Izz * wb[2]};
      const double Iwd[3] = {Ixx * wdb[0] + Ixy * wdb[1] + Ixz * wdb[2], Ixy * wdb[0] + Iyy * wdb[1] + Iyz * wdb[2],
                             Ixz * wdb[0] + Iyz * wdb[1] + Izz * wdb[2]};
      double gy[3], nb_[3], n[3], lev[3], cxf[3];
      dyn_cross(wb, Iw, gy);
      nb_[0] = Iwd[0] + gy[0]; nb_[1] = Iwd[1] + gy[1]; nb_[2] = Iwd[2] + gy[2];
      dyn_rot(r, nb_, n);
      lev[0] = c[0] - x0[0]; lev[1] = c[1] - x0[1]; lev[2] = c[2] - x0[2];
      dyn_cross(lev, f, cxf);
      dyn_w[0 * kFkWave + lane] = f[0]; dyn_w[1 * kFkWave + lane] = f[1]; dyn_w[2 * kFkWave + lane] = f[2];
      dyn_w[3 * kFkWave + lane] = n[0] + cxf[0]; dyn_w[4 * kFkWave + lane] = n[1] + cxf[1]; dyn_w[5 * kFkWave + lane] = n[2] + cxf[2];
      dyn_w[6 * kFkWave + lane] = mass * c[0]; dyn_w[7 * kFkWave + lane] = mass * c[1]; dyn_w[8 * kFkWave + lane] = mass * c[2];
    }
    wave_lds_sync();

    // the subtree sums, in body order, for the lanes that own a joint
    if (live && (hinge || root)) {
      double F[3] = {0.0, 0.0, 0.0}, N[3] = {0.0, 0.0, 0.0}, mc[3] = {0.0, 0.0, 0.0};
      for (int i = bj; i < end; ++i) {
        const int sl = slot0 + i;
        F[0] = F[0] + dyn_w[0 * kFkWave + sl]; F[1] = F[1] + dyn_w[1 * kFkWave + sl]; F[2] = F[2] + dyn_w[2 * kFkWave + sl];
        N[0] = N[0] + dyn_w[3 * kFkWave + sl]; N[1] = N[1] + dyn_w[4 * kFkWave + sl]; N[2] = N[2] + dyn_w[5 * kFkWave + sl];
        if (root) { mc[0] = mc[0] + dyn_w[6 * kFkWave + sl]; mc[1] = mc[1] + dyn_w[7 * kFkWave + sl]; mc[2] = mc[2] + dyn_w[8 * kFkWave + sl]; }
      }
      if (hinge) {
        if (a.tau) {
          const double lev[3] = {x[0] - x0[0], x[1] - x0[1], x[2] - x0[2]};
          double pxf[3];
          dyn_cross(lev, F, pxf);
          const double Wm[3] = {N[0] - pxf[0], N[1] - pxf[1], N[2] - pxf[2]};
          a.tau[g * nh + qadr - 7] = (ax_w[0] * Wm[0] + ax_w[1] * Wm[1] + ax_w[2] * Wm[2]) + arm * thdd;
        }
      } else {
        double *const o_wrench = (double *)dyn_u[0], *const o_com = (double *)dyn_u[1], *const o_zmp = (double *)dyn_u[2];
        if (o_wrench) {
          double *o = o_wrench + g * 6;
          o[0] = F[0]; o[1] = F[1]; o[2] = F[2]; o[3] = N[0]; o[4] = N[1]; o[5] = N[2];
        }
        if (o_com) {
          const double mt = __longlong_as_double((long long)dyn_u[4]);
          double *o = o_com + g * 3;
          o[0] = mc[0] / mt; o[1] = mc[1] / mt; o[2] = mc[2] / mt;
        }
        if (o_zmp) {
          const double thr = __longlong_as_double((long long)dyn_u[3]), gz0 = __longlong_as_double((long long)dyn_u[5]);
          double xf[3];
          dyn_cross(x0, F, xf);
          const double Mox = N[0] + xf[0], Moy = N[1] + xf[1];
          const bool unloaded = F[2] < thr;
          o_zmp[g * 2] = unloaded ? nan : (gz0 * F[0] - Moy) / F[2];
          o_zmp[g * 2 + 1] = unloaded ? nan : (Mox + gz0 * F[1]) / F[2];
        }
      }
    }
  }
}

// ------------------------------------------------------------------ b: per clip
// grid (n_seq); lane = hinge (nh <= 64)
__global__ void __launch_bounds__(kFkWave) motion_dynamics_stats_kernel(const DynamicsArgs a) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x, nh = a.nh;
  const bool mine = lane < nh;
  const int64_t s = blockIdx.x;
  const int64_t r0 = dyn_clamp(a.seq_offsets[s], 0, a.n_frames);
  const int64_t r1 = dyn_clamp(a.seq_offsets[s + 1], r0, a.n_frames);
  const double mtot = dyn_total_mass(a.mass, a.nbody);
  const double weight = mtot * a.gnorm, thr = a.fz_min * weight;
  const double lim = mine ? a.limit[lane] : __longlong_as_double(0x7ff0000000000000ll);
  double amax = 0.0, ss = 0.0, rmax = 0.0, fzmax = 0.0, fzmin = 0.0;
  int over = 0, any_over = 0, unloaded = 0, nonfinite = 0, finite = 0;
  for (int64_t g = r0; g < r1; ++g) {
    const double t = mine ? a.tau[g * nh + lane] : 0.0;
    const double *wr = a.wrench + g * 6;
    const double fz = wr[2];
    const bool bad = !__builtin_isfinite(t) || !__builtin_isfinite(wr[0]) || !__builtin_isfinite(wr[1]) || !__builtin_isfinite(fz) ||
                     !__builtin_isfinite(wr[3]) || !__builtin_isfinite(wr[4]) || !__builtin_isfinite(wr[5]);
    if (__ballot(bad) != 0) { ++nonfinite; continue; }   // a non-finite frame is counted and takes part in nothing else
    const double at = fabs(t), ratio = at / lim, fzr = fz / weight;
    amax = at > amax ? at : amax;
    rmax = ratio > rmax ? ratio : rmax;
    ss = ss + t * t;
    over += at > lim;
    any_over += __ballot(at > lim) != 0;
    fzmax = finite == 0 || fzr > fzmax ? fzr : fzmax;
    fzmin = finite == 0 || fzr < fzmin ? fzr : fzmin;
    unloaded += fz < thr;
    ++finite;
  }
  if (mine) {
    if (a.tau_abs_max) a.tau_abs_max[s * nh + lane] = amax;
    if (a.tau_rms) a.tau_rms[s * nh + lane] = finite > 0 ? sqrt(ss / (double)finite) : 0.0;
    if (a.tau_ratio_max) a.tau_ratio_max[s * nh + lane] = rmax;
    if (a.frames_over) a.frames_over[s * nh + lane] = over;
  }
  if (lane == 0) {
    if (a.any_over) a.any_over[s] = any_over;
    if (a.fz_max) a.fz_max[s] = fzmax;
    if (a.fz_min_out) a.fz_min_out[s] = fzmin;
    if (a.unloaded) a.unloaded[s] = unloaded;
    if (a.nonfinite) a.nonfinite[s] = nonfinite;
  }
}

}  // namespace gmr

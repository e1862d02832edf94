// slice_plan.h -- which frames round r of a sliced IK launch covers (ik_kernel_sliced, "Slices" in DESIGN 4.2).
//
// Plain C++17, host and device, no HIP include: the kernel, the host (api.hip) and a stand-alone host test share these functions.
//
// T = frames of the longest item, L = the slice length (gmr_ik_balance_plan), f = the taper floor.  Round r covers frames
// [slice_begin(r), slice_end(r)) of every item, clipped to the item's length.
//   - uniform (f == 0, ceil(L / 2) < f or T <= L): begin(r) = r L, max(1, ceil(T / L)) rounds;
//   - tapered: the last L frames of the longest item, from tb = T - L, are cut into ever shorter slices -- each takes the larger half
//     of what is left of the L frames while that half is still >= f, then one closing slice takes the rest (slice_taper_cut):
//     L = 256, f = 32 -> 128 64 32 32;  L = 7, f = 1 -> 4 2 1;  L = 64, f = 32 -> 32 32;  L = 16, f = 1 -> 8 4 2 1 1.
//     (For a power of two L every piece is half the one before it.  Halving what is left, not the piece before, keeps the last slice
//     under 2 f for every L: 5 frames at f = 1 are cut 3 1 1, not 3 2.)  Frames [0, tb) are cut from 0 in slices of L; the ragged
//     piece, shorter than L, sits directly in front of the taper.  T = 3000, L = 256, f = 16: 10 x 256, 184, 128, 64, 32, 16, 16.
// The taper shortens the tail of the last round, in which wavefront slots stand idle once the tickets have run out, without
// paying the per-slice set-up more often over the whole clip.
//
// SlicePlan is the form the kernel reads (it travels in the kernarg segment): the body rounds are arithmetic -- a forced L = 1 launch has
// thousands of them -- and only the taper, at most kSliceTaperMax slices, is a table.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GMR_SP_HD __host__ __device__
#else
#define GMR_SP_HD
#endif

namespace gmr {

constexpr int kSliceTaperMax = 32;  // L < 2^31 halves to nothing in 31 steps
constexpr int kSliceNever = 0x7fffffff;  // begin / end of a round past the plan's last: behind every item's end

struct SlicePlan {
  int slice_len;                  // L
  int t_body;                     // the body rounds cover [0, t_body): tb when tapered, else T
  int n_body;                     // body rounds: ceil(t_body / L), at least 1
  int n_taper;                    // taper rounds, 0 = uniform
  int taper_end[kSliceTaperMax];  // taper round j covers [j ? taper_end[j - 1] : t_body, taper_end[j])
};

GMR_SP_HD inline bool slice_plan_tapers(int T, int L, int f) { return f > 0 && L / 2 + (L & 1) >= f && T > L; }

// The taper's slice lengths, in order, into len[kSliceTaperMax]; returns their number.  They add up to L and never grow.
GMR_SP_HD inline int slice_taper_cut(int L, int f, int *len) {
  int n = 0, left = L;
  while (n < kSliceTaperMax - 1) {
    const int h = left / 2 + (left & 1);
    if (h < f || h == 0) break;
    len[n++] = h;
    left -= h;
  }
  if (left > 0) len[n++] = left;
  return n;
}

// T >= 0, L >= 1, f >= 0.
GMR_SP_HD inline SlicePlan slice_plan_make(int T, int L, int f) {
  SlicePlan P{};
  P.slice_len = L;
  if (!slice_plan_tapers(T, L, f)) {
    P.t_body = T > 0 ? T : 0;
    P.n_body = T > L ? (int)(((long long)T + L - 1) / L) : 1;
    return P;
  }
  P.t_body = T - L;
  P.n_body = (int)(((long long)P.t_body + L - 1) / L);
  int len[kSliceTaperMax];
  P.n_taper = slice_taper_cut(L, f, len);
  for (int j = 0, e = P.t_body; j < P.n_taper; ++j) P.taper_end[j] = e += len[j];
  return P;
}

template <class Plan>  // (a template: the kernel reads the plan through a constant-address-space pointer)
GMR_SP_HD inline int slice_plan_rounds(const Plan &P) { return P.n_body + P.n_taper; }

// First frame of round r >= 0, and one past its last.  A round past the plan's last starts behind every item's end; no index leaves
// taper_end whatever r is.
template <class Plan>
GMR_SP_HD inline int slice_begin(const Plan &P, int r) {
  const int j = r - P.n_body;
  if (j < 0) return r * P.slice_len;  // (< t_body: fits)
  if (j == 0) return P.n_taper > 0 ? P.t_body : kSliceNever;
  return j < P.n_taper ? P.taper_end[j - 1] : kSliceNever;
}
template <class Plan>
GMR_SP_HD inline int slice_end(const Plan &P, int r) {
  const int j = r - P.n_body;
  if (j < 0) {
    const long long e = ((long long)r + 1) * P.slice_len;
    return e < P.t_body ? (int)e : P.t_body;
  }
  return j < P.n_taper ? P.taper_end[j] : kSliceNever;
}

// The same schedule as a walk along the longest item: the strictly rising boundaries 0 = b[0] < .. < b[rounds] = T (T = 0: one empty
// round, b = {0, 0}).  Writes at most `cap` entries and returns the number of rounds.
GMR_SP_HD inline int slice_boundaries(int T, int L, int f, int *b, int cap) {
  int n = 0, at = 0;
  if (n < cap) b[n] = 0;
  const bool taper = slice_plan_tapers(T, L, f);
  const int tb = taper ? T - L : T;
  do {  // (at least one round)
    at = tb - at > L ? at + L : tb;
    if (++n < cap) b[n] = at;
  } while (at < tb);
  if (taper) {
    int len[kSliceTaperMax];
    const int nt = slice_taper_cut(L, f, len);
    for (int j = 0; j < nt; ++j) {
      at += len[j];
      if (++n < cap) b[n] = at;
    }
  }
  return n;
}

}  // namespace gmr

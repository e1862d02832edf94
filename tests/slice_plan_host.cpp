// Stand-alone check of gmr_amd/csrc/slice_plan.h (tests/test_ik_slice_plan_host.py builds it with the host compiler under
// AddressSanitizer and UBSan and runs it; nothing is loaded into Python).  Every T in 1..600, L in 1..70 and 256, f in 0..40.
//   slice_plan_host           the sweep; prints "ok <schedules> <tapered> <item lengths>"
//   slice_plan_host T L f     prints the round count and the slice lengths of one schedule
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "slice_plan.h"

using namespace gmr;

static int gT, gL, gF, gR, gN;
#define CHECK(c)                                                                                                \
  do {                                                                                                          \
    if (!(c)) {                                                                                                 \
      fprintf(stderr, "line %d: %s (T %d L %d f %d round %d item length %d)\n", __LINE__, #c, gT, gL, gF, gR, gN); \
      exit(1);                                                                                                  \
    }                                                                                                           \
  } while (0)

static int ceil_div(int a, int b) { return (a + b - 1) / b; }

// What the kernel does with a ticket of round r of an item of n frames (ik_sliced_item, ik_body): false = leaves at once.
static bool ticket(const SlicePlan &P, int r, int n, int &kf0, int &kend) {
  if (r > 0 && slice_begin(P, r) >= n) return false;
  kf0 = slice_begin(P, r);
  kend = slice_end(P, r) < n ? slice_end(P, r) : n;
  return true;
}

static void expect_cut(int L, int f, std::vector<int> want) {
  int len[kSliceTaperMax];
  gT = 0, gL = L, gF = f;
  const int n = slice_taper_cut(L, f, len);
  CHECK(n == (int)want.size());
  for (int j = 0; j < n; ++j) CHECK(len[j] == want[j]);
}

int main(int argc, char **argv) {
  if (argc == 4) {
    const int T = atoi(argv[1]), L = atoi(argv[2]), f = atoi(argv[3]);
    if (T < 0 || L < 1 || f < 0) return 2;
    const SlicePlan P = slice_plan_make(T, L, f);
    printf("%d", slice_plan_rounds(P));
    for (int r = 0; r < slice_plan_rounds(P); ++r) printf(" %d", slice_end(P, r) - slice_begin(P, r));
    printf("\n");
    return 0;
  }
  static_assert(sizeof(SlicePlan) % 8 == 0, "SlicePlan closes IkSliceArgs, whose alignment is 8");
  // the worked examples
  expect_cut(256, 32, {128, 64, 32, 32});
  expect_cut(7, 1, {4, 2, 1});
  expect_cut(64, 32, {32, 32});
  expect_cut(16, 1, {8, 4, 2, 1, 1});
  expect_cut(16, 4, {8, 4, 4});
  {
    gT = 3000, gL = 256, gF = 32;
    const SlicePlan P = slice_plan_make(3000, 256, 32);
    const int want[15] = {256, 256, 256, 256, 256, 256, 256, 256, 256, 256, 184, 128, 64, 32, 32};
    CHECK(slice_plan_rounds(P) == 15);
    for (gR = 0; gR < 15; ++gR) CHECK(slice_end(P, gR) - slice_begin(P, gR) == want[gR]);
    CHECK(slice_plan_rounds(slice_plan_make(3000, 256, 0)) == 12);
  }
  {  // the longest slice length an int holds: the taper table does not overflow
    int len[kSliceTaperMax];
    gT = 0, gL = 0x7fffffff, gF = 1;
    const int n = slice_taper_cut(0x7fffffff, 1, len);
    long long sum = 0;
    for (int j = 0; j < n; ++j) sum += len[j];
    CHECK(n <= kSliceTaperMax && sum == 0x7fffffff);
  }

  long schedules = 0, tapered = 0, lengths = 0;
  std::vector<int> Ls;
  for (int L = 1; L <= 70; ++L) Ls.push_back(L);
  Ls.push_back(256);
  std::vector<int> b(602), owner(600);
  std::vector<SlicePlan> checked;  // the plans of this (T, L) whose item lengths are done
  for (int T = 1; T <= 600; ++T)
    for (int L : Ls)
      for (int f = 0; f <= 40; ++f) {
        if (f == 0) checked.clear();
        gT = T, gL = L, gF = f, gR = -1, gN = -1;
        ++schedules;
        const bool uniform = f == 0 || ceil_div(L, 2) < f || T <= L;
        CHECK(uniform == !slice_plan_tapers(T, L, f));
        const int rounds = slice_boundaries(T, L, f, b.data(), (int)b.size());
        CHECK(rounds >= 1 && rounds <= T);
        // 1. boundaries rise strictly from 0 to T, no slice longer than L
        CHECK(b[0] == 0 && b[rounds] == T);
        for (gR = 0; gR < rounds; ++gR) CHECK(b[gR] < b[gR + 1] && b[gR + 1] - b[gR] <= L);
        if (uniform) {  // 2. the parent's schedule
          CHECK(rounds == ceil_div(T, L));
          for (gR = 0; gR < rounds; ++gR) CHECK(b[gR] == gR * L);
        } else {  // 3. the taper
          ++tapered;
          const int tb = T - L;
          int first = 0;  // the taper's first round
          while (b[first] < tb) ++first;
          gR = first;
          CHECK(b[first] == tb && first == ceil_div(tb, L));
          for (gR = 0; gR + 1 < first; ++gR) CHECK(b[gR + 1] - b[gR] == L);  // the ragged piece directly in front of the taper
          CHECK(b[rounds] - b[rounds - 1] < 2 * f);
          CHECK(b[first + 1] - b[first] == ceil_div(L, 2));
          for (gR = first + 1; gR < rounds; ++gR) CHECK(b[gR + 1] - b[gR] <= b[gR] - b[gR - 1]);
          for (gR = first; gR + 1 < rounds; ++gR) CHECK(b[gR + 1] - b[gR] >= f);  // only the closing slice may be under the floor
          int lg = 0;  // ceil(log2(L / f))
          while (((long long)f << lg) < L) ++lg;
          CHECK(rounds <= ceil_div(T, L) + lg + 2);
        }
        // 4. the device form
        const SlicePlan P = slice_plan_make(T, L, f);
        CHECK(slice_plan_rounds(P) == rounds && P.n_body >= 1 && P.n_taper >= 0 && P.n_taper <= kSliceTaperMax && P.slice_len == L);
        CHECK(uniform == (P.n_taper == 0));
        for (gR = 0; gR < rounds; ++gR) CHECK(slice_begin(P, gR) == b[gR] && slice_end(P, gR) == b[gR + 1]);
        for (gR = rounds; gR < rounds + 3; ++gR) CHECK(slice_begin(P, gR) >= T && slice_end(P, gR) >= T);  // past the plan: behind every end
        // 5. every item length n <= T, once per distinct plan of this (T, L): many floors give the same cut.
        // owner[k]: the round whose slice holds frame k of the longest item (each frame once).
        bool seen = false;
        for (const SlicePlan &Q : checked) seen = seen || memcmp(&Q, &P, sizeof P) == 0;
        if (seen) continue;
        checked.push_back(P);
        for (int k = 0; k < T; ++k) owner[k] = -1;
        for (gR = 0; gR < rounds; ++gR)
          for (int k = slice_begin(P, gR); k < slice_end(P, gR); ++k) {
            CHECK(k >= 0 && k < T && owner[k] < 0);
            owner[k] = gR;
          }
        for (gN = 1; gN <= T; ++gN) {
          ++lengths;
          int kf0 = 0, kend = 0;
          const int last = owner[gN - 1];  // the one slice that ends the item ...
          gR = last;
          CHECK(last >= 0 && ticket(P, last, gN, kf0, kend) && kf0 < gN && kend == gN);
          if (last > 0) {  // ... behind a slice that hands over at the frame this one starts from ...
            int p0 = 0, pend = 0;
            CHECK(ticket(P, last - 1, gN, p0, pend) && pend == kf0 && pend < gN);
          }
          if (last + 1 < rounds) CHECK(!ticket(P, last + 1, gN, kf0, kend));  // ... and in front of tickets that leave at once
          if (T <= 40) {  // the same from every ticket of the grid, as the kernel sees them
            int at = 0, enders = 0;
            for (gR = 0; gR < rounds; ++gR) {
              if (!ticket(P, gR, gN, kf0, kend)) {
                CHECK(gR > last && slice_begin(P, gR) >= gN);
                continue;
              }
              CHECK(gR <= last && kf0 == at && kend > kf0 && kend <= gN);
              at = kend;
              enders += kend == gN;
            }
            CHECK(at == gN && enders == 1);
          }
        }
        {  // an empty item: round 0 runs over no frames and ends the item, every other ticket leaves
          int kf0 = -1, kend = -1;
          gN = 0;
          CHECK(ticket(P, 0, 0, kf0, kend) && kf0 == 0 && kend == 0);
          for (gR = 1; gR < rounds; ++gR) CHECK(!ticket(P, gR, 0, kf0, kend));
        }
      }
  printf("ok %ld %ld %ld\n", schedules, tapered, lengths);
  return 0;
}

// model_plan_host.cpp -- gmr_amd/csrc/model_plan.h without a GPU and without Python: a stand-alone program (tests/test_model_plan_host.py
// builds it with the host compiler under AddressSanitizer and UBSan; tools/record_model_plan.py builds it plain).
//
//   model_plan_host MANIFEST      one line per case: <blob file> <min_nvp> <force_generic> <dump file or ->
//   model_plan_host --too-many-passes
//
// Per case it plans the blob and prints one line
//   <code>|<message>|<shape index>|<instance name>|<the 15 GMR_IK_SHAPE_FIELDS, comma separated>
// A case that plans is then checked against what the kernels assume of the tables (CHECK: the program exits 1 at the first
// violation) and, with a dump file, dumped: every section as "<name> <offset in the image> <bytes>\n" + the bytes + "\n".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <set>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "model_plan.h"

using namespace gmr;

static const char *g_case = "";
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s: line %d: %s\n", g_case, __LINE__, #c); exit(1); } } while (0)

// ---------------------------------------------------------------------------------------------------------------- dump
static void section(FILE *f, const char *name, size_t at, const void *p, size_t bytes) {
  fprintf(f, "%s %zu %zu\n", name, at, bytes);
  if (bytes) fwrite(p, 1, bytes, f);
  fputc('\n', f);
}
template <class T>
static void table(FILE *f, const char *name, ModelImage &I, CallBlock::Uploaded<T> h) {
  CHECK(h.at + h.n * sizeof(T) <= I.block.uploaded_bytes());
  section(f, name, h.at, I.block[h], h.n * sizeof(T));
}
static void dump(const char *path, ModelPlan &p) {
  FILE *f = fopen(path, "wb");
  CHECK(f != nullptr);
  ModelImage &I = p.image;
  section(f, "dm", 0, &p.dm, sizeof(p.dm));
  section(f, "dm_eval", 0, &p.dm_eval, sizeof(p.dm_eval));
  section(f, "lay", 0, &p.lay, sizeof(p.lay));
  section(f, "lay_eval", 0, &p.lay_eval, sizeof(p.lay_eval));
  const int32_t scalars[12] = {p.lds_bytes, p.lds_bytes_eval, p.nvp, p.n_act, p.shape, p.fk_lds_bytes, p.fk_lds_bytes_min, p.nslots,
                               p.dof_in_order, p.k_maxd, (int32_t)I.block.uploaded_bytes(), (int32_t)I.block.total_bytes()};
  section(f, "scalars", 0, scalars, sizeof(scalars));
  table(f, "image.dm", I, I.dm); table(f, "image.dm_eval", I, I.dm_eval);
  table(f, "parent", I, I.parent); table(f, "dofidx", I, I.dofidx); table(f, "src_slot", I, I.src_slot); table(f, "save_slot", I, I.save_slot);
  table(f, "lpos", I, I.lpos); table(f, "lrot", I, I.lrot); table(f, "jaxis", I, I.jaxis); table(f, "jaxis64", I, I.jaxis64);
  table(f, "fkbody", I, I.fkbody);
  table(f, "k_dof_body", I, I.k_dof_body); table(f, "k_lo", I, I.k_lo); table(f, "k_hi", I, I.k_hi);
  table(f, "k_depth", I, I.k_depth); table(f, "k_order", I, I.k_order);
  table(f, "rep_lo", I, I.rep_lo); table(f, "rep_hi", I, I.rep_hi);
  section(f, "image", 0, I.block.image(), I.block.uploaded_bytes());
  CHECK(fclose(f) == 0);
}

// ---------------------------------------------------------------------------------------------------------------- invariants
static void check_order(const PlanStages &s) {
  const ActiveDofs &A = s.act;
  CHECK(A.n_act >= 6 && A.n_act <= 64 && A.n_act <= A.nvp);
  for (int k = 0; k < 6; ++k) CHECK(A.body[k] == 0 && (A.kind[k] == k || A.kind[k] == 7));  // the root's six dofs lead the order
  for (int a = 6; a < A.n_act; ++a) CHECK(A.kind[a] == 6 && A.body[a] > 0);
  for (int a = 0; a < 64; ++a) {
    CHECK(a == 0 ? s.order.aanc[a] == 0 : (s.order.aanc[a] >> a) == 0);  // only bits below a
    if (a >= A.n_act) CHECK(s.order.aanc[a] == 0);
  }
  for (int a = 1; a < A.n_act; ++a) CHECK(A.height[a] <= A.height[a - 1]);
}

static void check_hplan(const PlanStages &s, const ModelPlan &p) {
  const LdsLayout &L = p.lay;
  const size_t npairs = s.order.hpair.size();
  const int ne = (int)s.hplan.size() / 2;
  CHECK(s.hplan.size() == s.hplan_pairs.size() && ne % 128 == 0 && ne == p.dm.npairp && (size_t)ne >= npairs && (size_t)ne < npairs + 128);
  CHECK(ne <= kMaxPairsPadded);
  typedef std::pair<uint32_t, uint32_t> E;
  std::vector<E> a, b;
  for (int i = 0; i < ne; ++i) { a.push_back(E(s.hplan_pairs[2 * i], s.hplan_pairs[2 * i + 1])); b.push_back(E(s.hplan[2 * i], s.hplan[2 * i + 1])); }
  for (int i = 0; i < ne; ++i) CHECK(p.dm.hplan[i].x == b[i].first && p.dm.hplan[i].y == b[i].second);
  std::sort(a.begin(), a.end()); std::sort(b.begin(), b.end());
  CHECK(a == b);  // the ordered plan is a permutation of the pairs plus padding
  const int hsize = s.use_sq ? 1024 : p.nvp * p.nvp;
  const E pad(E((uint32_t)(L.S * 8) | ((uint32_t)(L.F * 8) << 16), (uint32_t)((L.H + hsize) * 8) | ((uint32_t)((L.H + hsize + 1) * 8) << 16)));
  CHECK((L.H + hsize + 2) * 8 <= L.cplan * 8 && L.cplan * 8 <= 65535);  // the two dummy slots lie inside the H region
  std::set<uint32_t> reads, writes;
  size_t npad = 0;
  for (int i = 0; i < ne; ++i) {
    if (b[i] == pad) { ++npad; continue; }
    const int so = (int)(b[i].first & 0xffffu), fo = (int)(b[i].first >> 16), d0 = (int)(b[i].second & 0xffffu), d1 = (int)(b[i].second >> 16);
    CHECK(so % 48 == (L.S * 8) % 48 && so >= L.S * 8 && so + 48 <= (L.S + 6 * p.n_act) * 8);
    CHECK(fo % 48 == (L.F * 8) % 48 && fo >= L.F * 8 + 48 && fo + 48 <= (L.F + 6 * p.n_act) * 8);
    CHECK(d0 % 8 == 0 && d1 % 8 == 0 && d0 >= L.H * 8 && d0 < (L.H + hsize) * 8 && d1 >= L.H * 8 && d1 < (L.H + hsize) * 8);
    CHECK(reads.insert(b[i].first).second);                                // each real pair appears once
    CHECK(writes.insert(d0).second && writes.insert(d1).second);           // and no entry of H is written twice
  }
  CHECK(npad == (size_t)ne - npairs && reads.size() == npairs);
  for (int i = 0; i < p.n_act; ++i) {  // ... nor is a diagonal entry
    const int diag = s.use_sq ? s.sq.diag[i] : i * p.nvp + i;
    CHECK(diag >= 0 && diag < hsize && !writes.count((uint32_t)((L.H + diag) * 8)));
  }
  for (size_t q = 0; q < npairs; ++q) {  // the pair order is (i, j) with j above i
    const int i = s.order.hpair[q] >> 8, j = s.order.hpair[q] & 0xff;
    CHECK(j < i && i < p.n_act && ((s.order.aanc[i] >> j) & 1ull));
    CHECK((s.hplan_pairs[2 * q] & 0xffffu) == (uint32_t)((L.S + 6 * j) * 8) && (s.hplan_pairs[2 * q] >> 16) == (uint32_t)((L.F + 6 * i) * 8));
  }
}

static void check_composite_plan(const PlanStages &s, const ModelPlan &p) {
  const LdsLayout &L = p.lay;
  const gmr_blob_header &h = s.blob.h;
  const int ntmax = std::max(h.ntask[0], h.ntask[1]);
  const int zoff = L.zero * 8, foff = L.F * 8, boff = L.B * 8, coff = L.Bc * 8, blk = kBT * 8;
  for (int k = 0; k < 2; ++k) {
    const int np = s.passes.ncpass[k], nc = s.comp.ncomp[k];
    CHECK(np >= 0 && np <= kMaxCompPass && np == p.dm.ncpass[k] && nc == p.dm.ncomp[k]);
    std::vector<std::vector<int>> written(nc);  // per composite: the passes that write it
    std::vector<int> src[kMaxCompPass][4];
    int dst[kMaxCompPass][4];
    for (auto &row : dst) for (int &d : row) d = -1;
    for (int pass = 0; pass < kMaxCompPass; ++pass)
      for (int q = 0; q < 4; ++q) {
        const uint32_t *row = s.passes.plan.data() + ((size_t)(k * kMaxCompPass + pass) * 4 + q) * 4;
        const uint4 &dev = p.dm.comp_plan[(k * kMaxCompPass + pass) * 4 + q];
        CHECK(dev.x == row[0] && dev.y == row[1] && dev.z == row[2] && dev.w == row[3]);
        if (pass >= np) { CHECK(row[0] == 0 && row[1] == 0 && row[2] == 0 && row[3] == 0); continue; }
        const int so[4] = {(int)(row[0] & 0xffffu), (int)(row[0] >> 16), (int)(row[1] & 0xffffu), (int)(row[1] >> 16)};
        CHECK(row[2] <= 0xffffu && row[3] == 0);
        dst[pass][q] = -1;
        int nsrc = 0;
        for (int j = 0; j < 4; ++j) {
          CHECK(so[j] + blk <= p.lds_bytes);
          if (so[j] == zoff) { src[pass][q].push_back(-1); continue; }  // an absent source reads the zero block
          ++nsrc;
          if (so[j] >= coff) {
            CHECK((so[j] - coff) % blk == 0 && (so[j] - coff) / blk < nc);
            src[pass][q].push_back(64 + (so[j] - coff) / blk);
          } else {
            CHECK(so[j] >= boff && (so[j] - boff) % blk == 0 && (so[j] - boff) / blk < h.ntask[k]);
            src[pass][q].push_back((so[j] - boff) / blk);
          }
        }
        const int d = (int)row[2];
        CHECK(d + blk <= p.lds_bytes);
        if (nsrc == 0 && d == foff) continue;  // an idle quarter writes to F
        CHECK(d >= coff && (d - coff) % blk == 0 && (d - coff) / blk < nc);
        if (nsrc == 0) CHECK(s.comp.mask[k * 2 * GMR_MAX_TASKS + (d - coff) / blk] == 0);  // the composite of no task: a block of zeros
        dst[pass][q] = (d - coff) / blk;
        for (int q2 = 0; q2 < q; ++q2) CHECK(dst[pass][q2] != dst[pass][q]);
        written[dst[pass][q]].push_back(pass);
      }
    for (int pass = 0; pass < np; ++pass)
      for (int q = 0; q < 4; ++q)
        for (int sidx : src[pass][q]) {
          if (sidx < 64) continue;
          const std::vector<int> &w = written[sidx - 64];
          CHECK(!w.empty() && w.front() < pass);  // written before it is read
          // a composite that another one reads is complete: no write in the same or a later pass (an entry that carries on
          // its own sum reads what an earlier pass left)
          if (sidx - 64 != dst[pass][q]) CHECK(w.back() < pass);
        }
    // a dof's block: a task block or a composite that some pass writes, inside [B, cplan)
    for (int i = 0; i < p.n_act; ++i) {
      const int b = p.dm.acomp[k * 64 + i];
      CHECK(b >= 0 && (L.B + kBT * (b + 1)) <= L.cplan);
      if (b < ntmax) CHECK(b < h.ntask[k]);
      else CHECK(b - ntmax < nc && !written[b - ntmax].empty());
    }
  }
}

static void check_structured_qp(const PlanStages &s) {
  const StructuredQp &Q = s.sq;
  const int n_act = s.act.n_act;
  if (!Q.ok) return;
  const int nl = Q.nlimb;
  CHECK(nl >= 6 && nl <= 15);
  std::vector<int> owners(n_act, 0);
  for (int L = 0; L < 64; ++L) {
    const int i = Q.gdof[L];
    CHECK(i >= -1 && i < n_act);
    if (i < 0) { CHECK(Q.owner[L] == 0); continue; }
    if (Q.owner[L]) { ++owners[i]; CHECK(Q.lane_of_dof[i] == L); }
  }
  for (int i = 0; i < n_act; ++i) CHECK(owners[i] == 1);  // each active dof is owned by exactly one lane
  std::vector<char> in_core(n_act, 0);
  for (int r = nl; r < 16; ++r) {  // core copies sit at rows nlimb .. 15 of every group
    const int c = Q.gdof[r];
    CHECK(c >= 0 && !in_core[c]);
    in_core[c] = 1;
    for (int g = 0; g < 4; ++g) CHECK(Q.gdof[16 * g + r] == c && Q.owner[16 * g + r] == (g == 0));
  }
  for (int g = 0; g < 4; ++g)
    for (int r = 0; r < nl; ++r) {
      const int i = Q.gdof[16 * g + r];
      if (i >= 0) CHECK(!in_core[i] && Q.owner[16 * g + r] == 1);
    }
  for (int i = 0; i < n_act; ++i) {
    const int L = Q.lane_of_dof[i], row = L % 16;
    CHECK(Q.diag[i] == row * 64 + L);
    if (in_core[i]) {  // the core is upward closed
      for (int j = 0; j < i; ++j) if ((s.order.aanc[i] >> j) & 1ull) CHECK(in_core[j]);
      continue;
    }
    for (int j = 0; j < i; ++j)  // a limb dof and all its non-core ancestors share a group
      if (((s.order.aanc[i] >> j) & 1ull) && !in_core[j]) CHECK(Q.lane_of_dof[j] / 16 == L / 16);
  }
}

static void check_lds(const PlanStages &s, const ModelPlan &p) {
  using plan_detail::even;
  const LdsLayout &L = p.lay;
  const gmr_blob_header &h = s.blob.h;
  const int ns = h.nslot, nb_ik = s.tree.nb_ik, nvp = p.nvp;
  const int ntmax = std::max(h.ntask[0], h.ntask[1]), ncmax = std::max(s.comp.ncomp[0], s.comp.ncomp[1]);
  const int hsize = s.use_sq ? 1024 : nvp * nvp;
  CHECK(L.total_doubles * 8 == p.lds_bytes && p.lds_bytes <= 65535);
  // the regions that alias nothing, in address order: each ends where the next begins or before
  const bool staged = !(s.use_sq && p.dm.npairp <= 64 * kHPlanRegsSQ);
  struct R { int at, len; } top[] = {
    {L.zero, kBT}, {L.hplan, staged ? p.dm.npairp : 0}, {L.q, h.nq}, {L.tp, 3 * ns}, {L.tq, 4 * ns},
    {L.bodyc < 0 ? L.S : L.bodyc, L.bodyc < 0 ? 0 : kBodyC * nb_ik}, {L.S, std::max(6 * nvp, s.use_sq ? 128 : 2 * (nvp + 2))}, {L.F, 6 * nvp},
    {L.H, L.cplan - L.H}, {L.cplan, 8 * (s.passes.ncpass[0] + s.passes.ncpass[1])}};
  int end = 0;
  for (const R &r : top) { CHECK(r.at >= end && r.len >= 0); end = r.at + r.len; }
  CHECK(L.zero == 0 && L.q % 2 == 0 && L.tp % 2 == 0 && L.tq % 2 == 0 && L.S % 2 == 0 && L.F % 2 == 0 && L.H % 2 == 0 && L.cplan % 2 == 0);
  // what may alias: Lb on S; H on [B | poses / Bc]; Bc on the poses
  CHECK(L.Lb == L.S && L.H == L.B && L.Bc == L.xpos);
  CHECK(L.B + kBT * ntmax <= L.xpos && L.xpos + 3 * nb_ik <= L.xquat && L.xquat + 4 * nb_ik <= L.cplan);
  CHECK(L.Bc + kBT * ncmax <= L.cplan && L.H + hsize + 2 <= L.cplan);
  // tring lies behind everything else
  if (L.tring >= 0) {
    CHECK(L.tring == end && ns <= kTargetBlockLanes && L.tq - L.tp + 4 * ns >= 7 * ns);
    end = L.tring + kTargetBlockFrames * (L.tq - L.tp + 4 * ns);
  } else CHECK(L.tring == -1);
  CHECK((p.shape >= 0 && ik_shape_is_plain(p.shape) && ns <= kTargetBlockLanes) == (L.tring >= 0));
  CHECK(end == L.total_doubles);
  const LdsLayout &E = p.lay_eval;
  CHECK(E.q == 0 && E.tp >= h.nq && E.tq >= E.tp + 3 * ns && E.xpos >= E.tq + 4 * ns && E.xquat >= E.xpos + 3 * h.nbody &&
        E.total_doubles == E.xquat + 4 * h.nbody && E.total_doubles * 8 == p.lds_bytes_eval);
}

static void check_fk_slots(const PlanStages &s, const ModelPlan &p) {
  const int nb = s.blob.h.nbody;
  const int32_t *parent = s.blob.parent;
  const FkSlots &F = s.slots;
  CHECK(F.nslots == p.nslots && p.nslots >= 0 && p.nslots <= kFkMaxSlots);
  std::vector<int> last_child(nb, -1), live(kFkMaxSlots, -1);  // live: the body whose pose a slot holds
  for (int b = 1; b < nb; ++b) last_child[parent[b]] = b;
  for (int b = 0; b < nb; ++b) {
    if (b > 0 && parent[b] != b - 1) {  // a branching child reads the slot its parent saved
      CHECK(F.src_slot[b] >= 0 && F.src_slot[b] == F.save_slot[parent[b]] && live[F.src_slot[b]] == parent[b]);
    } else CHECK(F.src_slot[b] == -1);
    if (b > 0 && last_child[parent[b]] == b && F.save_slot[parent[b]] >= 0) live[F.save_slot[parent[b]]] = -1;
    if (F.save_slot[b] >= 0) {
      CHECK(F.save_slot[b] < p.nslots && live[F.save_slot[b]] == -1);  // no slot is live twice
      live[F.save_slot[b]] = b;
    } else {
      CHECK(F.save_slot[b] == -1);
      for (int c = b + 2; c < nb; ++c) CHECK(parent[c] != b);  // nobody will look for it
    }
  }
  for (int sl = 0; sl < kFkMaxSlots; ++sl) CHECK(live[sl] == -1);
}

static void check_plan(const PlanStages &s, const ModelPlan &p) {
  check_order(s);
  check_hplan(s, p);
  check_composite_plan(s, p);
  check_structured_qp(s);
  check_lds(s, p);
  check_fk_slots(s, p);
}

// No blob reaches "more than kMaxCompPass passes": 32 tasks per table give at most 29 dependent passes (a chain of composites that
// each add one task to the one below).  The stage itself does, from a hand-made chain of 32 composites that each sum eight own tasks
// and their predecessor: three passes apiece.
static int too_many_passes() {
  gmr_blob_header h;
  memset(&h, 0, sizeof(h));
  h.ntask[0] = 32;
  Composites C;
  C.acomp.assign(2 * 64, 0);
  C.mask.assign(2 * 2 * GMR_MAX_TASKS, 0u); C.own.assign(64, 0u); C.kids.assign(64, 0u);
  C.ncomp[0] = 32;
  for (int c = 0; c < 32; ++c) { C.mask[c] = 0xffffffffu; C.own[c] = 0xffu; C.kids[c] = c ? 1u << (c - 1) : 0u; }
  const int ncomp[2] = {32, 0};
  LdsLayout lay = lds_layout(h, 1, 32, 0, ncomp, true);
  CompositePasses S;
  std::string msg;
  const int rc = composite_passes(h, 6, C, lay, S, msg);
  printf("%d|%s\n", rc, msg.c_str());
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "--too-many-passes")) return too_many_passes();
  if (argc != 2) { fprintf(stderr, "usage: %s MANIFEST | --too-many-passes\n", argv[0]); return 2; }
  std::ifstream manifest(argv[1]);
  std::string line;
  while (std::getline(manifest, line)) {
    std::istringstream ls(line);
    std::string blob_path, dump_path;
    int min_nvp = 0, force_generic = 0;
    if (!(ls >> blob_path >> min_nvp >> force_generic >> dump_path)) continue;
    g_case = line.c_str();
    std::ifstream bf(blob_path, std::ios::binary);
    CHECK(bf.good());
    // exactly as many bytes as the file has: a read behind them is a read behind the allocation
    const std::vector<char> blob((std::istreambuf_iterator<char>(bf)), std::istreambuf_iterator<char>());
    ModelPlan plan;
    PlanStages stages;
    std::string msg;
    const int rc = plan_model(blob.empty() ? nullptr : blob.data(), blob.size(), min_nvp, force_generic != 0, plan, msg, &stages);
    CHECK((rc == GMR_OK) == msg.empty());
    int shape = -1;
    std::string fields;
    if (rc == GMR_OK) {
      check_plan(stages, plan);
      shape = plan.shape;
      const DevModel &d = plan.dm;
#define GMR_X(f, e) fields += (fields.empty() ? "" : ",") + std::to_string(e);
      GMR_IK_SHAPE_FIELDS(GMR_X)
#undef GMR_X
      if (dump_path != "-") dump(dump_path.c_str(), plan);
    }
    printf("%d|%s|%d|%s|%s\n", rc, msg.c_str(), shape, ik_shape_name(shape), fields.c_str());
  }
  return 0;
}

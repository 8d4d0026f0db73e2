// Stand-alone check of csrc/stem_pool_plan.h (no HIP, no GPU): tests/test_stem_pool_plan_cpu.py builds and runs it.
//   1. the derived figures that tests/test_gpu_stem_pool_edges.py states beside its shapes, as literals: which chunk, strip,
//      segment or tile boundary a case sits on;
//   2. invariants of the three kernels' work decomposition and of the backward kernel's pooled loads over every geometry
//      the gates admit with Ho in [32, 70] + [250, 260], Wo in [3, 20], N in [1, 3], K in [1, 96], both strides.
// `--parent` runs the in-bounds check of the pooled loads on the arithmetic the kernel had BEFORE the plan header (every
// group of 16 filters loaded whatever M is, no lane masked): it must report loads past the end of the tensors for K < 96.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../mcncrossmodalemotions_amd/csrc/conv_plan.h"
#include "../mcncrossmodalemotions_amd/csrc/stem_pool_plan.h"

using namespace xm;

static std::atomic<long long> g_checked{0};
#define CHECK(cond)                                                                                      \
  do {                                                                                                   \
    if (!(cond)) {                                                                                       \
      std::printf("FAILED %s (line %d) %s\n", #cond, __LINE__, ctx);                                     \
      std::fflush(stdout);                                                                               \
      std::_Exit(1);                                                                                     \
    }                                                                                                    \
  } while (0)

// ---- the geometry as the library derives it ----------------------------------------------------------------------------
static Geo conv_geo(int H, int W, int N, int K, int FH, int FW, int sy, int sx, int pt, int pb, int pl, int pr) {
  Geo g{};
  g.H = H, g.W = W, g.C = 1, g.N = N, g.FH = FH, g.FW = FW, g.FC = 1, g.K = K, g.G = 1, g.Kg = K;
  g.Ho = (H + pt + pb - FH) / sy + 1, g.Wo = (W + pl + pr - FW) / sx + 1, g.R = FH * FW;
  g.sy = sy, g.sx = sx, g.pt = pt, g.pb = pb, g.pl = pl, g.pr = pr, g.dy = 1, g.dx = 1;
  return g;
}
static int pooled(int n) { return n < 3 ? 0 : (n - 3) / 2 + 1; }
static const uintptr_t kAligned = 0x7f0000001000, kOff4 = kAligned + 4;
static bool can(FusedStemDir d, const Geo &g, uintptr_t x = kAligned, uintptr_t pooled_ptrs = kAligned, int ppb = 0) {
  return fused_stem_can(d, g, x, 3, 3, 2, 2, 0, ppb, 0, ppb, pooled(g.Ho + ppb), pooled(g.Wo + ppb), pooled_ptrs);
}

// ---- 1. the figures of the edge tests --------------------------------------------------------------------------------
struct Fig {
  Geo g;
  int pHo, pWo;
  SpBwdPlan b;
  SfPlan f;
  int gram_units, gram_grid;
};
static Fig fig(int H, int W, int N, int K, int FH, int FW, int sy, int sx, int pt, int pb, int pl, int pr) {
  Fig r{};
  r.g = conv_geo(H, W, N, K, FH, FW, sy, sx, pt, pb, pl, pr);
  r.pHo = pooled(r.g.Ho), r.pWo = pooled(r.g.Wo);
  r.b = stem_bwd_plan(N, r.g.Ho, r.g.Wo);
  r.f = stem_fwd_plan(N, r.pHo, r.pWo, 2);
  r.gram_units = stem_pool_units(N, r.g.Ho, r.g.Wo), r.gram_grid = stem_pool_grid(r.gram_units, kSpGramOcc);
  return r;
}
struct Parent;
static void check_pooled_loads(int N, int Ho, int Wo, int M, bool parent, Parent *ps, std::vector<unsigned char> &quad,
                               std::vector<unsigned char> &front, const char *ctx);

// CASE FIGURES: tests/test_gpu_stem_pool_edges.py, GRAM_CASES / BWD_CASES / FWD_CASES in that file's order.  Every case is
// admitted by the gate of the kernel it is written for.
static void check_edge_figures() {
  const char *ctx = "GRAM_CASES";
  {
    const Fig c[] = {fig(68, 9, 1, 24, 7, 7, 2, 2, 1, 1, 1, 1),   fig(68, 18, 3, 24, 7, 7, 2, 2, 2, 2, 6, 1),
                     fig(132, 21, 2, 24, 8, 7, 2, 2, 0, 2, 1, 3), fig(132, 15, 1, 24, 7, 7, 2, 2, 4, 0, 1, 1),
                     fig(260, 8, 2, 24, 5, 5, 1, 1, 0, 0, 0, 0),  fig(260, 7, 1, 24, 5, 5, 1, 1, 0, 1, 1, 1),
                     fig(72, 10, 2, 24, 4, 4, 2, 1, 0, 0, 0, 0),  fig(40, 25, 1, 24, 4, 7, 1, 2, 0, 0, 0, 0),
                     fig(76, 12, 2, 24, 8, 4, 2, 2, 1, 1, 1, 1),  fig(68, 9, 700, 24, 7, 7, 2, 2, 1, 1, 1, 1)};
    const int Ho[] = {32, 33, 64, 65, 256, 257, 35, 37, 36, 32}, Wo[] = {3, 10, 10, 6, 4, 5, 7, 10, 6, 3};
    const int taps[] = {49, 49, 56, 49, 25, 25, 16, 28, 32, 49}, units[] = {2, 15, 10, 3, 4, 6, 8, 5, 6, 1400};
    const int grid[] = {8, 16, 16, 8, 8, 8, 8, 8, 8, 768};
    CHECK(units[9] > grid[9]);         // (the only case in which a block walks a second unit: its patch staged a unit ahead)
    for (int i = 0; i < 10; ++i) {
      CHECK(stem_pool_can(c[i].g, kAligned) && !stem_pool_can(c[i].g, kOff4));
      CHECK(c[i].g.Ho == Ho[i] && c[i].g.Wo == Wo[i] && c[i].g.R == taps[i] && c[i].gram_units == units[i] && c[i].gram_grid == grid[i]);
    }
    // Ho 32: wave 0 alone has rows, its second 32-row chunk is absent; 33: the second chunk has one row; 64: both full,
    // wave 1 idle; 65: wave 1 has one row
    const FastDiv one = make_fastdiv(1u);
    CHECK(!sp_gram_unit(0, 0, one, one, 32, 3).chunk1 && !sp_gram_unit(0, 1, one, one, 32, 3).live);
    CHECK(sp_gram_unit(0, 0, one, one, 33, 3).chunk1 && 33 - 32 == 1);
    CHECK(sp_gram_unit(0, 0, one, one, 64, 3).chunk1 && !sp_gram_unit(0, 1, one, one, 64, 3).live);
    CHECK(sp_gram_unit(0, 1, one, one, 65, 3).live && !sp_gram_unit(0, 1, one, one, 65, 3).chunk1 && 65 - 64 == 1);
    // Ho 256: one 256-row group, all four waves full; 257: a second group whose wave 0 has one row, waves 1 - 3 none
    CHECK(sp_row_groups(256) == 1 && sp_row_groups(257) == 2 && sp_gram_unit(0, 3, one, one, 256, 4).chunk1);
    const FastDiv two = make_fastdiv(2u);
    const SpUnit g1 = sp_gram_unit(1, 0, make_fastdiv(6u), two, 257, 5);
    CHECK(g1.jp == 0 && g1.cp == 4 && g1.live && !g1.chunk1 && !sp_gram_unit(1, 1, make_fastdiv(6u), two, 257, 5).live);
    // Wo 3 / 5 / 7: the last column pair has one column; the ones column (tap index R) of 32 taps opens column tile 1
    CHECK(!sp_gram_unit(1, 0, make_fastdiv(2u), one, 32, 3).col1 && sp_gram_unit(0, 0, make_fastdiv(2u), one, 32, 3).col1);
    CHECK(c[8].g.R == 32 && c[6].g.R == 16);
    // pt 0 and 4, pl 6 (the first output column sees source column 0 alone), pr > pl, strides (2, 1) and (1, 2)
    CHECK(c[2].g.pt == 0 && c[3].g.pt == 4 && c[1].g.pl == 6 && c[1].g.FW - c[1].g.pl == 1 && c[2].g.pr > c[2].g.pl);
    CHECK(c[6].g.sy == 2 && c[6].g.sx == 1 && c[7].g.sy == 1 && c[7].g.sx == 2);
  }
  ctx = "BWD_CASES";
  {
    const Fig c[] = {fig(68, 9, 1, 1, 7, 7, 2, 2, 1, 1, 1, 1),    fig(68, 18, 3, 15, 7, 7, 2, 2, 2, 2, 6, 1),
                     fig(132, 21, 1, 16, 8, 7, 2, 2, 0, 2, 1, 3), fig(132, 15, 3, 17, 7, 7, 2, 2, 4, 0, 1, 1),
                     fig(260, 8, 1, 33, 5, 5, 1, 1, 0, 0, 0, 0),  fig(260, 7, 2, 47, 5, 5, 1, 1, 0, 1, 1, 1),
                     fig(72, 10, 1, 65, 4, 4, 2, 1, 0, 0, 0, 0),  fig(40, 25, 3, 95, 4, 7, 1, 2, 0, 0, 0, 0),
                     fig(76, 12, 2, 96, 8, 4, 2, 2, 1, 1, 1, 1),  fig(132, 463, 3, 40, 7, 7, 2, 2, 4, 0, 1, 1)};
    const int Ho[] = {32, 33, 64, 65, 256, 257, 35, 37, 36, 65}, Wo[] = {3, 10, 10, 6, 4, 5, 7, 10, 6, 230};
    const int pHo[] = {15, 16, 31, 32, 127, 128, 17, 18, 17, 32}, pWo[] = {1, 4, 4, 2, 1, 2, 3, 4, 2, 114};
    const int ncp[] = {1, 1, 1, 2, 4, 5, 1, 1, 1, 2}, units[] = {2, 15, 5, 18, 8, 30, 4, 15, 6, 690};
    const int grid[] = {24, 24, 24, 24, 24, 24, 24, 24, 24, 504};
    for (int i = 0; i < 10; ++i) {
      CHECK(can(kFusedStemBackward, c[i].g) && !can(kFusedStemBackward, c[i].g, kOff4) && can(kFusedStemBackward, c[i].g, kAligned, kOff4));
      CHECK(!can(kFusedStemBackward, c[i].g, kAligned, kAligned + 2) && !can(kFusedStemBackward, c[i].g, kAligned, kAligned, 1));
      CHECK(c[i].g.Ho == Ho[i] && c[i].g.Wo == Wo[i] && c[i].pHo == pHo[i] && c[i].pWo == pWo[i]);
      CHECK(c[i].b.ncp == ncp[i] && c[i].b.nunits == units[i] && c[i].b.grid == grid[i] && c[i].b.nwc == grid[i] * 4 / 3);
      CHECK(c[i].b.npair == pWo[i] + 1);
    }
    // the grid grows with the units up to 504 blocks = 672 waves per row tile: only beyond 672 units does a wave walk a
    // second unit, its operands in flight a unit ahead (the last case: 18 waves per row tile do)
    CHECK(units[9] > 672 && units[9] - 672 == 18);
    // filters: which groups of 16 exist per row tile (rt, it) and how many lanes of the partly filled one
    struct { int K, groups, partial; } k[] = {{1, 1, 1}, {15, 1, 15}, {16, 1, 0}, {17, 2, 1}, {33, 3, 1}, {47, 3, 15}, {65, 5, 1}, {95, 6, 15}, {96, 6, 0}, {40, 3, 8}};
    for (int i = 0; i < 10; ++i) {
      int groups = 0;
      for (int rt = 0; rt < 3; ++rt)
        for (int it = 0; it < 2; ++it) groups += 32 * rt + 16 * it < k[i].K;
      CHECK(c[i].g.K == k[i].K && groups == k[i].groups && k[i].K % 16 == k[i].partial);
    }
    // pHo 15 (Ho 32): fewer window rows than a wave's 32 -- a quad reaches two columns / planes on; pHo 32 (Ho 65) and 128
    // (Ho 257): the last chunk pair holds ONE output row and is fed by the row in front (window row 31 / 127) alone
    CHECK(pHo[0] < 32 - 16 && 32 * 1 - 1 == pHo[3] - 1 && 64 * 1 + 1 == Ho[3] && 32 * 4 - 1 == pHo[5] - 1 && 64 * 4 + 1 == Ho[5]);
    CHECK(c[6].g.sy == 2 && c[6].g.sx == 1 && c[7].g.sy == 1 && c[7].g.sx == 2 && c[6].g.R == 16 && c[7].g.R == 28 && c[8].g.R == 32);
    // the pooled loads of exactly these launches (the last one lies outside the sweep below)
    std::vector<unsigned char> quad, front;
    for (int i = 0; i < 10; ++i) check_pooled_loads(c[i].g.N, c[i].g.Ho, c[i].g.Wo, c[i].g.K, false, nullptr, quad, front, ctx);
  }
  ctx = "FWD_CASES";
  {
    const Fig c[] = {fig(68, 9, 1, 8, 7, 7, 2, 2, 1, 1, 1, 1),     fig(264, 8, 3, 24, 7, 7, 2, 2, 1, 1, 6, 1),
                     fig(512, 30, 1, 32, 7, 7, 2, 2, 1, 3, 1, 2),  fig(68, 33, 2, 40, 5, 7, 2, 2, 0, 0, 1, 1),
                     fig(72, 37, 1, 72, 3, 7, 2, 2, 4, 0, 1, 1),   fig(68, 201, 1, 96, 7, 7, 2, 2, 1, 1, 1, 1),
                     fig(68, 9, 700, 8, 7, 7, 2, 2, 1, 1, 1, 1)};
    const int pHo[] = {15, 64, 127, 15, 18, 15, 15}, pWo[] = {1, 2, 6, 7, 8, 49, 1}, Wo[] = {3, 5, 14, 15, 17, 99, 3};
    const int NS[] = {1, 2, 3, 1, 1, 1, 1}, SG[] = {1, 2, 6, 7, 8, 13, 1}, units[] = {3, 36, 54, 42, 24, 39, 2100};
    CHECK(units[6] > 2048 && c[6].f.grid == 512);      // (the only case in which a wave takes a second unit)
    for (int i = 0; i < 7; ++i) {
      CHECK(can(kFusedStemForward, c[i].g) && !can(kFusedStemForward, c[i].g, kOff4) && can(kFusedStemForward, c[i].g, kAligned, kOff4));
      CHECK(c[i].pHo == pHo[i] && c[i].pWo == pWo[i] && c[i].g.Wo == Wo[i]);
      CHECK(c[i].f.NS == NS[i] && c[i].f.SG == SG[i] && c[i].f.nunits == units[i] && c[i].f.grid == std::min(512, (units[i] + 3) / 4));
    }
    // strips of 63 window rows: pHo 64 = 63 + 1, 127 = 2 * 63 + 1
    CHECK(64 - kSfStrip == 1 && 127 - 2 * kSfStrip == 1);
    // segments: up to 16 window columns the selection loop gives every window column a segment of its own (SG = pWo: three
    // output columns per unit, the ring of 7 source columns never wraps), so the ring period is reached through the column
    // count alone: 49 window columns in 13 segments (13 does not divide 49) of 3 and 4 = 7 and 9 output columns per unit,
    // exactly one period and a period + 2
    CHECK(49 % 13 != 0);
    int threes = 0, fours = 0;
    for (int seg = 0; seg < 13; ++seg) {
      const SfUnit u = sf_unit(3 * seg, make_fastdiv(3u), make_fastdiv(13u), make_fastdiv(1u), 49, 13);
      threes += u.pw1 - u.pw0 == 3, fours += u.pw1 - u.pw0 == 4;
    }
    CHECK(threes == 3 && fours == 10 && 2 * 3 + 1 == 7 && 2 * 4 + 1 == 9);
    // filters: groups of 8 that exist in the last live row tile: K 8 -> 1, 24 -> 3, 32 -> 4 (full), 40 -> 1, 72 -> 1, 96 -> 4
    const int K[] = {8, 24, 32, 40, 72, 96, 8}, last[] = {1, 3, 4, 1, 1, 4, 1};
    for (int i = 0; i < 7; ++i) {
      const int rt = (K[i] - 1) / 32;
      CHECK(c[i].g.K == K[i] && std::min(4, (K[i] - 32 * rt) >> 3) == last[i]);
    }
    CHECK(c[3].g.FH == 5 && c[4].g.FH == 3 && c[3].g.pt == 0 && c[4].g.pt == 4 && c[1].g.pl == 6);
    // every case runs the backward kernel through its own table as well
    std::vector<unsigned char> quad, front;
    for (int i = 0; i < 7; ++i) {
      CHECK(can(kFusedStemBackward, c[i].g));
      check_pooled_loads(c[i].g.N, c[i].g.Ho, c[i].g.Wo, c[i].g.K, false, nullptr, quad, front, ctx);
    }
    // gates: K % 8, Ho 31, a padded pooling
    Geo g = conv_geo(68, 20, 1, 12, 7, 7, 2, 2, 1, 1, 1, 1);
    CHECK(!can(kFusedStemForward, g) && can(kFusedStemBackward, g));
    g = conv_geo(64, 20, 1, 16, 7, 7, 2, 2, 2, 2, 2, 2);
    CHECK(g.Ho == 31 && !stem_pool_can(g, kAligned) && !can(kFusedStemForward, g) && !can(kFusedStemBackward, g));
    g = conv_geo(68, 20, 1, 16, 7, 7, 2, 2, 1, 1, 1, 1);
    CHECK(can(kFusedStemForward, g) && !can(kFusedStemForward, g, kAligned, kAligned, 1));
  }
}

// ---- 2. sweep ------------------------------------------------------------------------------------------------------------
struct Parent {
  long long oob = 0, loads = 0;
  int firstK = 0, firstN = 0, firstRt = 0, firstIt = 0, firstHo = 0, firstWo = 0;
  long long worst = 0;
  int worstK = 0, worstN = 0, worstRt = 0, worstIt = 0, worstHo = 0, worstWo = 0;
  long long oob96 = 0;
};

// The lane offsets as conv_stem_wgrad_pool_kernel formed them BEFORE stem_pool_plan.h existed (`--parent`): both groups of
// 16 filters whatever M is, no lane masked, quads shifted back in the tensor's last window column only.
static void parent_cand(SpCand &k, const SpUnit &c, int rt, int lane, int M, int N, int pHo, int pWo) {
  const int pHW = pHo * pWo, cl = lane >> 2, qd = lane & 3;
  k.jp = c.jp;
  k.ok[1] = c.live && c.jp < pWo;
  k.ok[0] = c.live && c.jp >= 1 && c.jp - 1 < pWo;
  const bool lastplane = c.n * M + 32 * rt + 32 >= M * N;
  k.anyshift = lastplane && c.jp >= pWo - 1 && 32 * c.cp + 32 > pHo;
  for (int h = 0; h < 2; ++h) {
    const int ph0 = 32 * c.cp + 16 * h + 4 * qd;
    k.voff[h] = (unsigned)(cl * pHW + (k.anyshift ? std::min(ph0, pHo - 4) : ph0));
  }
  const bool exok = c.cp > 0 && qd < 2 && (qd ? k.ok[1] : k.ok[0]);
  k.exoff = exok ? (unsigned)((cl * pWo + c.jp - 1 + qd) * pHo + 32 * c.cp - 1) : 0x3FFFFFFFu;
  k.grp[0] = k.grp[1] = true;
  k.sbase = (c.n * M + 32 * rt) * pHW;
}

// stem_gram_kernel: every (sample, column pair, 64-row chunk pair that holds rows) is multiplied by exactly one wave
static void check_gram(int N, int Ho, int Wo, const char *ctx) {
  const int nunits = stem_pool_units(N, Ho, Wo), grid = stem_pool_grid(nunits, kSpGramOcc);
  CHECK(grid % 8 == 0 && grid >= 8 && grid <= 256 * kSpGramOcc);
  CHECK(stem_gram_part_floats(N, Ho, Wo) == (size_t)grid * 64 * 64);
  const int npair = sp_col_pairs(Wo), G = sp_row_groups(Ho), ncp = sp_chunk_pairs(Ho);
  const FastDiv divJG = make_fastdiv((uint32_t)(npair * G)), divG = make_fastdiv((uint32_t)G);
  std::vector<int> seen((size_t)N * npair * ncp, 0);
  for (int b = 0; b < grid; ++b) {
    const SpGramWalk w = sp_gram_walk(b, grid, nunits);
    for (int q = w.q0; q < w.tend; q += w.tstep)
      for (int wave = 0; wave < 4; ++wave) {
        const SpUnit c = sp_gram_unit(w.tbase + q, wave, divJG, divG, Ho, Wo);
        CHECK(w.tbase + q < nunits && c.n >= 0 && c.n < N && c.jp >= 0 && c.jp < npair);
        CHECK(c.live == (64 * c.cp < Ho) && c.col1 == (2 * c.jp + 1 < Wo) && c.chunk1 == (64 * c.cp + 32 < Ho));
        if (c.live) ++seen[((size_t)c.n * npair + c.jp) * ncp + c.cp];
      }
  }
  for (int v : seen) CHECK(v == 1);
  g_checked += (long long)seen.size();
}

// conv_stem_bnpool_fwd_kernel: every (sample, strip, segment, row tile) is one wave unit; the segments tile [0, pWo)
static void check_fwd(int N, int pHo, int pWo, const char *ctx) {
  for (int sg = 1; sg <= std::min(16, pWo); ++sg) {          // every count the selection loop can choose
    int next = 0;
    for (int seg = 0; seg < sg; ++seg) {
      const SfUnit c = sf_unit(3 * seg, make_fastdiv(3u), make_fastdiv((uint32_t)sg), make_fastdiv(1u), pWo, sg);
      CHECK(c.seg == seg && c.rt == 0 && c.n == 0 && c.strip == 0);
      CHECK(c.pw0 == next && c.pw1 > c.pw0);                  // no gap, no overlap, no empty segment
      next = c.pw1;
    }
    CHECK(next == pWo);
    g_checked += sg;
  }
  const SfPlan p = stem_fwd_plan(N, pHo, pWo, 2);
  CHECK(p.SG >= 1 && p.SG <= std::min(16, pWo) && p.NS == (pHo + 62) / 63 && p.nunits == N * p.NS * p.SG * 3);
  CHECK(p.grid >= 1 && p.grid <= 512 && p.grid * 4 >= std::min(p.nunits, 2048));
  CHECK(63 * (p.NS - 1) < pHo && 63 * p.NS >= pHo);
  const FastDiv d3 = make_fastdiv(3u), dSG = make_fastdiv((uint32_t)p.SG), dNS = make_fastdiv((uint32_t)p.NS);
  std::vector<int> seen((size_t)p.nunits, 0);
  for (int b = 0; b < p.grid; ++b)
    for (int wv = 0; wv < 4; ++wv)
      for (int unit = b * 4 + wv; unit < p.nunits; unit += p.grid * 4) {
        const SfUnit c = sf_unit(unit, d3, dSG, dNS, pWo, p.SG);
        CHECK(c.n >= 0 && c.n < N && c.strip >= 0 && c.strip < p.NS && c.seg >= 0 && c.seg < p.SG && c.rt >= 0 && c.rt < 3);
        ++seen[(((size_t)c.n * p.NS + c.strip) * p.SG + c.seg) * 3 + c.rt];
      }
  for (int v : seen) CHECK(v == 1);
  g_checked += p.nunits;
}

// conv_stem_wgrad_pool_kernel: the logical waves are a permutation, a third of them per row tile; every unit is walked by
// exactly one wave of each row tile
static void check_bwd_units(int N, int Ho, int Wo, const char *ctx) {
  const SpBwdPlan p = stem_bwd_plan(N, Ho, Wo);
  CHECK(p.grid % 24 == 0 && p.grid >= 24 && p.grid <= 504 && p.nwc * 3 == p.grid * 4);
  CHECK(p.ncp == (Ho + 63) / 64 && p.npair == (Wo + 1) / 2 && p.nunits == N * p.npair * p.ncp);
  const FastDiv divG = make_fastdiv((uint32_t)p.ncp), divJG = make_fastdiv((uint32_t)p.npair);
  std::vector<int> wseen((size_t)p.grid * 4, 0), useen((size_t)p.nunits * 3, 0);
  for (int b = 0; b < p.grid; ++b)
    for (int wv = 0; wv < 4; ++wv) {
      const SpWave w = sp_bwd_wave(b, p.grid, wv);
      CHECK(w.wl >= 0 && w.wl < p.grid * 4 && w.rt == w.wl % 3 && w.wc == w.wl / 3 && w.wc < p.nwc);
      ++wseen[w.wl];
      for (int u = w.wc; u < p.nunits; u += p.nwc) {
        const SpUnit c = sp_bwd_unit(u, p.nunits, divG, divJG, Ho, Wo);
        CHECK(c.live && u == (c.n * p.npair + c.jp) * p.ncp + c.cp && c.n < N && c.jp < p.npair && c.cp < p.ncp);
        CHECK(c.col1 == (2 * c.jp + 1 < Wo) && c.chunk1 == (64 * c.cp + 32 < Ho) && 64 * c.cp < Ho);
        ++useen[(size_t)u * 3 + w.rt];
      }
    }
  for (int v : wseen) CHECK(v == 1);
  for (int v : useen) CHECK(v == 1);
  // what the kernel asks for beyond the last unit (its prefetch): the last unit's geometry, not live
  const SpUnit c = sp_bwd_unit(p.nunits + 5, p.nunits, divG, divJG, Ho, Wo);
  CHECK(!c.live && c.n == N - 1 && c.jp == p.npair - 1 && c.cp == p.ncp - 1);
  g_checked += (long long)useen.size();
}

// The pooled loads of conv_stem_wgrad_pool_kernel for one (Ho, Wo, N, M): dzdy_pool / y_pool (4-byte elements, 16-byte
// quads and the 4-byte row in front) and argmax (1-byte elements, 4-byte quads and a 1-byte row in front) share the
// offsets in ELEMENTS.  The hardware compares the lane part alone with num_records (the tensor's bytes) and returns zero
// without an access at or above it; otherwise lane part + scalar part + width must lie inside the tensor.
//
// Deliveries the kernel's design states (header of conv_stem_wgrad_pool_kernel): a pooled element (ph, pw, m, n) belongs to
// the wave row tile m / 32, group it = (m % 32) / 16, lanes cl = m % 16, qd = (ph % 16) / 4, chunk h = (ph % 32) / 16,
// element e = ph % 4, and is delivered live
//   * as part of a quad TWICE per row tile walk: by the unit (n, jp = pw, cp = ph / 32) as window column p = 1 and by the
//     unit (n, jp = pw + 1, cp) as p = 0 (there are pWo + 1 column pairs for pWo window columns: both units exist);
//   * as the single row in front of a chunk pair TWICE more when ph = 32 cp' - 1 for a chunk pair cp' = (ph + 1) / 32 that
//     exists: by (n, pw, cp') on the lane qd = 1 and by (n, pw + 1, cp') on the lane qd = 0;
// and a lane whose filter does not exist (>= M) accesses nothing.
static void check_pooled_loads(int N, int Ho, int Wo, int M, bool parent, Parent *ps, std::vector<unsigned char> &quad,
                               std::vector<unsigned char> &front, const char *ctx) {
  const int pHo = pooled(Ho), pWo = pooled(Wo), pHW = pHo * pWo;
  const long long total = (long long)pHW * M * N;
  const unsigned elems = (unsigned)total;
  const SpBwdPlan bp = stem_bwd_plan(N, Ho, Wo);
  CHECK(bp.npair == pWo + 1);
  const FastDiv divG = make_fastdiv((uint32_t)bp.ncp), divJG = make_fastdiv((uint32_t)bp.npair);
  if (!parent) {
    quad.assign((size_t)total, 0);
    front.assign((size_t)total, 0);
  }
  // one load of `width` elements at lane part vo, scalar part so: true when it reaches memory (then it is inside)
  auto access = [&](unsigned vo, int so, int width, int rt, int it) {
    // the kernel forms BYTE offsets in 32 bits: element offset * 4 for the float tensors, * 1 for the table
    const unsigned vo4 = vo * 4u;
    const bool reach4 = vo4 < elems * 4u, reach1 = vo < elems;
    if (!parent) CHECK(reach4 == reach1);
    if (!reach4) return false;
    const long long lo = (long long)so + vo, hi = lo + width;
    const bool inside = so >= 0 && lo >= 0 && hi <= total;
    if (parent) {
      ++ps->loads;
      if (!inside) {
        if (M == 96) ++ps->oob96;
        if (!ps->oob++) ps->firstK = M, ps->firstN = N, ps->firstRt = rt, ps->firstIt = it, ps->firstHo = Ho, ps->firstWo = Wo;
        if (hi - total > ps->worst)
          ps->worst = hi - total, ps->worstK = M, ps->worstN = N, ps->worstRt = rt, ps->worstIt = it, ps->worstHo = Ho, ps->worstWo = Wo;
      }
      return inside;
    }
    CHECK(inside);
    return true;
  };
  long long n = 0;
  for (int rt = 0; rt < 3; ++rt)
    for (int u = 0; u <= bp.nunits; ++u) {                         // (u == nunits: the prefetch behind the last unit)
      const SpUnit c = sp_bwd_unit(u, bp.nunits, divG, divJG, Ho, Wo);
      for (int lane = 0; lane < 64; ++lane) {
        const int cl = lane >> 2, qd = lane & 3;
        SpCand k = sp_cand_of(c, rt, lane, M, pHo, pWo, elems);
        if (parent) parent_cand(k, c, rt, lane, M, N, pHo, pWo);
        if (!c.live) CHECK(!k.ok[0] && !k.ok[1] && k.exoff == kSpNoLoad);
        CHECK(k.ok[1] == (c.live && c.jp < pWo) && k.ok[0] == (c.live && c.jp >= 1));
        if (!parent) CHECK(k.grp[0] == (32 * rt < M) && k.grp[1] == (32 * rt + 16 < M));
        for (int it = 0; it < 2; ++it) {
          const int m = 32 * rt + 16 * it + cl;
          const bool mine = sp_filter_ok(rt, it, lane, M);
          CHECK(mine == (m < M));
          if (!parent) CHECK(!mine || k.grp[it]);
          for (int p = 0; p < 2; ++p) {
            if (parent ? !k.ok[p] : !sp_cand_issued(k, it, p)) continue;
            const int so = sp_cand_so(k, it, p, pHo, pWo), col = c.jp - 1 + p;
            for (int h = 0; h < 2; ++h) {
              const unsigned vo = parent ? k.voff[h] : sp_cand_voff(k, h, mine);
              const bool reached = access(vo, so, 4, rt, it);
              if (parent) continue;
              CHECK(reached == mine);                              // a filter that does not exist: no access
              if (!mine) continue;
              const int ph0 = 32 * c.cp + 16 * h + 4 * qd;
              CHECK((long long)so + vo == (((long long)c.n * M + m) * pWo + col) * pHo + ph0 - k.shift[h]);
              CHECK(k.shift[h] >= 0 && (k.shift[h] == 0 || k.anyshift));
              for (int e = 0; e < 4; ++e) {
                const bool live = (k.vmask >> (4 * h + e)) & 1u;
                CHECK(live == (ph0 + e < pHo));
                if (!live) continue;
                CHECK(e + k.shift[h] <= 3);                        // the re-aligned quad holds it
                ++quad[(size_t)((((long long)c.n * M + m) * pWo + col) * pHo + ph0 + e)];
              }
            }
          }
          const int so = sp_cand_exso(k, it, pHo, pWo);
          const unsigned xo = parent ? k.exoff : sp_cand_exoff(k, mine);
          const bool reached = access(xo, so, 1, rt, it);
          if (parent) continue;
          const bool want = mine && c.live && c.cp > 0 && qd < 2 && (qd ? k.ok[1] : k.ok[0]);
          CHECK(reached == want);
          if (reached) {
            const long long at = (((long long)c.n * M + m) * pWo + c.jp - 1 + qd) * pHo + 32 * c.cp - 1;
            CHECK((long long)so + xo == at);
            ++front[(size_t)at];
          }
        }
        ++n;
      }
    }
  if (!parent) {
    size_t i = 0;
    for (int s = 0; s < N; ++s)
      for (int m = 0; m < M; ++m)
        for (int pw = 0; pw < pWo; ++pw)
          for (int ph = 0; ph < pHo; ++ph, ++i) {
            CHECK(quad[i] == 2);
            CHECK(front[i] == ((ph % 32 == 31 && (ph + 1) / 32 < bp.ncp) ? 2 : 0));
          }
    n += (long long)total;
  }
  g_checked += n;
}

// the (Ho, stride) pairs some admitted geometry reaches: H a multiple of 4 up to 512, <= 8 filter rows, pt <= 4
static bool admitted(int Ho, int Wo, int N, int K, int sy, const char *ctx) {
  for (int FH = 4; FH <= 8; ++FH)
    for (int pt = 0; pt <= 4; ++pt)
      for (int pb = 0; pb <= 4; ++pb) {
        const int H = (Ho - 1) * sy + FH - pt - pb;
        if (H <= 0 || H % 4) continue;
        const int FW = 7, W = (Wo - 1) * sy + FW;
        const Geo g = conv_geo(H, W, N, K, FH, FW, sy, sy, pt, pb, 0, 0);
        CHECK(g.Ho == Ho && g.Wo == Wo);
        if (can(kFusedStemBackward, g)) return true;
      }
  return false;
}

int main(int argc, char **argv) {
  const bool parent = argc > 1 && !std::strcmp(argv[1], "--parent");
  if (!parent) check_edge_figures();
  std::vector<int> hos;
  for (int Ho = 32; Ho <= 70; ++Ho) hos.push_back(Ho);
  for (int Ho = 250; Ho <= 260; ++Ho) hos.push_back(Ho);
  if (parent) hos = {32, 65};      // (enough to show it: one and two chunk pairs)
  const unsigned hw = std::thread::hardware_concurrency();
  const int nthreads = (int)std::max(1u, std::min(8u, hw ? hw : 1u));
  std::vector<Parent> stats((size_t)nthreads);
  std::atomic<int> nextHo{0};
  std::atomic<long long> geos{0};
  auto work = [&](int tid) {
    std::vector<unsigned char> quad, front;
    char ctx[128];
    for (int i = nextHo++; i < (int)hos.size(); i = nextHo++) {
      const int Ho = hos[(size_t)i];
      for (int Wo = 3; Wo <= 20; ++Wo)
        for (int N = 1; N <= 3; ++N) {
          std::snprintf(ctx, sizeof ctx, "Ho %d Wo %d N %d", Ho, Wo, N);
          bool any = false;
          for (int sy = 1; sy <= 2; ++sy) {
            if (!admitted(Ho, Wo, N, 96, sy, ctx)) continue;
            any = true;
            ++geos;
            if (parent) continue;
            // (the plans read the output grid alone: the same assertions hold, and are made, for either stride)
            check_gram(N, Ho, Wo, ctx);
            check_bwd_units(N, Ho, Wo, ctx);
            check_fwd(N, pooled(Ho), pooled(Wo), ctx);
          }
          if (!any) continue;
          for (int K = 1; K <= 96; ++K) {
            std::snprintf(ctx, sizeof ctx, "Ho %d Wo %d N %d K %d", Ho, Wo, N, K);
            check_pooled_loads(N, Ho, Wo, K, parent, &stats[(size_t)tid], quad, front, ctx);
          }
        }
    }
  };
  std::vector<std::thread> th;
  for (int i = 0; i < nthreads; ++i) th.emplace_back(work, i);
  for (auto &t : th) t.join();
  if (parent) {
    // totals over the threads; "first" = the smallest K (then N) among the threads' first offenders
    Parent s{};
    bool have = false;
    for (const Parent &p : stats) {
      s.oob += p.oob, s.loads += p.loads, s.oob96 += p.oob96;
      if (p.oob && (!have || p.firstK < s.firstK || (p.firstK == s.firstK && p.firstN < s.firstN)))
        s.firstK = p.firstK, s.firstN = p.firstN, s.firstRt = p.firstRt, s.firstIt = p.firstIt, s.firstHo = p.firstHo, s.firstWo = p.firstWo, have = true;
      if (p.worst > s.worst)
        s.worst = p.worst, s.worstK = p.worstK, s.worstN = p.worstN, s.worstRt = p.worstRt, s.worstIt = p.worstIt, s.worstHo = p.worstHo, s.worstWo = p.worstWo;
    }
    std::printf("parent arithmetic: %lld of %lld loads that reach memory end past the tensor (%lld of them at K = 96)\n", s.oob,
                s.loads, s.oob96);
    {
      // the reported example: 40 filters, two samples -- planes of the last sample's rows 40 .. 95 lie behind the tensor
      Parent e{};
      std::vector<unsigned char> quad, front;
      check_pooled_loads(2, 65, 6, 40, true, &e, quad, front, "K 40 N 2");
      const int pHW = pooled(65) * pooled(6);
      std::printf("K 40, N 2 (Ho 65, Wo 6): %lld loads end past the tensor, the furthest in plane %lld of %d (rt %d it %d)\n", e.oob,
                  (2LL * 40 * pHW + e.worst - 1) / pHW, 2 * 40, e.worstRt, e.worstIt);
    }
    if (s.oob) {
      std::printf("FAILED in-bounds: e.g. K %d N %d rt %d it %d (Ho %d Wo %d); furthest: %lld elements past the end at K %d N %d rt %d it %d (Ho %d Wo %d)\n",
                  s.firstK, s.firstN, s.firstRt, s.firstIt, s.firstHo, s.firstWo, s.worst, s.worstK, s.worstN, s.worstRt, s.worstIt,
                  s.worstHo, s.worstWo);
      return 1;
    }
    return 0;
  }
  std::printf("%lld checks over %lld (Ho, Wo, N, stride) geometries x 96 filter counts OK\n", g_checked.load(), geos.load());
  return 0;
}

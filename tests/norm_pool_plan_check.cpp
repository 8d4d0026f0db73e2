// Stand-alone check of csrc/norm_pool_plan.h (no HIP, no GPU): tests/test_norm_pool_plan_cpu.py builds and runs it.
//   1. the derived quantities that tests/test_gpu_norm_pool_edges.py, tests/pool_routing.py (LDS_CASES) and
//      tests/test_gpu_misc_edges.py state beside their shapes, as literals: which kernel and which branch a case reaches;
//   2. invariants of every plan over a sweep of small geometries.
#include <cstdio>
#include <cstdlib>

#include "../mcncrossmodalemotions_amd/csrc/norm_pool_plan.h"

using namespace xm;

static long g_checked = 0;
static const char *g_case = "";
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) {                                                               \
      std::printf("FAILED %s (line %d) %s\n", #cond, __LINE__, g_case);          \
      std::exit(1);                                                              \
    }                                                                            \
  } while (0)

// the geometry as the library's pool_geo derives it; false where it refuses (pad >= window, window past the padded input)
static bool geo(PoolGeo &g, int H, int W, int ph, int pw, int sy, int sx, int pt, int pb, int pl, int pr) {
  if (pt >= ph || pb >= ph || pl >= pw || pr >= pw) return false;
  const int th = H + pt + pb - ph, tw = W + pl + pr - pw;
  if (th < 0 || tw < 0) return false;
  g = PoolGeo{H, W, th / sy + 1, tw / sx + 1, ph, pw, sy, sx, pt, pl};
  return true;
}
static PoolGeo geo_of(int H, int W, int ph, int pw, int sy, int sx, int pt = 0, int pb = 0, int pl = 0, int pr = 0) {
  PoolGeo g{};
  CHECK(geo(g, H, W, ph, pw, sy, sx, pt, pb, pl, pr));
  return g;
}

// what block (plane, group) of pool_fwd_lds_kernel does with the plan: first staged input column, offset of its run inside
// a 16-byte unit, and whether the last quad it loads ends past the tensor of `total` elements (the three-scalar tail load)
struct LdsBlock {
  int wlo, cols, lead;
  bool tail;
};
static LdsBlock lds_block(const PoolGeo &g, const PoolLds &p, int plane, int group, size_t total) {
  const int wo0 = group * p.wob, nwo = std::min(p.wob, g.Wo - wo0);
  const int wlo = std::max(wo0 * g.sx - g.pl, 0), whi = std::min((wo0 + nwo - 1) * g.sx - g.pl + g.pw, g.W);
  const size_t base = (size_t)plane * g.H * g.W + (size_t)wlo * g.H;
  const int lead = (int)(base & 3), cnt = (whi - wlo) * g.H + lead;
  return LdsBlock{wlo, whi - wlo, lead, base - lead + (size_t)((cnt - 1) / 4 * 4) + 3 >= total};
}

// ---- 1. the figures of the edge tests --------------------------------------------------------------------------------
static const uintptr_t kAligned = 0x7f0000001000, kOff4 = kAligned + 4;   // misaligned(): one float past a 16-byte boundary

static void check_bnorm_figures() {
  g_case = "BN_EDGE_SHAPES";
  CHECK(bn_splits(300, 9) == 6 && bn_dxsum_splits(300, 9) == 9);
  CHECK(bn_splits(600, 9) == 3 && bn_dxsum_splits(600, 9) == 6);
  CHECK(bn_splits(4100, 3) == 1 && bn_dxsum_splits(4100, 3) == 1);
  CHECK(bn_splits(8, 70) == 70 && bn_dxsum_splits(8, 70) == 70);
  CHECK(bn_splits(32, 17) == 17 && bn_dxsum_splits(32, 17) == 17);
  // run lengths of the reduction kernels: (2,2) one quad, (3,1) three elements, (1,8) two quads, (1,1) one element
  CHECK(bn_vec(4, kAligned) && bn_run(4, true) == 1 && !bn_vec(3, kAligned) && bn_run(3, false) == 3);
  CHECK(bn_vec(8, kAligned) && bn_run(8, true) == 2 && !bn_vec(1, kAligned) && bn_run(1, false) == 1);
  CHECK(!bn_vec(4, kOff4) && bn_run(4, false) == 4);                       // bn_stats_partial_kernel from an unaligned x
  // (64,64,32,17): 557,056 quads on 2,048 blocks of 256 -> a second trip; the scalar arm with ONE operand misaligned
  const size_t total = (size_t)64 * 64 * 32 * 17;
  CHECK(total / 4 == 557056 && ew_grid(557056) == 2048 && (size_t)2048 * 256 < 557056);
  CHECK(bn_vec(64 * 64, kAligned, kAligned) && bn_vec(64 * 64, kAligned, kAligned, kAligned, kAligned));
  CHECK(bn_vec(64 * 64, kAligned, kAligned, kAligned, (uintptr_t)0));      // yfwd == NULL
  for (int k = 0; k < 4; ++k)
    CHECK(!bn_vec(64 * 64, k == 0 ? kOff4 : kAligned, k == 1 ? kOff4 : kAligned, k == 2 ? kOff4 : kAligned,
                  k == 3 ? kOff4 : kAligned));
  CHECK(!bn_vec(64 * 64, kOff4, kAligned) && !bn_vec(64 * 64, kAligned, kOff4) && ew_grid(total) == 2048);
  CHECK(bn_vec(2 * 2, kAligned, kAligned) && bn_vec(4 * 2, kAligned, kAligned) && !bn_vec(3 * 3, kAligned, kAligned));
  // tests/test_gpu_misc_edges.py: n = 2,100,003
  CHECK(ew_grid(2100003 / 4 + 1) == 2048 && ew_grid(2100003) == 2048 && ew_grid(3) == 1 && ew_grid(0) == 1);
  CHECK(aligned16(kAligned, (uintptr_t)0, kAligned) && !aligned16(kAligned, kOff4) && !aligned16(kAligned + 8));
  const float *null = nullptr;
  CHECK(aligned16(null, kAligned));                                        // pointers and integers alike
}

struct LdsCase {
  const char *name;
  int H, W, C, N, sy, sx, pt, pb, pl, pr;
  // expected: output size, 4096 / H, the plan, lead of planes 0 .. 5, tail load in the last block
  int Ho, Wo, maxcols;
  bool run;
  int groups, wob, ncols, lead[6];
  bool tail;
};
static const LdsCase kLdsCases[] = {
    {"a", 35, 33, 3, 2, 2, 2, 0, 0, 0, 0, 17, 16, 117, true, 1, 16, 33, {0, 3, 2, 1, 0, 3}, true},
    {"b", 34, 34, 2, 2, 2, 2, 0, 1, 0, 1, 17, 17, 120, true, 1, 17, 35, {0, 0, 0, 0, 0, 0}, false},
    {"c", 20, 18, 4, 2, 1, 1, 1, 1, 1, 1, 20, 18, 204, true, 1, 18, 20, {0, 0, 0, 0, 0, 0}, false},
    {"d", 31, 15, 3, 2, 2, 1, 2, 2, 2, 2, 17, 17, 132, true, 1, 17, 19, {0, 1, 2, 3, 0, 1}, true},
    {"e", 200, 52, 2, 2, 2, 2, 0, 0, 0, 0, 99, 25, 20, true, 3, 9, 19, {0, 0, 0, 0, 0, 0}, false},
    {"f", 60, 80, 2, 2, 3, 4, 0, 0, 0, 0, 20, 20, 68, true, 2, 10, 39, {0, 0, 0, 0, 0, 0}, false},
    {"g1", 1365, 3, 3, 2, 2, 2, 0, 0, 0, 0, 682, 1, 3, true, 1, 1, 3, {0, 3, 2, 1, 0, 3}, true},
    {"g2", 1366, 3, 3, 2, 2, 2, 0, 0, 0, 0, 682, 1, 2, false, 0, 0, 0, {0, 0, 0, 0, 0, 0}, false},
    {"g3", 700, 9, 3, 2, 2, 2, 0, 0, 0, 0, 349, 4, 5, false, 0, 0, 0, {0, 0, 0, 0, 0, 0}, false},
};

static void check_lds_figures() {
  for (const LdsCase &c : kLdsCases) {
    g_case = c.name;
    const PoolGeo g = geo_of(c.H, c.W, 3, 3, c.sy, c.sx, c.pt, c.pb, c.pl, c.pr);
    const int planes = c.C * c.N;
    const size_t total = (size_t)c.H * c.W * planes;
    CHECK(g.Ho == c.Ho && g.Wo == c.Wo && 4096 / c.H == c.maxcols && g.Ho * g.Wo >= 256);
    CHECK(!pool_is_global(g, false, false));
    CHECK(!pool_lds_plan(g, true, kOff4).run && !pool_lds_plan(g, false, kAligned).run);   // unaligned x; average pooling
    const PoolLds p = pool_lds_plan(g, true, kAligned);
    CHECK(p.run == c.run);
    if (!p.run) continue;
    CHECK(p.groups == c.groups && p.wob == c.wob && p.ncols == c.ncols && p.ncols <= c.maxcols);
    CHECK(p.lds_bytes == ((size_t)c.ncols * c.H + 8) * 4);
    for (int plane = 0; plane < planes; ++plane)
      for (int grp = 0; grp < p.groups; ++grp) {
        const LdsBlock b = lds_block(g, p, plane, grp, total);
        CHECK(plane >= 6 || b.lead == c.lead[plane]);
        CHECK(b.cols <= p.ncols && (size_t)b.cols * c.H + b.lead <= (size_t)p.ncols * c.H + 8);
        CHECK(b.tail == (c.tail && plane == planes - 1 && grp == p.groups - 1));
      }
  }
  g_case = "e";   // groups of 9, 9 and 7 columns over input columns 0, 18, 36 (runs of 19, 19 and 15)
  {
    const PoolGeo g = geo_of(200, 52, 3, 3, 2, 2);
    const PoolLds p = pool_lds_plan(g, true, kAligned);
    const int wlo[3] = {0, 18, 36}, cols[3] = {19, 19, 15}, nwo[3] = {9, 9, 7};
    for (int grp = 0; grp < 3; ++grp) {
      const LdsBlock b = lds_block(g, p, 0, grp, (size_t)200 * 52 * 4);
      CHECK(b.wlo == wlo[grp] && b.cols == cols[grp] && std::min(p.wob, g.Wo - grp * p.wob) == nwo[grp]);
    }
  }
  g_case = "f";   // wob 17 before the groups are evened out; input columns 0 and 40
  {
    const PoolGeo g = geo_of(60, 80, 3, 3, 3, 4);
    const PoolLds p = pool_lds_plan(g, true, kAligned);
    CHECK((68 - 3) / 4 + 1 == 17 && p.groups == (20 + 16) / 17);
    CHECK(lds_block(g, p, 0, 0, 60 * 80 * 4).wlo == 0 && lds_block(g, p, 0, 1, 60 * 80 * 4).wlo == 40);
  }
  g_case = "g1";  // the tallest plane: 4095 + 8 floats of LDS
  CHECK(pool_lds_plan(geo_of(1365, 3, 3, 3, 2, 2), true, kAligned).lds_bytes == (4095 + 8) * 4);
}

static bool launch_is(const PoolLaunch &l, int bx, int by, int bz, int gx, int gy, int gz) {
  return l.bx == bx && l.by == by && l.bz == bz && l.gx == gx && l.gy == gy && l.gz == gz;
}

static void check_pool_figures() {
  g_case = "PLANE_STRIDE_SHAPE";   // (301, 41) x 120 planes, stride 1: gy < planes, a block strides over planes
  PoolGeo g = geo_of(301, 41, 2, 2, 1, 1);
  CHECK(g.Ho == 300 && g.Wo == 40 && launch_is(pool_launch(g.Ho, g.Wo, 120), 256, 1, 1, 40, 102, 2) && pool_cover_2x2(g));
  g = geo_of(301, 41, 5, 3, 1, 1);
  CHECK(g.Ho == 297 && g.Wo == 39 && launch_is(pool_launch(g.Ho, g.Wo, 120), 256, 1, 1, 39, 105, 2) && !pool_cover_2x2(g));
  g = geo_of(301, 41, 4, 3, 1, 1);
  CHECK(g.Ho == 298 && g.Wo == 39 && launch_is(pool_launch(g.Ho, g.Wo, 120), 256, 1, 1, 39, 105, 2) && !pool_cover_2x2(g));
  CHECK(launch_is(pool_launch(301, 41, 120), 256, 1, 1, 41, 99, 2));                   // backward: over the inputs
  g_case = "PACKED_SHAPE";         // (6, 6) x 32,781 planes: four planes per block, gy = 8192 < ceil(32781 / 4) = 8196
  g = geo_of(6, 6, 2, 2, 1, 1);
  CHECK(g.Ho == 5 && g.Wo == 5 && launch_is(pool_launch(5, 5, 32781), 8, 8, 4, 1, 8192, 1) && (32781 + 3) / 4 == 8196);
  CHECK(launch_is(pool_launch(6, 6, 32781), 8, 8, 4, 1, 8192, 1));
  g_case = "window limit";         // 15 x 17 / 1: the runtime-loop arm of the backward; 5 x 3 / (2, 1): refused by the fused one
  CHECK(!pool_cover_2x2(geo_of(16, 18, 15, 17, 1, 1)) && !pool_cover_2x2(geo_of(13, 9, 5, 3, 2, 1)));
  CHECK(pool_cover_2x2(geo_of(35, 33, 3, 3, 2, 2)) && pool_cover_2x2(geo_of(7, 6, 5, 3, 3, 2)));
  g_case = "GLOBAL_SHAPES";        // window = plane, no padding, no table
  const int gs[4][2] = {{7, 7}, {8, 8}, {1, 3}, {30, 30}};
  for (const int *s : gs) {
    g = geo_of(s[0], s[1], s[0], s[1], 1, 1);
    CHECK(pool_is_global(g, false, false) && !pool_is_global(g, true, false) && !pool_is_global(g, false, true));
  }
  CHECK(!pool_is_global(geo_of(8, 8, 8, 8, 1, 1, 1, 0, 0, 0), false, false));
}

static void check_fused_figures() {
  g_case = "SPLIT_CASES";
  // (6,6,1500,3) 3 x 3 / 2: S = 4096 / 1500 = 2 < 3 in the element kernels; apply by the patch kernel <2, 2, true>, pS = 3
  BnPoolBwd p = bnpool_bwd_plan(geo_of(6, 6, 3, 3, 2, 2), 1500, 3, kAligned, kAligned, false);
  CHECK(p.gx == 1 && p.gz == 1 && p.pgx == 1 && p.pgz == 1 && p.S == 2 && p.patch_can && p.vec2 && p.pS == 3 && !p.pooled_can);
  CHECK(p.npart(false) == 2 && p.npart2(true) == 3 && p.npart2(false) == 2);
  // ... 2 x 2 / 1, pad (1,0,1,0): no patch kernel, bnpool_bwd_apply_kernel with S = 2
  p = bnpool_bwd_plan(geo_of(6, 6, 2, 2, 1, 1, 1, 0, 1, 0), 1500, 3, kAligned, kAligned, false);
  CHECK(p.S == 2 && !p.patch_can && !p.vec2);
  // (6,6,6000,3): pS = 16384 / 6000 = 2 < 3, S = 1; <2, 2, true>: H and pt even
  p = bnpool_bwd_plan(geo_of(6, 6, 3, 3, 2, 2), 6000, 3, kAligned, kAligned, false);
  CHECK(p.S == 1 && p.pS == 2 && p.patch_can && p.vec2 && p.KH == 3 && p.KW == 3);
  CHECK(!bnpool_bwd_plan(geo_of(6, 6, 3, 3, 2, 2), 6000, 3, kOff4, kAligned, false).vec2);   // 4-byte aligned x: <2, 2, false>
  CHECK(!bnpool_bwd_plan(geo_of(6, 6, 3, 3, 2, 2), 6000, 3, kAligned, 0, false).patch_can);  // no dx: nothing to apply
  // (7,6,6000,3): odd H -> <2, 2, false>
  p = bnpool_bwd_plan(geo_of(7, 6, 3, 3, 2, 2), 6000, 3, kAligned, kAligned, false);
  CHECK(p.pS == 2 && p.patch_can && !p.vec2 && p.KH == 4 && p.KW == 3);
  // (7,6,6000,3) 5 x 3 / (3, 2) -> <3, 2, false>, KH = KW = 3
  p = bnpool_bwd_plan(geo_of(7, 6, 5, 3, 3, 2), 6000, 3, kAligned, kAligned, false);
  CHECK(p.pS == 2 && p.patch_can && !p.vec2 && p.KH == 3 && p.KW == 3);
  // (6,6,700,3) with y_pool: S2 = 2048 / 700 = 2 < 3 in bnpool_bwd_partial_pooled_kernel
  p = bnpool_bwd_plan(geo_of(6, 6, 3, 3, 2, 2), 700, 3, kAligned, kAligned, true);
  CHECK(p.pooled_can && p.S2 == 2 && p.npart(true) == 2 && p.npart(false) == 3);
}

// ---- 2. invariants over a sweep ----------------------------------------------------------------------------------------
static void check_ws(const BnWs &w, size_t npart, bool backward, size_t npart2, bool mom, int C) {
  const size_t c = (size_t)C;
  CHECK(w.part.count == 2 * c * npart && w.sums.count == (backward ? 2 * c : 0) && w.part2.count == c * npart2 &&
        w.mom.count == (mom ? 2 * c : 0));
  size_t sum = 0;
  const size_t bytes[4] = {w.part.count * 8, w.sums.count * 8, w.part2.count * 8, w.mom.count * 4};
  for (size_t b : bytes) sum += (b + 255) / 256 * 256;      // a segment that is not taken has no bytes
  CHECK(w.bytes() == sum && ws_bytes(w.part) % 256 == 0 && ws_bytes(w.part) >= bytes[0] && ws_bytes(w.part) < bytes[0] + 256);
  CHECK(ws_bytes(WsSeg<unsigned char>{0}) == 0 && ws_bytes(WsSeg<unsigned char>{257}) == 512);
}

static void check_launch(int rows, int cols, long long planes) {
  const PoolLaunch l = pool_launch(rows, cols, planes);
  CHECK(l.bx * l.by * l.bz == 256);
  CHECK(l.gz * l.bx >= rows && (l.gz - 1) * l.bx < rows && l.gx * l.by >= cols && (l.gx - 1) * l.by < cols);
  CHECK(l.gy >= 1 && l.gy <= 65535 && (long long)(l.gy - 1) * l.bz < planes);   // no block row without a plane
  ++g_checked;
}

static const int kCs[] = {1, 3, 8, 300, 600, 1500, 4100, 6000}, kNs[] = {1, 2, 3, 9, 70};

static void check_geometry(const PoolGeo &g) {
  for (long long planes : {1LL, 6LL, 120LL, 32781LL, 65536LL, 1LL << 24}) {
    check_launch(g.Ho, g.Wo, planes);
    check_launch(g.H, g.W, planes);
  }
  for (int max_pool = 0; max_pool < 2; ++max_pool) {
    CHECK(!pool_lds_plan(g, max_pool, kOff4).run);
    const PoolLds p = pool_lds_plan(g, max_pool, kAligned);
    ++g_checked;
    if (!p.run) continue;
    CHECK(max_pool && g.ph == 3 && g.pw == 3 && g.Ho * g.Wo >= 256);
    CHECK(p.wob >= 1 && p.groups >= 1 && p.groups * p.wob >= g.Wo && (p.groups - 1) * p.wob < g.Wo);
    CHECK(p.ncols == (p.wob - 1) * g.sx + g.pw && p.ncols * g.H <= 4096);
    CHECK(p.lds_bytes == ((size_t)p.ncols * g.H + 8) * 4 && p.lds_bytes <= 16384 + 32);
    for (int grp = 0; grp < p.groups; ++grp) {   // every block's run, with its lead, fits the tile
      const LdsBlock b = lds_block(g, p, 1, grp, (size_t)g.H * g.W * 2);
      CHECK(b.cols >= 1 && b.cols <= p.ncols && (size_t)(b.cols * g.H + b.lead + 3) / 4 * 4 <= p.lds_bytes / 4);
    }
  }
  for (int C : kCs)
    for (int N : kNs) {
      const BnPoolBwd p = bnpool_bwd_plan(g, C, N, kAligned, kAligned, true);
      CHECK(p.bx * p.by <= 256 && p.gz * p.bx >= g.H && p.gx * p.by >= g.W && (p.gz - 1) * p.bx < g.H && (p.gx - 1) * p.by < g.W);
      CHECK(p.pbx * p.pby <= 256 && p.pgz * p.pbx >= p.KH && p.pgx * p.pby >= p.KW);
      CHECK(p.KH * g.sy >= g.H + g.pt && p.KW * g.sx >= g.W + g.pl);            // the stride cells cover every element
      CHECK(p.S >= 1 && p.S <= N && p.pS >= 1 && p.pS <= N && p.S2 >= 1 && p.S2 <= N && p.S2 == bn_splits(C, N));
      CHECK(p.patch_can == ((g.sy == 2 || g.sy == 3) && g.sx == 2) && (!p.vec2 || (g.sy == 2 && g.H % 2 == 0 && g.pt % 2 == 0)));
      CHECK(p.npart(false) == (size_t)p.gx * p.gz * p.S && p.npart2(true) == (size_t)p.pgx * p.pgz * p.pS);
      for (int f = 0; f < 8; ++f) {   // pooled, patch, dxsum
        const size_t np = p.npart(f & 1), np2 = (f & 4) ? p.npart2(f & 2) : 0;
        check_ws(bn_ws(C, np, true, np2, false), np, true, np2, false, C);
      }
      ++g_checked;
    }
}

static void check_sweep() {
  g_case = "sweep";
  for (int C : kCs)
    for (int N : kNs) {
      const int S = bn_splits(C, N), S2 = bn_dxsum_splits(C, N);
      CHECK(S >= 1 && S <= N && S2 >= 1 && S2 <= N && S <= S2 && (long long)C * S <= std::max(2048, C));
      for (int f = 0; f < 8; ++f) {   // moments given, moments wanted back, dxsum
        const bool in = f & 1, out = f & 2, dxsum = f & 4;
        check_ws(bn_ws(C, in ? 0 : S, false, 0, !in && !out), in ? 0 : S, false, 0, !in && !out, C);            // forward
        check_ws(bn_ws(C, S, true, dxsum ? S2 : 0, !in && !out), S, true, dxsum ? S2 : 0, !in && !out, C);      // backward
      }
      ++g_checked;
    }
  for (size_t n : {(size_t)0, (size_t)1, (size_t)256, (size_t)257, (size_t)524288, (size_t)524289, (size_t)1 << 31}) {
    const unsigned b = ew_grid(n);
    CHECK(b >= 1 && b <= 2048 && (b == 2048 || (size_t)b * 256 >= n));
    ++g_checked;
  }
  // windows, strides and pads of the tests (+ the whole plane: global pooling)
  const int win[][2] = {{2, 2}, {3, 3}, {5, 3}, {4, 3}, {15, 17}, {0, 0}}, str[][2] = {{1, 1}, {2, 2}, {2, 1}, {3, 4}, {3, 2}};
  const int pad[][4] = {{0, 0, 0, 0}, {1, 1, 1, 1}, {2, 2, 2, 2}, {0, 1, 0, 1}, {1, 0, 1, 0}};
  const int tall[][2] = {{200, 52}, {301, 41}, {700, 9}, {1365, 3}, {1366, 3}, {4096, 3}, {4097, 4}};
  for (int i = 0; i < 70 * 70 + 7; ++i) {
    const int H = i < 4900 ? 1 + i / 70 : tall[i - 4900][0], W = i < 4900 ? 1 + i % 70 : tall[i - 4900][1];
    for (const int *w : win)
      for (const int *s : str)
        for (const int *p : pad) {
          PoolGeo g{};
          if (!geo(g, H, W, w[0] ? w[0] : H, w[1] ? w[1] : W, s[0], s[1], p[0], p[1], p[2], p[3])) continue;
          CHECK(pool_is_global(g, false, false) == (g.ph >= H && g.pw >= W && !p[0] && !p[2] && g.Ho == 1 && g.Wo == 1));
          CHECK(pool_cover_2x2(g) == (g.ph <= 2 * g.sy && g.pw <= 2 * g.sx));
          check_geometry(g);
        }
  }
}

int main() {
  check_bnorm_figures();
  check_lds_figures();
  check_pool_figures();
  check_fused_figures();
  check_sweep();
  std::printf("%ld plans checked\n", g_checked);
  return 0;
}

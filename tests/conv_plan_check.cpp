// Stand-alone check of csrc/conv_plan.h (no HIP, no GPU): tests/test_conv_plan_cpu.py builds and runs it.
//   1. dgrad planning against the definition of the convolution, brute force over a grid of small geometries;
//   2. the "can run" predicates on the layers of the shipped networks, and on single-field changes of them.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../mcncrossmodalemotions_amd/csrc/conv_plan.h"

using namespace xm;

static long g_checked = 0;
#define CHECK(cond, g)                                                                                              \
  do {                                                                                                              \
    if (!(cond)) {                                                                                                  \
      std::printf("FAILED %s (line %d): X %dx%d F %dx%d stride %d,%d dilate %d,%d pad %d %d %d %d\n", #cond, __LINE__, \
                  (g).H, (g).W, (g).FH, (g).FW, (g).sy, (g).sx, (g).dy, (g).dx, (g).pt, (g).pb, (g).pl, (g).pr);      \
      std::exit(1);                                                                                                 \
    }                                                                                                               \
  } while (0)

// the geometry as the library's make_geo derives it; false when the filter does not fit the padded input
static bool geo(Geo &g, int H, int W, int C, int N, int FH, int FW, int FC, int K, int sy, int sx, int pt, int pb, int pl,
                int pr, int dy, int dx) {
  const int th = H + pt + pb - ((FH - 1) * dy + 1), tw = W + pl + pr - ((FW - 1) * dx + 1);
  if (th < 0 || tw < 0) return false;
  g = Geo{H, W, C, N, FH, FW, FC, K, C / FC, K / (C / FC), th / sy + 1, tw / sx + 1, FH * FW * FC, sy, sx, pt, pb, pl, pr, dy, dx};
  return true;
}

// ---- 1. dgrad planning -----------------------------------------------------------------------------------------------
// one counter per (input pixel, output pixel, tap, filter): + 1 by the forward definition, - 1 through classes and tables
static std::vector<int> g_count;
static size_t key_of(const Geo &g, int hi, int wi, int ho, int wo, int u, int v, int k) {
  return (((((size_t)hi * g.W + wi) * g.Ho + ho) * g.Wo + wo) * g.FH * g.FW + u + g.FH * v) * g.K + k;
}

static void check_dgrad(const Geo &g) {
  const bool foldH = dgrad_fold_h(g);
  CHECK(!foldH || (g.Ho == 1 && g.FH == g.H), g);                                                    // (iv)
  bool covers_all = true;
  const std::vector<DgradClass> cls = dgrad_classes(g, foldH, &covers_all);
  // (i) every input pixel in exactly one enumerated class, or in none and then its parity class has no tap
  bool uncovered = false, tapsU[3] = {false, false, false}, tapsV[3] = {false, false, false};   // parity has a tap
  for (int u = 0; u < g.FH; ++u) tapsU[(u * g.dy) % g.sy] = true;
  for (int v = 0; v < g.FW; ++v) tapsV[(v * g.dx) % g.sx] = true;
  for (int wi = 0; wi < g.W; ++wi)
    for (int hi = 0; hi < g.H; ++hi) {
      int in = 0;
      for (const DgradClass &c : cls) {
        const int di = hi - c.hi0, dj = wi - c.wi0;
        in += di >= 0 && di % g.sy == 0 && di / g.sy < c.PI && dj >= 0 && dj % g.sx == 0 && dj / g.sx < c.PJ;
      }
      CHECK(in == ((tapsU[(hi + g.pt) % g.sy] && tapsV[(wi + g.pl) % g.sx]) ? 1 : 0), g);
      uncovered = uncovered || in == 0;
    }
  CHECK(covers_all == !uncovered, g);
  // (ii) forward definition ...
  long forward = 0, backward = 0;
  for (int k = 0; k < g.K; ++k)
    for (int wo = 0; wo < g.Wo; ++wo)
      for (int ho = 0; ho < g.Ho; ++ho)
        for (int v = 0; v < g.FW; ++v)
          for (int u = 0; u < g.FH; ++u) {
            const int hi = ho * g.sy - g.pt + u * g.dy, wi = wo * g.sx - g.pl + v * g.dx;
            if (hi < 0 || hi >= g.H || wi < 0 || wi >= g.W) continue;
            ++g_count[key_of(g, hi, wi, ho, wo, u, v, k)];
            ++forward;
          }
  // ... against the classes, decoded with the addressing of the GEMM arguments
  for (const DgradClass &c : cls) {
    CHECK(c.Rc == (foldH ? c.nV : c.nU * c.nV) * g.Kg && c.Rp % kBK == 0 && c.Rp >= c.Rc && c.Rp - c.Rc < kBK, g);   // (v)
    const DgradGather q = dgrad_gather(g, c, foldH);
    const std::vector<Tap2> t = dgrad_tap_table(g, c, foldH);
    CHECK((int)t.size() == c.Rp + 3 * kBK, g);
    for (size_t r = c.Rc; r < t.size(); ++r) CHECK(t[r].off == 0 && t[r].uv == 63, g);                // (iii)
    const int rows = foldH ? g.FH : 1, PI = foldH ? 1 : c.PI;     // foldH: GEMM row m carries filter row m % FH
    for (int row = 0; row < rows; ++row)
      for (int j = 0; j < c.PJ; ++j)
        for (int i = 0; i < PI; ++i)
          for (int r = 0; r < c.Rc; ++r) {
            const int iu = t[r].uv % q.nU, iv = t[r].uv / q.nU, k = r / (q.nU * c.nV);
            CHECK(iu < q.nU && iv < c.nV && k < g.Kg, g);
            const int du = q.du0 + iu * q.dus, dv = q.dv0 + iv * q.dvs;
            CHECK(t[r].off == 4 * (du + g.Ho * dv + g.Ho * g.Wo * k), g);
            const int ho = i + q.gh0 + du, wo = j + q.gw0 + dv;      // source row = class row + du0 + iu dus, ...
            if (ho < 0 || ho >= g.Ho || wo < 0 || wo >= g.Wo) continue;   // masked by the gather's bounds
            const int hi = foldH ? row : c.hi0 + i * g.sy, wi = c.wi0 + j * g.sx;
            const int u = foldH ? row : c.u0 + iu * c.ustep, v = c.v0 + iv * c.vstep;
            CHECK(hi >= 0 && hi < g.H && wi >= 0 && wi < g.W && u >= 0 && u < g.FH && v >= 0 && v < g.FW, g);
            CHECK(--g_count[key_of(g, hi, wi, ho, wo, u, v, k)] >= 0, g);
            ++backward;
          }
  }
  CHECK(forward == backward, g);     // every counter is back at zero: the multisets are equal
  ++g_checked;
}

static void sweep() {
  const int sizes[] = {1, 4, 5, 9, 12}, taps[] = {1, 2, 3, 5, 7}, pads[] = {0, 1, 3};
  g_count.assign((size_t)12 * 12 * 18 * 18 * 49 * 2, 0);
  Geo g;
  for (int H : sizes) for (int W : sizes) for (int FH : taps) for (int FW : taps)
    for (int sy = 1; sy <= 3; ++sy) for (int sx = 1; sx <= 3; ++sx) for (int d = 1; d <= 2; ++d)
      for (int pt : pads) for (int pb : pads) for (int pl : pads) for (int pr : pads)
        if (geo(g, H, W, 1, 1, FH, FW, 1, 2, sy, sx, pt, pb, pl, pr, d, d)) check_dgrad(g);
}

// ---- 2. the layers of the shipped networks (oracle/graphs.py) --------------------------------------
static int g_failed = 0;
static void expect(bool got, bool want, const char *what) {
  if (got != want) {
    std::printf("FAILED: %s is %s\n", what, got ? "accepted" : "rejected");
    ++g_failed;
  }
}
#define ACCEPT(e) expect((e), true, #e)
#define REJECT(e) expect((e), false, #e)

static Geo layer(int H, int W, int C, int FH, int FW, int K, int s, int p) {
  Geo g;
  if (!geo(g, H, W, C, 32, FH, FW, C, K, s, s, p, p, p, p, 1, 1)) std::exit(2);
  return g;
}

static void real_layers() {
  const uintptr_t x = 0x7f0000001000, y = 0x7f0000801000;     // 4 KiB aligned, as the allocator hands them out
  // student conv1: 512 x 300 x 1, 7 x 7 / 2, pad 1, 96 filters
  for (int change = 0; change < 6; ++change) {
    int H = 512, C = 1, FW = 7;
    uintptr_t xp = x;
    if (change == 1) C = 2;
    if (change == 2) H = 511;       // odd
    if (change == 3) H = 510;       // even, no multiple of 4
    if (change == 4) xp = x + 4;    // not 16-byte aligned
    if (change == 5) FW = 8;        // one filter column too many
    const Geo g = layer(H, 300, C, 7, FW, 96, 2, 1);
    expect(stem_fwd_can(g, xp, kEpiVecStore), change == 0, "student conv1: stem_fwd_can");
    expect(stem_fwd_can(g, xp, kEpiVecStore | kEpiStats), change == 0, "student conv1 + statistics: stem_fwd_can");
    expect(stem_wgrad_can(g, xp, y), change == 0, "student conv1: stem_wgrad_can");
    expect(stem_pool_can(g, xp), change == 0, "student conv1: stem_pool_can");
  }
  const Geo c1 = layer(512, 300, 1, 7, 7, 96, 2, 1);
  REJECT(stem_fwd_can(c1, x, kEpiVecStore | kEpiRelu));
  REJECT(stem_fwd_can(c1, x, 0));
  REJECT(stem_wgrad_can(c1, x, y + 8));
  // ... and its fused bnorm + relu + 3 x 3 / 2 max-pool: 254 x 148 -> 126 x 73
  ACCEPT(fused_stem_can(kFusedStemForward, c1, x, 3, 3, 2, 2, 0, 0, 0, 0, 126, 73, y));
  ACCEPT(fused_stem_can(kFusedStemBackward, c1, x, 3, 3, 2, 2, 0, 0, 0, 0, 126, 73, y));
  REJECT(fused_stem_can(kFusedStemForward, c1, x, 3, 3, 2, 2, 0, 1, 0, 1, 127, 74, y));
  REJECT(fused_stem_can(kFusedStemBackward, c1, x, 3, 3, 2, 2, 0, 0, 0, 0, 126, 73, y + 2));
  ACCEPT(fused_stem_can(kFusedStemForward, c1, x, 3, 3, 2, 2, 0, 0, 0, 0, 3, 73, y));      // the two directions differ on
  REJECT(fused_stem_can(kFusedStemBackward, c1, x, 3, 3, 2, 2, 0, 0, 0, 0, 3, 73, y));     // fewer than four pooled rows
  ACCEPT(pool3x3s2_unpadded(3, 3, 2, 2, 0, 0, 0, 0));
  REJECT(pool3x3s2_unpadded(3, 3, 2, 1, 0, 0, 0, 0));
  // student conv2: 126 x 73 x 96, 5 x 5 / 2, pad 1, 256 filters (these kernels take any channel count: no C = 2 case)
  for (int change = 0; change < 4; ++change) {
    int H = 126, FH = 5;
    uintptr_t xp = x;
    if (change == 1) H = 125;       // odd
    if (change == 2) xp = x + 4;    // not 8-byte aligned
    if (change == 3) FH = 6;        // one filter row too many
    const Geo g = layer(H, 73, 96, FH, 5, 256, 2, 1);
    expect(dgrad_s2_can(g, y, xp, false), change == 0, "student conv2: dgrad_s2_can");
    expect(wgrad_patch_s2_can(g, xp, y), change == 0, "student conv2: wgrad_patch_s2_can");
  }
  REJECT(dgrad_s2_can(layer(126, 73, 96, 5, 5, 256, 2, 1), y, x, true));
  // student conv3: 30 x 17 x 256, 3 x 3, pad 1, 384 filters
  for (int change = 0; change < 4; ++change) {
    int H = 30, FH = 3;
    uintptr_t xp = x;
    if (change == 1) H = 31;
    if (change == 2) xp = x + 4;
    if (change == 3) FH = 4;
    expect(wgrad_patch_can(layer(H, 17, 256, FH, 3, 384, 1, 1), xp, y), change == 0, "student conv3: wgrad_patch_can");
  }
  // teacher conv1: 224 x 224 x 3, 7 x 7 / 2, pad 3, 64 filters
  for (int change = 0; change < 5; ++change) {
    int H = 224, C = 3, FH = 7;
    uintptr_t xp = x;
    if (change == 1) C = 2;
    if (change == 2) H = 225;
    if (change == 3) xp = x + 4;
    if (change == 4) FH = 8;
    expect(stem3_can(layer(H, 224, C, FH, 7, 64, 2, 3), xp, kEpiVecStore | kEpiScale | kEpiRelu), change == 0,
           "teacher conv1: stem3_can");
  }
  REJECT(stem3_can(layer(224, 224, 3, 7, 7, 64, 2, 3), x, kEpiVecStore | kEpiStats));
  // 2 GiB: 2^29 floats do not fit 32-bit byte offsets
  ACCEPT(fits_i32_bytes(((size_t)1 << 29) - 1));
  REJECT(fits_i32_bytes((size_t)1 << 29));
}

int main() {
  sweep();
  real_layers();
  std::printf("%ld geometries, %d predicate failures\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}

// csrc/imread_plan.h alone (no HIP), built with -fsanitize=address,undefined and run as a program by
// tests/test_imread_aug_cpu.py: over a sweep of image sizes, output sizes, filters, antialias, crop locations and the
// anisotropy and size ranges it checks that every window lies inside its image, that the weights of every output sample
// sum to 1 within 1e-12 and cover the kernel's whole support, that every tap is within the support's reach of the image
// and clamps into it, and that the LDS row tiling fits its budget: no chunk of output rows needs more source rows than
// the tile holds.  Prints "<plans> <images> <samples> <chunks> <most rows in a chunk> <refusals>".
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../mcncrossmodalemotions_amd/csrc/imread_plan.h"

using namespace xm;

static uint64_t g_state = 88172645463325252ULL;
static double uniform() {   // xorshift64, in [0, 1)
  g_state ^= g_state << 13;
  g_state ^= g_state >> 7;
  g_state ^= g_state << 17;
  return (double)(g_state >> 11) / 9007199254740992.0;
}

#define CHECK(cond, ...)                        \
  do {                                          \
    if (!(cond)) {                              \
      fprintf(stderr, "FAILED %s: ", #cond);    \
      fprintf(stderr, __VA_ARGS__);             \
      fprintf(stderr, "\n");                    \
      exit(1);                                  \
    }                                           \
  } while (0)

static long long g_samples = 0, g_chunks = 0, g_maxrows = 0;

// one axis of one image: n inputs, m outputs, window (c0, len)
static void check_axis(int filter, int n, int m, double c0, double len, double r, double s, int T, bool flip, bool tiled, int oc) {
  CHECK(c0 >= -1e-9 && c0 + len <= n + 1e-9, "window %g + %g in %d", c0, len, n);
  CHECK(T == imread_tap_count(filter, s) && T >= 2 && T <= 257, "T %d", T);
  std::vector<double> w((size_t)T);
  std::vector<int> first((size_t)m);
  const double S = imread_support(filter);
  for (int o = 0; o < m; ++o) {
    const int op = flip ? m - 1 - o : o;
    first[o] = imread_taps(filter, c0, r, s, T, op, w.data(), 1);
    const double u = c0 + (op + 0.5) * r - 0.5;
    double sum = 0;
    for (int t = 0; t < T; ++t) {
      sum += w[t];
      const int idx = std::min(std::max(first[o] + t, 0), n - 1);
      CHECK(idx >= 0 && idx < n, "index %d of %d", idx, n);
    }
    CHECK(std::fabs(sum - 1) <= 1e-12, "weights sum to %.17g", sum);
    // (a box edge that falls on a sample in exact arithmetic may round to either side of 1/2: the tap list decides)
    const double below = ((first[o] - 1) - u) / s, above = ((first[o] + T) - u) / s;
    const bool tie = filter == XM_IMREAD_BOX && (std::fabs(std::fabs(below) - 0.5) < 1e-9 || std::fabs(std::fabs(above) - 0.5) < 1e-9);
    // (and an edge of a continuous kernel that falls on a sample may leave it a weight of the order of the rounding)
    CHECK(tie || (std::fabs(imread_kernel_value(filter, below)) <= 1e-12 && std::fabs(imread_kernel_value(filter, above)) <= 1e-12),
          "filter %d: taps %d .. %d do not cover the support of width %g around %.17g (%.17g, %.17g)", filter, first[o], first[o] + T - 1,
          S * s, u, below, above);
    CHECK(first[o] >= -(int)std::ceil(S * s / 2) - 1 && first[o] + T - 1 <= n + (int)std::ceil(S * s / 2) + 1, "tap range %d + %d of %d",
          first[o], T, n);
    ++g_samples;
  }
  if (!tiled) return;
  CHECK(oc >= 1 && oc <= m && oc == imread_chunk_rows(r, T, m), "chunk of %d rows", oc);
  for (int oa = 0; oa < m; oa += oc) {
    const int ob = std::min(oa + oc, m);
    const int rows = first[ob - 1] + T - first[oa];
    CHECK(rows >= T && rows <= kImreadTileRows, "a chunk of %d source rows, the tile holds %d", rows, kImreadTileRows);
    for (int o = oa; o < ob; ++o) CHECK(first[o] >= first[oa] && first[o] + T - first[oa] <= rows, "rows not monotone");
    g_maxrows = std::max<long long>(g_maxrows, rows);
    ++g_chunks;
  }
}

int main() {
  static_assert(kImreadTileRows * kImreadTW * 3 * (int)sizeof(float) <= kImreadTileBytes, "tile bytes");
  static_assert(kImreadTileBytes <= kImreadLdsPerWorkgroup && kImreadLdsPerWorkgroup == 160 * 1024, "LDS of a workgroup");
  static_assert(3 * 256 <= kImreadTileRows * kImreadTW * 3, "the block sums reuse the tile");
  const int Hs[] = {1, 2, 3, 17, 37, 300, 2000, 4096}, Ws[] = {1, 3, 23, 53, 200};
  const double outs[][3] = {{1, 1, 1}, {1, 5, 7}, {1, 16, 20}, {2, 8, 0}, {0, 0, 0}, {1, 64, 80}};
  const double ranges[][4] = {{0, 0, 1, 1}, {0.75, 1.3333333333333333, 0.35, 1}, {1, 1, 0.625, 0.625}};
  long long plans = 0, images = 0, refusals = 0;
  char msg[256];
  std::vector<long long> hw;
  for (int H : Hs)
    for (int W : Ws) {
      hw.push_back(H), hw.push_back(W), hw.push_back((long long)hw.size() * 1000);
    }
  const int N = (int)hw.size() / 3;
  std::vector<double> rows((size_t)N * XM_IMREAD_ROW), draws((size_t)N * XM_IMREAD_DRAWS);
  for (const auto &out : outs)
    for (int filter = 0; filter < 3; ++filter)
      for (int aa = 0; aa < 2; ++aa)
        for (int loc = 0; loc < 2; ++loc)
          for (const auto &rg : ranges)
            for (int flip = 0; flip < 2; ++flip) {
              double opts[XM_IMREAD_OPTS] = {0};
              opts[IO_RESIZE] = out[0], opts[IO_HO] = out[1], opts[IO_WO] = out[2];
              opts[IO_AMIN] = rg[0], opts[IO_AMAX] = rg[1], opts[IO_SMIN] = rg[2], opts[IO_SMAX] = rg[3];
              opts[IO_RANDOM] = loc, opts[IO_FLIP] = flip, opts[IO_FILTER] = filter, opts[IO_AA] = aa;
              opts[IO_CONTRAST] = 0.4, opts[IO_SATURATION] = 0.3, opts[IO_BRIGHT] = 2, opts[IO_BRIGHT + 4] = 3, opts[IO_BRIGHT + 8] = 1;
              for (auto &v : draws) v = uniform();
              for (int i = 0; i < N; ++i) {   // image by image: a refusal of one (a ratio above 64) must not hide the others
                long long sizes[XM_IMREAD_SIZES];
                const int rc = imread_plan_batch(&hw[3 * (size_t)i], 1, opts, &draws[(size_t)i * XM_IMREAD_DRAWS], rows.data(), sizes, msg,
                                                 (int)sizeof msg);
                ++plans;
                if (rc == XM_ENOTSUP) {
                  ++refusals;
                  continue;
                }
                CHECK(rc == XM_OK, "plan: %s", msg);
                const double *d = rows.data();
                const int H = (int)d[IR_H], W = (int)d[IR_W], Ho = (int)d[IR_HO], Wo = (int)d[IR_WO];
                CHECK(H == hw[3 * (size_t)i] && W == hw[3 * (size_t)i + 1] && Ho >= 1 && Wo >= 1, "sizes");
                CHECK(d[IR_RY] <= kImreadMaxRatio && d[IR_RX] <= kImreadMaxRatio, "ratio");
                CHECK(sizes[IS_OUT] == 3LL * Ho * Wo && sizes[IS_TABLE] == (long long)Ho * (int)d[IR_TY] + (long long)Wo * (int)d[IR_TX] + Ho + Wo,
                      "sizes of image %d", i);
                CHECK(sizes[IS_PART] == 3 * (long long)d[IR_TILES] && (long long)d[IR_TILES] == (Wo + kImreadTW - 1) / kImreadTW, "tiles");
                check_axis(filter, H, Ho, d[IR_Y0], d[IR_CH], d[IR_RY], d[IR_SY], (int)d[IR_TY], false, true, (int)d[IR_OC]);
                check_axis(filter, W, Wo, d[IR_X0], d[IR_CW], d[IR_RX], d[IR_SX], (int)d[IR_TX], d[IR_FLIP] != 0, false, 0);
                double rowsum[3] = {0, 0, 0};
                for (int c = 0; c < 3; ++c)
                  for (int k = 0; k < 3; ++k) rowsum[c] += d[IR_M + 3 * c + k];
                for (int c = 0; c < 3; ++c) CHECK(std::fabs(rowsum[c] - d[IR_GAMMA]) <= 1e-12, "colour matrix rows sum to gamma");
                ++images;
              }
            }
  printf("%lld %lld %lld %lld %lld %lld\n", plans, images, g_samples, g_chunks, g_maxrows, refusals);
  return 0;
}

// Host-side planning of vl.vl_imreadjpeg's crop / flip / filter / colour stage (xm_imread_plan): from the size of every
// decoded image, the options and the random draws to one row of XM_IMREAD_ROW doubles per image -- output size and
// offsets, crop window, flip, filter, tap counts, colour terms, the LDS row tiling -- and the tap weights of one output
// sample, the one routine the device's table kernel and the CPU check both call.  Arithmetic only, nothing from HIP
// (compiles with g++ -std=c++17; tests/imread_plan_check.cpp holds it to its invariants under the address and
// undefined-behaviour sanitizers).  include/xmodal.h documents the row and the options; DESIGN section 24 the semantics;
// csrc/imread_xform.hip holds the C entry points and the kernels.
#pragma once
#include <cmath>
#include <cstdarg>
#include <cstdio>

#include "../../include/xmodal.h"

#if defined(__HIPCC__)
#define XM_IMREAD_HD __host__ __device__
#else
#define XM_IMREAD_HD
#endif

namespace xm {

// row columns (XM_IMREAD_ROW doubles per image)
enum { IR_H = 0, IR_W, IR_PIX, IR_HO, IR_WO, IR_OUT, IR_Y0, IR_X0, IR_CH, IR_CW, IR_FLIP, IR_FILTER, IR_AA, IR_TY, IR_TX,
       IR_M = 15, IR_K = 24, IR_GAMMA = 27, IR_SIGMA = 28, IR_B = 29, IR_TAB = 32, IR_OC = 33, IR_RY = 34, IR_RX = 35,
       IR_SY = 36, IR_SX = 37, IR_TILES = 38, IR_PART = 39, IR_AVG = 40, IR_CONTRAST = 41 };
// option slots (XM_IMREAD_OPTS doubles)
enum { IO_RESIZE = 0, IO_HO, IO_WO, IO_AMIN, IO_AMAX, IO_SMIN, IO_SMAX, IO_RANDOM, IO_FLIP, IO_FILTER, IO_AA, IO_CONTRAST,
       IO_SATURATION, IO_BRIGHT = 13, IO_AVG = 22 };
// draw slots (XM_IMREAD_DRAWS doubles per image): u0 anisotropy, u1 size, u2 y, u3 x, u4 flip, u5 contrast,
// u6 saturation, g0..g2 brightness
enum { ID_ANISO = 0, ID_SIZE, ID_Y, ID_X, ID_FLIP, ID_CONTRAST, ID_SATURATION, ID_G = 7 };
// sizes slots (XM_IMREAD_SIZES int64)
enum { IS_OUT = 0, IS_TABLE, IS_PART, IS_MAXTILES, IS_CONTRAST, IS_UNIFORM, IS_MAXOUT, IS_N };

// A workgroup on gfx950 may allocate all 160 KiB of its CU's LDS; the resampling kernel takes kImreadTileBytes of it for
// the horizontally filtered rows of one tile (source rows x kImreadTW output columns x 3 channels), which leaves room
// for five workgroups per CU.  kImreadTileRows source rows fit; a window of more rows is walked in chunks of output rows.
constexpr int kImreadLdsPerWorkgroup = 163840;
constexpr int kImreadTileBytes = 32768;
constexpr int kImreadTW = 8;
constexpr int kImreadTileRows = kImreadTileBytes / (kImreadTW * 3 * 4);   // 341
constexpr double kImreadMaxRatio = 64.0;
constexpr int kImreadMaxSide = 32768;
static_assert(kImreadTileRows * kImreadTW * 3 * 4 <= kImreadTileBytes && kImreadTileBytes <= kImreadLdsPerWorkgroup, "LDS tile");

XM_IMREAD_HD inline double imread_support(int filter) { return filter == XM_IMREAD_BOX ? 1.0 : filter == XM_IMREAD_BILINEAR ? 2.0 : 4.0; }

XM_IMREAD_HD inline double imread_kernel_value(int filter, double t) {
  const double a = fabs(t);
  if (filter == XM_IMREAD_BOX) return (t > -0.5 && t <= 0.5) ? 1.0 : 0.0;
  if (filter == XM_IMREAD_BILINEAR) return a < 1.0 ? 1.0 - a : 0.0;
  if (a <= 1.0) return (1.5 * a - 2.5) * a * a + 1.0;          // Keys, a = -1/2
  if (a < 2.0) return ((-0.5 * a + 2.5) * a - 4.0) * a + 2.0;
  return 0.0;
}

// number of taps of an axis whose kernel is widened by s
XM_IMREAD_HD inline int imread_tap_count(int filter, double s) { return (int)ceil(imread_support(filter) * s) + 1; }

// the taps of output sample `oprime` (already mirrored on a flipped axis) of an axis with window start c0, ratio r and
// widening s: returns the first tap's index (unclamped) and writes the T weights, normalised in double and rounded once
// to float, to w[0], w[stride], ... (the CPU check asks for them in double, before that rounding)
template <class Wt>
XM_IMREAD_HD inline int imread_taps(int filter, double c0, double r, double s, int T, int oprime, Wt *w, long long stride) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double u = c0 + (oprime + 0.5) * r - 0.5;
  const int first = (int)floor(u - imread_support(filter) * s / 2) + 1;
  double sum = 0;
  for (int t = 0; t < T; ++t) sum += imread_kernel_value(filter, ((first + t) - u) / s);
  for (int t = 0; t < T; ++t) w[t * stride] = (Wt)(imread_kernel_value(filter, ((first + t) - u) / s) / sum);
  return first;
}

// output rows one LDS chunk may hold: the source rows of oc consecutive outputs span at most
// ceil((oc - 1) r) + T + 1 <= kImreadTileRows rows (the first taps of two outputs d apart differ by at most ceil(d r))
inline int imread_chunk_rows(double r, int T, int Ho) {
  const int room = kImreadTileRows - T - 1;
  if (room < 0) return 0;
  double oc = floor(room / r) + 1;
  while (oc > 1 && ceil((oc - 1) * r) + T + 1 > kImreadTileRows) oc -= 1;
  return oc > Ho ? Ho : (int)oc;
}

static inline int imread_fail(char *err, int errlen, int code, const char *fmt, ...) {
  if (err && errlen > 0) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, (size_t)errlen, fmt, ap);
    va_end(ap);
  }
  return code;
}

// hw: N x 3 int64 (H, W, offset of the H x W x 3 pixels in the ragged buffer, in floats).  opts: XM_IMREAD_OPTS doubles.
// draws: N x XM_IMREAD_DRAWS doubles, or NULL when no option is random.  rows: N x XM_IMREAD_ROW doubles.  sizes:
// XM_IMREAD_SIZES int64.
static inline int imread_plan_batch(const long long *hw, int N, const double *opts, const double *draws, double *rows,
                                    long long *sizes, char *err, int errlen) {
#define IBAD(...) return imread_fail(err, errlen, XM_EINVAL, __VA_ARGS__)
  if (!sizes) IBAD("imread_plan: NULL sizes");
  for (int k = 0; k < XM_IMREAD_SIZES; ++k) sizes[k] = 0;
  if (N < 0) IBAD("imread_plan: N must be >= 0 (got %d)", N);
  if (!opts) IBAD("imread_plan: NULL options");
  const int mode = (int)opts[IO_RESIZE], filter = (int)opts[IO_FILTER];
  const double amin = opts[IO_AMIN], amax = opts[IO_AMAX], smin = opts[IO_SMIN], smax = opts[IO_SMAX];
  const double C = opts[IO_CONTRAST], S = opts[IO_SATURATION];
  const bool aa = opts[IO_AA] != 0, random_loc = opts[IO_RANDOM] != 0, flip_on = opts[IO_FLIP] != 0;
  const int avg = (int)opts[IO_AVG];
  if (mode < 0 || mode > 2 || opts[IO_RESIZE] != mode) IBAD("imread_plan: Resize mode must be 0 (none), 1 ([Ho Wo]) or 2 (scalar)");
  if (mode == 1 && !(opts[IO_HO] >= 1 && opts[IO_WO] >= 1 && opts[IO_HO] == floor(opts[IO_HO]) && opts[IO_WO] == floor(opts[IO_WO])))
    IBAD("imread_plan: Resize [Ho Wo] must be positive integers (got [%g %g])", opts[IO_HO], opts[IO_WO]);
  if (mode == 2 && !(opts[IO_HO] >= 1 && opts[IO_HO] == floor(opts[IO_HO])))
    IBAD("imread_plan: Resize S must be a positive integer (got %g)", opts[IO_HO]);
  if (filter != XM_IMREAD_BOX && filter != XM_IMREAD_BILINEAR && filter != XM_IMREAD_BICUBIC)
    IBAD("imread_plan: Interpolation must be box, bilinear or bicubic (code %g)", opts[IO_FILTER]);
  if (!(amin <= amax)) IBAD("imread_plan: CropAnisotropy [%g %g]: the minimum is above the maximum", amin, amax);
  if (!(amin == 0 && amax == 0) && !(amin > 0 && std::isfinite(amax)))
    IBAD("imread_plan: CropAnisotropy [%g %g] must be [0 0] or positive", amin, amax);
  if (!(smin > 0 && smin <= 1 && smax > 0 && smax <= 1)) IBAD("imread_plan: CropSize [%g %g] is outside (0, 1]", smin, smax);
  if (!(smin <= smax)) IBAD("imread_plan: CropSize [%g %g]: the minimum is above the maximum", smin, smax);
  if (!(C >= 0 && C <= 1)) IBAD("imread_plan: Contrast %g is outside [0, 1]", C);
  if (!(S >= 0 && S <= 1)) IBAD("imread_plan: Saturation %g is outside [0, 1]", S);
  if (avg < 0 || avg > 2) IBAD("imread_plan: SubtractAverage kind must be 0 (none), 1 (3 values) or 2 (an image)");
  bool bright = false;
  for (int k = 0; k < 9; ++k) {
    if (!std::isfinite(opts[IO_BRIGHT + k])) IBAD("imread_plan: Brightness is not finite");
    bright = bright || opts[IO_BRIGHT + k] != 0;
  }
  if (!draws && (amin != amax || smin != smax || random_loc || flip_on || bright || C > 0 || S > 0))
    IBAD("imread_plan: a random option (CropAnisotropy or CropSize range, CropLocation random, Flip, Brightness, Contrast, "
         "Saturation) needs the draws");
  if (N == 0) return XM_OK;
  if (!hw || !rows) IBAD("imread_plan: NULL argument");
  long long out = 0, tab = 0, part = 0, maxtiles = 0, maxout = 0;
  bool uniform = true;
  for (int i = 0; i < N; ++i) {
    const long long H = hw[3 * i], W = hw[3 * i + 1], pix = hw[3 * i + 2];
    if (H < 1 || W < 1 || pix < 0 || H > kImreadMaxSide || W > kImreadMaxSide)
      IBAD("imread_plan: image %d: size %lld x %lld at offset %lld (sides must be 1 .. %d)", i, H, W, pix, kImreadMaxSide);
    double u[XM_IMREAD_DRAWS] = {0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0, 0, 0};
    if (draws)
      for (int k = 0; k < XM_IMREAD_DRAWS; ++k) {
        u[k] = draws[(long long)i * XM_IMREAD_DRAWS + k];
        if (!std::isfinite(u[k]) || (k < ID_G && !(u[k] >= 0 && u[k] <= 1))) IBAD("imread_plan: image %d: draw %d is %g", i, k, u[k]);
      }
    long long Ho = H, Wo = W;
    if (mode == 1) {
      Ho = (long long)opts[IO_HO];
      Wo = (long long)opts[IO_WO];
    } else if (mode == 2) {
      const double Sz = opts[IO_HO];
      const double lng = (double)(H <= W ? W : H), sht = (double)(H <= W ? H : W);
      double other = floor(Sz * lng / sht + 0.5);
      if (other < 1) other = 1;
      if (other > kImreadMaxSide) other = kImreadMaxSide + 1.0;
      Ho = H <= W ? (long long)Sz : (long long)other;
      Wo = H <= W ? (long long)other : (long long)Sz;
    }
    if (Ho > kImreadMaxSide || Wo > kImreadMaxSide)
      return imread_fail(err, errlen, XM_ETOOBIG, "imread_plan: image %d: output %lld x %lld (sides must be 1 .. %d)", i, Ho, Wo, kImreadMaxSide);
    double ch0 = (double)H, cw0 = (double)W;
    if (!(amin == 0 && amax == 0)) {
      const double a = amin + u[ID_ANISO] * (amax - amin), rho = a * (double)Wo / (double)Ho;
      if (H * rho <= W) {
        cw0 = H * rho;
      } else {
        ch0 = W / rho;
      }
    }
    const double s = smin + u[ID_SIZE] * (smax - smin);
    const double ch = s * ch0, cw = s * cw0;
    const double y0 = (random_loc ? u[ID_Y] : 0.5) * (H - ch), x0 = (random_loc ? u[ID_X] : 0.5) * (W - cw);
    const double ry = ch / Ho, rx = cw / Wo;
    if (!(ch > 0 && cw > 0)) IBAD("imread_plan: image %d: empty crop window", i);
    if (ry > kImreadMaxRatio || rx > kImreadMaxRatio)
      return imread_fail(err, errlen, XM_ENOTSUP, "imread_plan: image %d: a %g x %g window to %lld x %lld reduces by more than %g", i, ch, cw,
                         Ho, Wo, kImreadMaxRatio);
    const double sy = aa && ry > 1 ? ry : 1.0, sx = aa && rx > 1 ? rx : 1.0;
    const int Ty = imread_tap_count(filter, sy), Tx = imread_tap_count(filter, sx);
    const int oc = imread_chunk_rows(ry, Ty, (int)Ho);
    if (oc < 1) return imread_fail(err, errlen, XM_ENOTSUP, "imread_plan: image %d: %d taps do not fit a tile", i, Ty);
    const double gamma = 1 - C + 2 * C * u[ID_CONTRAST], sigma = 1 - S + 2 * S * u[ID_SATURATION];
    double *d = rows + (long long)i * XM_IMREAD_ROW;
    for (int k = 0; k < XM_IMREAD_ROW; ++k) d[k] = 0;
    d[IR_H] = (double)H, d[IR_W] = (double)W, d[IR_PIX] = (double)pix;
    d[IR_HO] = (double)Ho, d[IR_WO] = (double)Wo, d[IR_OUT] = (double)out;
    d[IR_Y0] = y0, d[IR_X0] = x0, d[IR_CH] = ch, d[IR_CW] = cw;
    d[IR_FLIP] = flip_on && u[ID_FLIP] < 0.5 ? 1 : 0;
    d[IR_FILTER] = filter, d[IR_AA] = aa ? 1 : 0, d[IR_TY] = Ty, d[IR_TX] = Tx;
    double b[3];
    for (int c = 0; c < 3; ++c) {
      b[c] = 0;
      for (int k = 0; k < 3; ++k) b[c] += opts[IO_BRIGHT + 3 * c + k] * u[ID_G + k];
      d[IR_B + c] = b[c];
    }
    for (int c = 0; c < 3; ++c) {
      double kc = 0;
      for (int k = 0; k < 3; ++k) {
        const double m = (c == k ? sigma * gamma : 0.0) + (1 - sigma) * gamma / 3;
        d[IR_M + 3 * c + k] = m;
        kc += m * b[k];
      }
      d[IR_K + c] = kc;
    }
    d[IR_GAMMA] = gamma, d[IR_SIGMA] = sigma;
    d[IR_TAB] = (double)tab, d[IR_OC] = oc, d[IR_RY] = ry, d[IR_RX] = rx, d[IR_SY] = sy, d[IR_SX] = sx;
    const long long tiles = (Wo + kImreadTW - 1) / kImreadTW;
    d[IR_TILES] = (double)tiles, d[IR_PART] = (double)part;
    d[IR_AVG] = avg, d[IR_CONTRAST] = C > 0 ? 1 : 0;
    if (i > 0 && (Ho != (long long)rows[IR_HO] || Wo != (long long)rows[IR_WO])) uniform = false;
    out += Ho * Wo * 3;
    tab += Ho * Ty + Wo * Tx + Ho + Wo;
    part += 3 * tiles;
    if (tiles > maxtiles) maxtiles = tiles;
    if (Ho > maxout) maxout = Ho;
    if (Wo > maxout) maxout = Wo;
    if (out >= (1LL << 40) || tab >= (1LL << 40))
      return imread_fail(err, errlen, XM_ETOOBIG, "imread_plan: image %d: the batch is too large", i);
  }
  if (avg == 2 && !uniform) IBAD("imread_plan: SubtractAverage with an image needs outputs of one size");
  sizes[IS_OUT] = out, sizes[IS_TABLE] = tab, sizes[IS_PART] = part, sizes[IS_MAXTILES] = maxtiles;
  sizes[IS_CONTRAST] = C > 0 ? 1 : 0, sizes[IS_UNIFORM] = uniform ? 1 : 0, sizes[IS_MAXOUT] = maxout, sizes[IS_N] = N;
  return XM_OK;
#undef IBAD
}

}  // namespace xm

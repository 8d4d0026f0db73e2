// Host-side planning of vl_nnconv: integer arithmetic on the geometry, nothing from HIP (compiles with g++ -std=c++17;
// tests/conv_plan_check.cpp checks it against the definition of the convolution without a GPU).
//   * the stride-parity classes and tap tables of dgrad, the tap tables of forward / wgrad;
//   * the CAN half of every kernel's eligibility: "can this kernel run this geometry" -- limits of the instantiated
//     kernels, alignment of the operands (addresses come in as uintptr_t), 32-bit byte offsets.
// The WANT half -- path switches, force hooks, size thresholds, the tuning table -- is conv.hip's (*_ok = policy && *_can).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace xm {

// limits of the kernels the predicates below read (conv_kernels.h / stem_pool_kernels.h size their LDS from them)
constexpr int kBK = 16;          // reduction depth per LDS stage of the implicit GEMM
constexpr int kHaloCB = 8;       // channels per reduction stage of the halo-patch kernels
constexpr int kStemHP = 520;     // conv_stem_kernel: source columns of <= 512 rows (+ 4 rows of padding either side)
constexpr int kStemNV = 7;       // ... filter columns; 8 filter rows (the 8th has zero weights) per column
constexpr int kStem3CS = 232;    // conv_stem3_kernel: patch rows of a source column
constexpr int kSpNC = 9;         // stem_pool_kernels.h: source columns under two output columns (stride 2: 7 + 2)
constexpr int kDgS2Rows = 96;    // conv_dgrad_s2_kernel: input channels per block

// ---- geometry shared by the three directions ------------------------------------------------
struct Geo {
  int H, W, C, N, FH, FW, FC, K, G, Kg, Ho, Wo, R;
  int sy, sx, pt, pb, pl, pr, dy, dx;
};

// kernels that form BYTE offsets into a tensor in 32-bit arithmetic take tensors below 2 GiB
inline bool fits_i32_bytes(size_t elements) { return elements * 4 < (1ull << 31); }
inline size_t x_elements(const Geo &g) { return (size_t)g.H * g.W * g.C * g.N; }
inline size_t y_elements(const Geo &g) { return (size_t)g.Ho * g.Wo * g.K * g.N; }

// ---- tap tables -----------------------------------------------------------------------------------------------------
struct Tap2 {   // layout of HIP's int2: {byte offset in the gather source, (u, v) index of the validity mask}
  int off, uv;
};
struct Tap4 {   // layout of HIP's int4: {byte offset in X, u * dy, v * dx, 0}
  int off, du, dv, zero;
};

// reduction index r = u + FH*(v + FW*c) of forward / wgrad -> byte offset of the tap in X
inline int x_tap(const Geo &g, int r, int *u, int *v) {
  *u = r % g.FH, *v = (r / g.FH) % g.FW;
  return 4 * (*u * g.dy + g.H * (*v * g.dx) + g.H * g.W * (r / (g.FH * g.FW)));
}
// forward tap table for the implicit GEMM: {byte offset in X, (u,v) index}; the kernels fetch it three stages ahead
inline std::vector<Tap2> fwd_tap_table(const Geo &g, int Rp, bool all_valid) {
  std::vector<Tap2> t(Rp + 3 * kBK, Tap2{0, 63});
  for (int r = 0, u, v; r < g.R; ++r) {
    const int off = x_tap(g, r, &u, &v);
    t[r] = Tap2{off, all_valid ? 0 : u + g.FH * v};   // all_valid (no spatial padding, > 63 taps): all share mask bit 0 = tap (0,0)
  }
  return t;
}
// wgrad tap table (count >= R entries): {byte offset in X, u*dy, v*dx}
inline std::vector<Tap4> wgrad_tap_table(const Geo &g, int count) {
  std::vector<Tap4> t(count, Tap4{0, -(1 << 28), 0, 0});
  for (int r = 0, u, v; r < g.R; ++r) {
    const int off = x_tap(g, r, &u, &v);
    t[r] = Tap4{off, u * g.dy, v * g.dx, 0};
  }
  return t;
}

// ---- forward on an output lattice (xm_nnconv_forward_lattice) -------------------------------------------------------
// The lattice holds the output pixels (ly i, lx j): PI x PJ of them per sample, enumerated like the full-extent pixels
// (i fastest, then j, then the sample), so the map from a full-extent pixel index to its lattice index is monotone.
inline int lattice_extent(int full, int step) { return (full - 1) / step + 1; }
// the number of lattice pixels whose FULL-EXTENT index i + Ho (j + Wo n) lies below p0: what a cut of the full-extent
// pixel range at p0 (the start of a hybrid launch's split remainder) becomes in lattice indices
inline long long lattice_pixels_below(long long p0, int Ho, int Wo, int ly, int lx) {
  const int PI = lattice_extent(Ho, ly), PJ = lattice_extent(Wo, lx);
  const long long n = p0 / ((long long)Ho * Wo);
  const int q = (int)(p0 - n * Ho * Wo), j = q / Ho, i = q % Ho;
  // whole samples, whole lattice columns left of column j, and the lattice rows above row i when j is a lattice column
  return n * PI * PJ + (long long)((j + lx - 1) / lx) * PI + (j % lx == 0 ? (i + ly - 1) / ly : 0);
}

// ---- dgrad: one implicit GEMM per stride-parity class (a, b) of the input pixels ------------------------------------
// Class (a, b) holds the input pixels (hi, wi) with (hi + pt) % sy == a, (wi + pl) % sx == b: hi = hi0 + sy i (i < PI),
// wi = wi0 + sx j (j < PJ).  Only the taps with (u dy) % sy == a, (v dx) % sx == b reach them: u = u0 + ustep iu
// (iu < nU), v = v0 + vstep iv (iv < nV).  Rc = reduction length (taps x filters of a group), Rp = Rc padded to kBK.
struct DgradClass {
  int a, b, u0, ustep, nU, v0, vstep, nV, Rc, Rp, i0, hi0, PI, j0, wi0, PJ;
};

// H-collapsing convolution (FC layer sliding along W only, e.g. the student's fc6: 9x1 filter on a
// 9 x Wi map): every input row hi is touched by exactly one filter row u = hi, so folding u into
// the GEMM rows (M = FH*FC) avoids multiplying FH-1 masked-out taps per pixel.
inline bool dgrad_fold_h(const Geo &g) {
  return g.Ho == 1 && g.FH > 1 && g.FH == g.H && g.pt == 0 && g.pb == 0 && g.dy == 1 && g.sy == 1;
}

// the taps t < F with (t * d) % s == a form an arithmetic progression t0, t0 + step, ... (n of them; t0 = -1: none)
inline void class_taps(int F, int d, int s, int a, int *t0, int *step, int *n) {
  *t0 = -1, *step = 1, *n = 0;
  for (int t = 0; t < F; ++t)
    if ((t * d) % s == a) {
      if (*t0 < 0) *t0 = t;
      else if (*n == 1) *step = t - *t0;
      ++*n;
    }
}

// the classes that hold pixels AND taps; *covers_all = false when some class with pixels has no tap (1 x 1 / stride 2:
// its pixels receive no gradient and no GEMM writes them)
inline std::vector<DgradClass> dgrad_classes(const Geo &g, bool foldH, bool *covers_all) {
  std::vector<DgradClass> cls;
  *covers_all = true;
  for (int b = 0; b < g.sx; ++b)
    for (int a = 0; a < g.sy; ++a) {
      DgradClass c{};
      c.a = a, c.b = b;
      class_taps(g.FH, g.dy, g.sy, a, &c.u0, &c.ustep, &c.nU);
      class_taps(g.FW, g.dx, g.sx, b, &c.v0, &c.vstep, &c.nV);
      c.i0 = g.pt > a ? (g.pt - a + g.sy - 1) / g.sy : 0;
      c.hi0 = g.sy * c.i0 + a - g.pt;
      c.PI = c.hi0 < g.H ? (g.H - c.hi0 + g.sy - 1) / g.sy : 0;
      c.j0 = g.pl > b ? (g.pl - b + g.sx - 1) / g.sx : 0;
      c.wi0 = g.sx * c.j0 + b - g.pl;
      c.PJ = c.wi0 < g.W ? (g.W - c.wi0 + g.sx - 1) / g.sx : 0;
      if (c.PI <= 0 || c.PJ <= 0) continue;
      if (c.nU == 0 || c.nV == 0) {
        *covers_all = false;
        continue;
      }
      c.Rc = (foldH ? c.nV : c.nU * c.nV) * g.Kg;
      c.Rp = (c.Rc + kBK - 1) / kBK * kBK;
      cls.push_back(c);
    }
  return cls;
}

// The class's gather in dY space, in the fields of ConvGemmArgs: pixel (i, j) of the class has its origin at dY row
// i + gh0, column j + gw0; tap (iu, iv) sits (du0 + iu dus, dv0 + iv dvs) from it.  With u' = (u dy - a) / sy:
// ho = i' - u'.  foldH: the single dY row, the filter row is the GEMM row's (m % FH).
struct DgradGather {
  int gh0, gw0, nU, du0, dus, dv0, dvs;
};
inline DgradGather dgrad_gather(const Geo &g, const DgradClass &c, bool foldH) {
  const int up0 = ((c.u0 * g.dy) - c.a) / g.sy, ups = c.ustep * g.dy / g.sy;
  const int vp0 = ((c.v0 * g.dx) - c.b) / g.sx, vps = c.vstep * g.dx / g.sx;
  return DgradGather{foldH ? 0 : c.i0, c.j0, foldH ? 1 : c.nU, foldH ? 0 : -up0, -ups, -vp0, -vps};
}

// tap table in dY space: r' = iu + nU*(iv + nV*k) -> {byte offset from the origin, (iu, iv) index}
inline std::vector<Tap2> dgrad_tap_table(const Geo &g, const DgradClass &c, bool foldH) {
  const DgradGather q = dgrad_gather(g, c, foldH);
  std::vector<Tap2> t(c.Rp + 3 * kBK, Tap2{0, 63});
  for (int r = 0; r < c.Rc; ++r) {
    const int iu = foldH ? 0 : r % c.nU, iv = foldH ? r % c.nV : (r / c.nU) % c.nV, k = r / (foldH ? c.nV : c.nU * c.nV);
    t[r] = Tap2{4 * (q.du0 + iu * q.dus + g.Ho * (q.dv0 + iv * q.dvs) + g.Ho * g.Wo * k), iu + q.nU * iv};
  }
  return t;
}

// ---- what each special-purpose kernel can run ------------------------------------------------------------------------
// epilogue of a forward launch, as far as the stem kernels care
enum : unsigned { kEpiVecStore = 1, kEpiScale = 2, kEpiResid = 4, kEpiGate = 8, kEpiRelu = 16, kEpiStats = 32 };

// the geometry common to the single-channel stem kernels (conv_stem_kernel, conv_stem_wgrad_kernel, stem_pool_kernels.h):
// ONE input channel, <= 8 x 7 and >= 16 taps, stride 1 / 2 along H, <= 96 filters, source columns of <= 512 rows
inline bool stem_shape_can(const Geo &g, uintptr_t x, int max_taps) {
  if (g.C != 1 || g.G != 1 || g.FC != 1 || g.dy != 1 || g.dx != 1) return false;
  if (g.FH > 8 || g.FW > kStemNV || g.FH * g.FW < 16 || g.FH * g.FW > max_taps || g.Kg > 96) return false;
  if (g.sy != 1 && g.sy != 2) return false;
  if (g.H % 4 != 0 || g.H > kStemHP - 8 || (x & 15) != 0) return false;
  return g.pt <= 4 && 4 * ((g.sy * (g.Ho - 1) - g.pt + 4 + 7) >> 2) + 3 < kStemHP;   // last 16-byte row unit a tile loads
}
inline bool stem_fwd_can(const Geo &g, uintptr_t x, unsigned epi) {
  if (!stem_shape_can(g, x, 8 * kStemNV)) return false;   // conv_stem_kernel: every tap arrangement of the shape
  if ((epi & ~kEpiStats) != kEpiVecStore) return false;   // ... carries the plain 16-byte-store epilogue (+ statistics) only
  return g.Ho >= 128;                                     // ... a 128-pixel tile spans <= 2 output columns
}
inline bool stem_wgrad_can(const Geo &g, uintptr_t x, uintptr_t dzdy) {
  if (!stem_shape_can(g, x, 64)) return false;            // conv_stem_wgrad_kernel: 64 partial columns per filter
  if ((dzdy & 15) != 0 || (g.Ho * g.Wo) % 4 != 0) return false;   // ... dY pixel quads stay inside a sample
  return g.Ho >= 128;                                     // ... tiles as the forward kernel's
}
inline bool stem_pool_can(const Geo &g, uintptr_t x) {
  if (!stem_shape_can(g, x, 63)) return false;            // Gram matrix: 63 taps + the column of ones in 64 x 64
  if (g.sx + g.FW > kSpNC) return false;                  // ... two output columns sit on <= 9 source columns
  return g.Ho >= 32;                                      // ... a wave's chunk of an output column
}

// conv_stem3_kernel: 7 x 7 / stride 2 over RGB images, 64 filters (the teachers' conv1)
inline bool stem3_can(const Geo &g, uintptr_t x, unsigned epi) {
  if (g.C != 3 || g.G != 1 || g.FC != 3 || g.FH != 7 || g.FW != 7 || g.sy != 2 || g.sx != 2 || g.dy != 1 || g.dx != 1) return false;
  if (g.Kg != 64 || !(epi & kEpiVecStore) || (epi & (kEpiResid | kEpiGate | kEpiStats))) return false;
  if ((g.Ho * g.Wo) % 128 != 0 || g.Ho < 64 || (g.H & 1) || g.pt > 4 || g.pl > 6) return false;
  if (2 * (g.Ho - 1) + 8 + (4 - g.pt) + 1 > kStem3CS) return false;                 // patch rows of a column
  return (x & 7) == 0 && fits_i32_bytes(x_elements(g));
}

// conv_wgrad_patch_kernel<30>: 3 x 3 / stride 1 / pad 1 layers over 30-row maps
inline bool wgrad_patch_can(const Geo &g, uintptr_t x, uintptr_t dzdy) {
  if (g.G != 1 || g.FH != 3 || g.FW != 3 || g.sy != 1 || g.sx != 1 || g.dy != 1 || g.dx != 1) return false;
  if (g.pt != 1 || g.pb != 1 || g.pl != 1 || g.pr != 1) return false;
  if (g.H != 30 || g.Ho != g.H || g.Wo != g.W) return false;          // instantiated row counts (HH)
  if (((x | dzdy) & 7) != 0) return false;
  return fits_i32_bytes(x_elements(g)) && fits_i32_bytes(y_elements(g));
}

// conv_wgrad_patch_s2_kernel<5, 2>: 5 x 5 / stride 2 layers (the student's conv2)
inline bool wgrad_patch_s2_can(const Geo &g, uintptr_t x, uintptr_t dzdy) {
  if (g.G != 1 || g.FH != 5 || g.FW != 5 || g.sy != 2 || g.sx != 2 || g.dy != 1 || g.dx != 1) return false;
  if (g.pt < 1 || g.pt > 2 || g.pl < 0 || g.pl > 4) return false;
  if ((g.H & 1) || (g.Ho & 1)) return false;                            // 8-byte loads of row pairs
  if (((x | dzdy) & 7) != 0) return false;
  return fits_i32_bytes(x_elements(g)) && fits_i32_bytes(y_elements(g));   // (904 MB / 585 MB at 256 spectrograms)
}

// conv_dgrad_s2_kernel: 5 x 5 / stride 2 layers, both row parities per wave; no accumulating epilogue
inline bool dgrad_s2_can(const Geo &g, uintptr_t dzdy, uintptr_t dxo, bool accum) {
  if (accum || g.G != 1 || g.FH != 5 || g.FW != 5 || g.sy != 2 || g.sx != 2 || g.dy != 1 || g.dx != 1) return false;
  if (g.pt != 1 || g.pl < 0 || g.pl > 4 || (g.H & 1) || (g.Ho & 1) || (g.K & 7)) return false;
  if (((dzdy | dxo) & 7) != 0) return false;
  return fits_i32_bytes(y_elements(g));
}

// ---- conv1 -> bnorm -> relu -> pool in one kernel, forward and backward (stem_pool_kernels.h) -------------------------
// the pooling all three fused stem entry points are written for
inline bool pool3x3s2_unpadded(int ph, int pw, int psy, int psx, int ppt, int ppb, int ppl, int ppr) {
  return ph == 3 && pw == 3 && psy == 2 && psx == 2 && ppt == 0 && ppb == 0 && ppl == 0 && ppr == 0;
}

enum FusedStemDir { kFusedStemForward, kFusedStemBackward };
// xm_nnconv_bnorm_relu_pool_forward / xm_nnconv_backward_filter_bnrelupool_gram side by side.  `pooled_ptrs`: the
// addresses of the pooled tensors the call touches, or-ed (4-byte accesses).  The two directions do NOT accept the same
// shapes: the forward takes any pooled height, the backward needs four pooled rows.
inline bool fused_stem_can(FusedStemDir dir, const Geo &g, uintptr_t x, int ph, int pw, int psy, int psx, int ppt, int ppb,
                           int ppl, int ppr, int pHo, int pWo, uintptr_t pooled_ptrs) {
  if (!stem_pool_can(g, x) || g.K != g.Kg || !pool3x3s2_unpadded(ph, pw, psy, psx, ppt, ppb, ppl, ppr)) return false;
  if (pWo < 1 || (long long)pHo * pWo * g.K * g.N >= (1LL << 30) || (pooled_ptrs & 3) != 0) return false;
  if (dir == kFusedStemBackward) return pHo >= 4;        // conv_stem_wgrad_pool_kernel, either stride
  // conv_stem_bnpool_fwd_kernel: stride 2 both ways, <= 7 x exactly 7 taps, filters in groups of 8
  return g.sy == 2 && g.sx == 2 && g.FH <= 7 && g.FW == kStemNV && g.K % 8 == 0 && pHo >= 1;
}

}  // namespace xm

// conv1 -> bnorm -> relu -> pool of a single-channel first layer through the Gram matrix of the input patches
// (stem_pool_kernels.h): host side + C ABI.  Nothing of conv.hip's implicit-GEMM machinery -- no tile configuration,
// no tuning table, no tap tables -- only the checked geometry (make_geo) and the stem force switch (xm_common.h).
#include <algorithm>

#include "prof.h"
#include "stem_pool_kernels.h"

namespace xm {

static bool stem_pool_ok(const Geo &g, const float *x) { return path_on(kPathStem) && stem_pool_can(g, (uintptr_t)x); }

static void stem_pool_args(StemPoolArgs &a, const float *x, const Geo &g) {
  a.X = x, a.M = g.Kg, a.R = g.R, a.nU = g.FH, a.nV = g.FW, a.PI = g.Ho, a.PJ = g.Wo;
  const int G = sp_row_groups(g.Ho);
  a.divJG = make_fastdiv((uint32_t)(sp_col_pairs(g.Wo) * G)), a.divG = make_fastdiv((uint32_t)G);
  a.gsx = g.sx, a.gh0 = -g.pt, a.gw0 = -g.pl, a.LimH = g.H, a.LimW = g.W, a.xSampleStride = g.H * g.W;
}

// (units, grids and unit -> work maps of all three kernels: stem_pool_plan.h)
static size_t stem_gram_need(const Geo &g) { return WsCarver::need(stem_gram_part_floats(g.N, g.Ho, g.Wo), 4); }

// G (fp64 [64][64]) of the patches of x; scratch from the caller's carver
static int launch_stem_gram(WsCarver &ws, const float *x, const Geo &g, double *gram, hipStream_t st) {
  StemPoolArgs a{};
  stem_pool_args(a, x, g);
  const int nunits = stem_pool_units(g.N, g.Ho, g.Wo), grid = stem_pool_grid(nunits, kSpGramOcc);
  a.part = ws.take<float>(stem_gram_part_floats(g.N, g.Ho, g.Wo));
  static bool attr_done = false;
  if (!attr_done) {
    XM_HIP(hipFuncSetAttribute((const void *)stem_gram_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, kSpGramSmem));
    XM_HIP(hipFuncSetAttribute((const void *)stem_gram_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, kSpGramSmem));
    attr_done = true;
  }
  {
    // three of the four 32 x 32 tiles of the padded 64 x 64 product are computed
    ProfScope ps(prof_key(kProfStemGram), 2.0 * (g.R + 1) * (g.R + 1) * (double)g.Ho * g.Wo * g.N, st, 4.0 * g.H * g.W * g.N);
    if (g.sy == 2) hipLaunchKernelGGL(stem_gram_kernel<2>, dim3(grid), dim3(256), kSpGramSmem, st, a, nunits);
    else hipLaunchKernelGGL(stem_gram_kernel<1>, dim3(grid), dim3(256), kSpGramSmem, st, a, nunits);
  }
  XM_LAUNCH_CHECK();
  hipLaunchKernelGGL(stem_gram_reduce_kernel, dim3(64), dim3(1024), 0, st, a.part, gram, grid);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

}  // namespace xm

using namespace xm;

extern "C" {

// G = P~' P~ of the im2col patches (+ a column of ones) of a single-channel first-layer convolution: fp64 [64][64],
// row / column t = u + FH v (t < FH FW), t = FH FW: the ones column; entries beyond are zero.
int xm_stem_gram(const float *x, int H, int W, int N, int FH, int FW, int sy, int sx, int pt, int pb, int pl, int pr,
                 double *gram, void *stream) {
  Geo g;
  int rc = make_geo(g, H, W, 1, N, FH, FW, 1, 1, sy, sx, pt, pb, pl, pr, 1, 1);
  if (rc) return rc;
  if (!x || !gram) return fail(XM_EINVAL, "xm_stem_gram: NULL tensor");
  if (!stem_pool_ok(g, x)) return fail(XM_ENOTSUP, "xm_stem_gram: geometry not covered");
  hipStream_t st = (hipStream_t)stream;
  WsCarver ws;
  rc = ws.init(stem_gram_need(g), st);
  if (rc) return rc;
  return launch_stem_gram(ws, x, g, gram, st);
}

// Batch moments [mean, sqrt(var + eps)] of Y = vl_nnconv(X, F, B) for a single-channel first layer, from G alone
int xm_stem_gram_moments(const double *gram, const float *f, const float *b, int FH, int FW, int K, float epsilon,
                         float *moments_out, void *stream) {
  if (!gram || !f || !moments_out) return fail(XM_EINVAL, "xm_stem_gram_moments: NULL tensor");
  if (FH * FW < 1 || FH * FW > 63 || K < 1) return fail(XM_EINVAL, "xm_stem_gram_moments: bad shape");
  hipLaunchKernelGGL(stem_gram_moments_kernel, dim3(K), dim3(64), 0, (hipStream_t)stream, gram, f, b, K, FH * FW,
                     (double)epsilon, moments_out);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

// Y_POOL, ARGMAX, MOMENTS of vl_nnpool(vl_nnrelu(vl_nnbnorm(vl_nnconv(X, F, B), G, BB)), [3 3], 'stride', 2) for a
// single-channel first layer in one kernel (conv_stem_bnpool_fwd_kernel): the convolution's output is never written.
// Train mode (moments_in NULL): G = xm_stem_gram(X) is left in `gram` (fp64 [64][64], caller-owned: the backward call
// takes it) and the batch moments come from it.  The table marks windows whose maximum did not pass the ReLU with 255.
int xm_nnconv_bnorm_relu_pool_forward(const float *x, int H, int W, int C, int N, const float *f, int FH, int FW, int FC,
                                      int K, const float *bias, int sy, int sx, int pt, int pb, int pl, int pr, int dy, int dx,
                                      const float *bn_g, const float *bn_b, float epsilon, const float *moments_in, int ph,
                                      int pw, int psy, int psx, int ppt, int ppb, int ppl, int ppr, double *gram,
                                      float *y_pool, unsigned char *argmax, float *moments_out, void *stream) {
  Geo g;
  int rc = make_geo(g, H, W, C, N, FH, FW, FC, K, sy, sx, pt, pb, pl, pr, dy, dx);
  if (rc) return rc;
  if (!x || !f || !bn_g || !bn_b || !y_pool || !argmax || (!moments_in && (!gram || !moments_out)))
    return fail(XM_EINVAL, "vl_nnconv + bnorm + relu + pool (fused forward): NULL tensor");
  hipStream_t st = (hipStream_t)stream;
  const int pHo = out_size(g.Ho, ppt, ppb, ph, 1, psy), pWo = out_size(g.Wo, ppl, ppr, pw, 1, psx);
  const long long pooled = (long long)pHo * pWo * g.K * g.N;
  const bool ok = path_on(kPathStem) && g_force_stem != 0 &&
                  fused_stem_can(kFusedStemForward, g, (uintptr_t)x, ph, pw, psy, psx, ppt, ppb, ppl, ppr, pHo, pWo, (uintptr_t)y_pool);
  if (!ok)
    return fail(XM_ENOTSUP, "vl_nnconv + bnorm + relu + pool (fused forward): geometry not covered by the fused kernel");
  const float *moments = moments_in;
  if (!moments_in) {
    WsCarver ws;
    rc = ws.init(stem_gram_need(g), st);
    if (rc) return rc;
    rc = launch_stem_gram(ws, x, g, gram, st);
    if (rc) return rc;
    hipLaunchKernelGGL(stem_gram_moments_kernel, dim3(g.K), dim3(64), 0, st, gram, f, bias, g.K, g.R, (double)epsilon,
                       moments_out);
    XM_LAUNCH_CHECK();
    moments = moments_out;
  }
  StemFwdArgs a{};
  a.X = x, a.F = f, a.bias = bias, a.bn_g = bn_g, a.bn_b = bn_b, a.moments = moments;
  a.Y = y_pool, a.amax = argmax;
  a.M = g.K, a.R = g.R, a.nU = g.FH, a.nV = g.FW;
  a.PI = g.Ho, a.PJ = g.Wo, a.pHo = pHo, a.pWo = pWo;
  const SfPlan fp = stem_fwd_plan(g.N, pHo, pWo, XM_SF_OCC);      // strips, segments of window columns, wave units
  a.NS = fp.NS, a.SG = fp.SG, a.nunits = fp.nunits;
  a.div3 = make_fastdiv(3u), a.divSG = make_fastdiv((uint32_t)a.SG), a.divNS = make_fastdiv((uint32_t)a.NS);
  a.gh0 = -g.pt, a.gw0 = -g.pl, a.LimH = g.H, a.LimW = g.W, a.xSampleStride = g.H * g.W;
  a.yBytes = (unsigned)(pooled * 4), a.amBytes = (unsigned)pooled;
  static bool attr_done = false;
  if (!attr_done) {
    XM_HIP(hipFuncSetAttribute((const void *)conv_stem_bnpool_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kSfSmem));
    attr_done = true;
  }
  const int grid = fp.grid;
  {
    ProfScope ps(prof_key(kProfStemBnpoolFwd), 2.0 * g.K * (double)g.Ho * g.Wo * g.N * g.R, st, 4.0 * g.H * g.W * g.N + 5.0 * (double)pooled);
    hipLaunchKernelGGL(conv_stem_bnpool_fwd_kernel, dim3(grid), dim3(256), kSfSmem, st, a);
  }
  XM_LAUNCH_CHECK();
  return XM_OK;
}

// xm_nnconv_backward_filter_bnrelupool (conv.hip) without a pass over the convolution's output: the filter bank F (and
// bias B) take Y's place; `gram` = xm_stem_gram of X (NULL: computed here).
int xm_nnconv_backward_filter_bnrelupool_gram(const float *x, int H, int W, int C, int N, const float *f, int FH, int FW,
                                              int FC, int K, const float *bias, int sy, int sx, int pt, int pb, int pl,
                                              int pr, int dy, int dx, const float *bn_g, const float *moments, int train,
                                              int ph, int pw, int psy, int psx, int ppt, int ppb, int ppl, int ppr,
                                              const unsigned char *argmax, const float *y_pool, const float *dzdy_pool,
                                              const double *gram, float *df_out, float *dbias_out, float *dg_out,
                                              float *db_out, void *stream) {
  Geo g;
  int rc = make_geo(g, H, W, C, N, FH, FW, FC, K, sy, sx, pt, pb, pl, pr, dy, dx);
  if (rc) return rc;
  if (!x || !f || !bn_g || !moments || !argmax || !dzdy_pool || !df_out)
    return fail(XM_EINVAL, "vl_nnconv(filter derivative through bnorm+relu+pool, gram): NULL tensor");
  hipStream_t st = (hipStream_t)stream;
  const int pHo = out_size(g.Ho, ppt, ppb, ph, 1, psy), pWo = out_size(g.Wo, ppl, ppr, pw, 1, psx);
  const long long pooled = (long long)pHo * pWo * g.K * g.N;
  const bool ok = path_on(kPathStem) && g_force_stem != 0 &&      // (y_pool NULL: the table marks closed windows itself)
                  fused_stem_can(kFusedStemBackward, g, (uintptr_t)x, ph, pw, psy, psx, ppt, ppb, ppl, ppr, pHo, pWo,
                                 (uintptr_t)dzdy_pool | (uintptr_t)y_pool);
  if (!ok)
    return fail(XM_ENOTSUP, "vl_nnconv(filter derivative through bnorm+relu+pool, gram): geometry not covered by the fused kernel");
  StemPoolArgs a{};
  stem_pool_args(a, x, g);
  // wave units (sample, column pair, 64-row chunk pair) x 3 row tiles of filters
  const SpBwdPlan bp = stem_bwd_plan(g.N, g.Ho, g.Wo);
  const int nunits = bp.nunits, grid = bp.grid, nwc = bp.nwc;
  a.divJG = make_fastdiv((uint32_t)bp.npair);
  a.divG = make_fastdiv((uint32_t)bp.ncp);
  WsCarver ws;
  rc = ws.init(WsCarver::need((size_t)grid * 4 * 32 * 64, 4) + WsCarver::need(64 * 64, 8) + stem_gram_need(g), st);
  if (rc) return rc;
  a.part = ws.take<float>((size_t)grid * 4 * 32 * 64);
  double *gr = ws.take<double>(64 * 64);
  if (train && !gram) {
    rc = launch_stem_gram(ws, x, g, gr, st);
    if (rc) return rc;
    gram = gr;
  }
  a.dP = dzdy_pool;
  a.yP = y_pool ? y_pool : dzdy_pool;
  a.amax = argmax;
  a.pHo = pHo;
  a.pWo = pWo;
  a.dpBytes = (unsigned)(pooled * 4);
  a.amBytes = (unsigned)pooled;
  static bool attr_done = false;
  if (!attr_done) {
    XM_HIP(hipFuncSetAttribute((const void *)conv_stem_wgrad_pool_kernel<2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, kSp3Smem));
    XM_HIP(hipFuncSetAttribute((const void *)conv_stem_wgrad_pool_kernel<1, true>, hipFuncAttributeMaxDynamicSharedMemorySize, kSp3Smem));
    XM_HIP(hipFuncSetAttribute((const void *)conv_stem_wgrad_pool_kernel<2, false>, hipFuncAttributeMaxDynamicSharedMemorySize, kSp3Smem));
    XM_HIP(hipFuncSetAttribute((const void *)conv_stem_wgrad_pool_kernel<1, false>, hipFuncAttributeMaxDynamicSharedMemorySize, kSp3Smem));
    attr_done = true;
  }
  {
    const double abytes = 4.0 * g.H * g.W * g.N + (y_pool ? 9.0 : 5.0) * (double)pooled + 4.0 * a.M * a.R;
    ProfScope ps(prof_key(kProfStemWgradPool, y_pool ? 1 : 0), 2.0 * a.M * (double)g.Ho * g.Wo * g.N * a.R, st, abytes);
#define XM_SPW_LAUNCH(SY_, G_) hipLaunchKernelGGL((conv_stem_wgrad_pool_kernel<SY_, G_>), dim3(grid), dim3(256), kSp3Smem, st, a, nunits)
    if (g.sy == 2) {
      if (y_pool) XM_SPW_LAUNCH(2, true); else XM_SPW_LAUNCH(2, false);
    } else {
      if (y_pool) XM_SPW_LAUNCH(1, true); else XM_SPW_LAUNCH(1, false);
    }
#undef XM_SPW_LAUNCH
  }
  XM_LAUNCH_CHECK();
  hipLaunchKernelGGL(stem_pool_finalize_kernel, dim3(g.K), dim3(1024), 0, st, a.part, nwc, gram, f, bias, bn_g, moments, g.K,
                     g.R, train ? 1 : 0, df_out, dbias_out, dg_out, db_out);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

}  // extern "C"

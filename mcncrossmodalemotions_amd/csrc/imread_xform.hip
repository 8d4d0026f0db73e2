// vl.vl_imreadjpeg's crop / flip / filter / colour stage (ABI 125): from the ragged buffer of decoded pixels that every
// JPEG decoder of this library writes (H x W x 3 per image, MATLAB layout) to the resampled, colour-jittered outputs.
// The plan (imread_plan.h, host only) gives one row of doubles per image; three kernels run it:
//   imread_table_kernel     per (image, axis, output sample): first tap and T weights, in double, rounded once to float
//   imread_resample_kernel  per (image, tile of kImreadTW output columns): the horizontal pass reads the source with the
//                           lanes of a wave along a source column (contiguous) and leaves source rows x columns x 3 in
//                           LDS; the vertical pass runs from LDS with the lanes along an output column; windows of more
//                           source rows than the tile holds are walked in chunks of output rows (imread_chunk_rows).
//                           Without Contrast its epilogue applies the colour terms; with Contrast it stores p - a and
//                           one partial sum per block and channel
//   imread_colour_kernel    Contrast only: sums an image's partials in tile order and applies the colour terms to `out`
// Nothing is accumulated with atomics and a block's work depends on its own image's row alone, so an image gives the same
// bits alone and in any batch.  Source indices are clamped before the load (replicated border).
#include "imread_plan.h"
#include "prof.h"
#include "xm_common.h"

namespace xm {

struct ImreadColour {
  float m[9], k[3];
};

__device__ __forceinline__ void imread_colour_load(const double *__restrict__ d, ImreadColour &c) {
  for (int i = 0; i < 9; ++i) c.m[i] = (float)d[IR_M + i];
  for (int i = 0; i < 3; ++i) c.k[i] = (float)d[IR_K + i];
}

// M p + add, one order of operations for both kernels that apply the colour terms
__device__ __forceinline__ float imread_colour_apply(const float *m, float p0, float p1, float p2, float add) {
  return fmaf(m[2], p2, fmaf(m[1], p1, fmaf(m[0], p0, add)));
}

__global__ __launch_bounds__(256) void imread_table_kernel(const double *__restrict__ desc, float *__restrict__ table) {
  const int n = blockIdx.y >> 1, axis = blockIdx.y & 1;
  const int o = blockIdx.x * 256 + threadIdx.x;
  const double *d = desc + (size_t)n * XM_IMREAD_ROW;
  const int Ho = (int)d[IR_HO], Wo = (int)d[IR_WO], Ty = (int)d[IR_TY], Tx = (int)d[IR_TX], filter = (int)d[IR_FILTER];
  float *wy = table + (long long)d[IR_TAB];
  float *wx = wy + (size_t)Ho * Ty;
  int *fy = (int *)(wx + (size_t)Wo * Tx);
  int *fx = fy + Ho;
  if (axis == 0) {
    if (o < Ho) fy[o] = imread_taps(filter, d[IR_Y0], d[IR_RY], d[IR_SY], Ty, o, wy + o, Ho);
  } else if (o < Wo) {
    const int op = d[IR_FLIP] != 0 ? Wo - 1 - o : o;
    fx[o] = imread_taps(filter, d[IR_X0], d[IR_RX], d[IR_SX], Tx, op, wx + (size_t)o * Tx, 1);
  }
}

template <bool CONTRAST>
__global__ __launch_bounds__(256) void imread_resample_kernel(const float *__restrict__ pixels, const double *__restrict__ desc,
                                                               const float *__restrict__ table, const float *__restrict__ avg,
                                                               float *__restrict__ out, float *__restrict__ partial) {
  __shared__ float lds[kImreadTileRows * kImreadTW * 3];
  const double *d = desc + (size_t)blockIdx.y * XM_IMREAD_ROW;
  const int tile = blockIdx.x;
  if (tile >= (int)d[IR_TILES]) return;
  const int tid = threadIdx.x;
  const int H = (int)d[IR_H], W = (int)d[IR_W], Ho = (int)d[IR_HO], Wo = (int)d[IR_WO], Ty = (int)d[IR_TY], Tx = (int)d[IR_TX];
  const int oc = (int)d[IR_OC], avg_kind = (int)d[IR_AVG];
  const float *pix = pixels + (long long)d[IR_PIX];
  float *o_img = out + (long long)d[IR_OUT];
  const float *wy = table + (long long)d[IR_TAB];
  const float *wx = wy + (size_t)Ho * Ty;
  const int *fy = (const int *)(wx + (size_t)Wo * Tx);
  const int *fx = fy + Ho;
  const size_t HW = (size_t)H * W, HWo = (size_t)Ho * Wo;
  const int c0 = tile * kImreadTW, tw = min(kImreadTW, Wo - c0);
  ImreadColour col;
  imread_colour_load(d, col);
  float a3[3] = {0.f, 0.f, 0.f};
  if (avg_kind == 1)
    for (int c = 0; c < 3; ++c) a3[c] = avg[c];
  float tsum[3] = {0.f, 0.f, 0.f};

  for (int oa = 0; oa < Ho; oa += oc) {
    const int ob = min(oa + oc, Ho), no = ob - oa;
    const int base = fy[oa];
    const int rows = min(fy[ob - 1] + Ty - base, kImreadTileRows);
    // horizontal pass: lanes along the source column
    for (int i = tid; i < rows * tw * 3; i += 256) {
      const int j = i % rows, cc = i / rows, c = cc % tw, chn = cc / tw;
      const int sy = min(max(base + j, 0), H - 1);
      const float *src = pix + HW * chn + sy;
      const float *w = wx + (size_t)(c0 + c) * Tx;
      const int f = fx[c0 + c];
      float acc = 0.f;
      for (int t = 0; t < Tx; ++t) {
        const int sx = min(max(f + t, 0), W - 1);
        acc = fmaf(w[t], src[(size_t)H * sx], acc);
      }
      lds[(chn * kImreadTW + c) * kImreadTileRows + j] = acc;
    }
    __syncthreads();
    // vertical pass from LDS: lanes along the output column
    for (int i = tid; i < no * tw; i += 256) {
      const int oi = i % no, c = i / no, o = oa + oi;
      const int off = fy[o] - base;
      float v[3] = {0.f, 0.f, 0.f};
      for (int t = 0; t < Ty; ++t) {
        const float w = wy[(size_t)t * Ho + o];
        const int j = min(max(off + t, 0), kImreadTileRows - 1);
#pragma unroll
        for (int chn = 0; chn < 3; ++chn) v[chn] = fmaf(w, lds[(chn * kImreadTW + c) * kImreadTileRows + j], v[chn]);
      }
      const size_t q = o + (size_t)Ho * (c0 + c);
      if (avg_kind == 2)
        for (int chn = 0; chn < 3; ++chn) a3[chn] = avg[q + HWo * chn];
      const float p0 = v[0] - a3[0], p1 = v[1] - a3[1], p2 = v[2] - a3[2];
      if constexpr (CONTRAST) {
        o_img[q] = p0;
        o_img[q + HWo] = p1;
        o_img[q + 2 * HWo] = p2;
        tsum[0] += p0;
        tsum[1] += p1;
        tsum[2] += p2;
      } else {
        o_img[q] = imread_colour_apply(col.m, p0, p1, p2, col.k[0]);
        o_img[q + HWo] = imread_colour_apply(col.m + 3, p0, p1, p2, col.k[1]);
        o_img[q + 2 * HWo] = imread_colour_apply(col.m + 6, p0, p1, p2, col.k[2]);
      }
    }
    __syncthreads();
  }
  if constexpr (CONTRAST) {   // the block's sums, thread order fixed: a tree over the 256 threads per channel
    for (int chn = 0; chn < 3; ++chn) lds[chn * 256 + tid] = tsum[chn];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s)
        for (int chn = 0; chn < 3; ++chn) lds[chn * 256 + tid] += lds[chn * 256 + tid + s];
      __syncthreads();
    }
    if (tid < 3) partial[(long long)d[IR_PART] + 3 * tile + tid] = lds[tid * 256];
  }
}

__global__ __launch_bounds__(256) void imread_colour_kernel(const double *__restrict__ desc, const float *__restrict__ partial,
                                                             float *__restrict__ out) {
  __shared__ float add[3];
  const double *d = desc + (size_t)blockIdx.y * XM_IMREAD_ROW;
  const int Ho = (int)d[IR_HO], Wo = (int)d[IR_WO];
  const size_t HWo = (size_t)Ho * Wo;
  if ((size_t)blockIdx.x * 256 >= HWo) return;
  ImreadColour col;
  imread_colour_load(d, col);
  if (threadIdx.x == 0) {
    const float *p = partial + (long long)d[IR_PART];
    const int tiles = (int)d[IR_TILES];
    float m[3];
    for (int c = 0; c < 3; ++c) {
      float s = 0.f;
      for (int t = 0; t < tiles; ++t) s += p[3 * t + c];      // tile order
      m[c] = s / (float)HWo + (float)d[IR_B + c];              // mu of p - a + b
    }
    const float gamma = (float)d[IR_GAMMA], sigma = (float)d[IR_SIGMA];
    const float grey = (m[0] + m[1] + m[2]) / 3.f;
    for (int c = 0; c < 3; ++c) add[c] = fmaf(1.f - gamma, fmaf(sigma, m[c], (1.f - sigma) * grey), col.k[c]);
  }
  __syncthreads();
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= HWo) return;
  float *o_img = out + (long long)d[IR_OUT];
  const float p0 = o_img[q], p1 = o_img[q + HWo], p2 = o_img[q + 2 * HWo];
  o_img[q] = imread_colour_apply(col.m, p0, p1, p2, add[0]);
  o_img[q + HWo] = imread_colour_apply(col.m + 3, p0, p1, p2, add[1]);
  o_img[q + 2 * HWo] = imread_colour_apply(col.m + 6, p0, p1, p2, add[2]);
}

// min(max(floor(x + 1/2), 0), 255): the uint8 conversion that the narrow path applies inside its resampler, for callers
// that feed the unrounded outputs to a consumer of uint8 values (getImageBatch with a filter)
__global__ __launch_bounds__(256) void imread_round_kernel(const float *__restrict__ x, float *__restrict__ y, size_t n) {
  const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
  if (i < n) y[i] = fminf(fmaxf(floorf(x[i] + 0.5f), 0.f), 255.f);
}

}  // namespace xm

using namespace xm;

extern "C" {

int xm_imread_plan(const long long *hw, int N, const double *opts, const double *draws, double *rows, long long *sizes) {
  char msg[256];
  msg[0] = 0;
  const int rc = imread_plan_batch(hw, N, opts, draws, rows, sizes, msg, (int)sizeof msg);
  return rc ? fail(rc, "%s", msg) : XM_OK;
}

int xm_imread_geometry(int *launches, int *launches_contrast, int *tile_rows, int *tile_cols) {
  if (launches) *launches = 2;
  if (launches_contrast) *launches_contrast = 3;
  if (tile_rows) *tile_rows = kImreadTileRows;
  if (tile_cols) *tile_cols = kImreadTW;
  return XM_OK;
}

int xm_imread_round_u8(const float *x, long long n, float *y, void *stream) {
  if (n < 0) return fail(XM_EINVAL, "imread_round_u8: n must be >= 0 (got %lld)", n);
  if (n == 0) return XM_OK;
  if (!x || !y) return fail(XM_EINVAL, "imread_round_u8: NULL tensor");
  if (n >= (1LL << 39)) return fail(XM_ETOOBIG, "imread_round_u8: tensor too large");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(prof_key(kProfImread, 4), 0, st);
  hipLaunchKernelGGL(imread_round_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, y, (size_t)n);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_imread_transform_batch(const float *pixels, const double *desc, int N, const double *rows, const float *avg, float *out,
                              void *stream) {
  if (N < 0) return fail(XM_EINVAL, "imread_transform_batch: N must be >= 0 (got %d)", N);
  if (N == 0) return XM_OK;
  if (N > 32767) return fail(XM_ETOOBIG, "imread_transform_batch: at most 32767 images in a call (got %d)", N);
  if (!pixels || !desc || !rows || !out) return fail(XM_EINVAL, "imread_transform_batch: NULL argument");
  if (((uintptr_t)pixels & 3) || ((uintptr_t)desc & 7) || ((uintptr_t)out & 3) || ((uintptr_t)avg & 3))
    return fail(XM_EINVAL, "imread_transform_batch: pixels, avg and out must be 4-byte aligned, desc 8-byte");
  // the launch geometry comes from the host copy of the rows; each row is checked against what the plan writes
  long long tab = 0, part = 0, maxtiles = 0, maxout = 0, maxpix = 0;
  const bool contrast = rows[IR_CONTRAST] != 0;
  for (int i = 0; i < N; ++i) {
    const double *d = rows + (size_t)i * XM_IMREAD_ROW;
    const long long H = (long long)d[IR_H], W = (long long)d[IR_W], Ho = (long long)d[IR_HO], Wo = (long long)d[IR_WO];
    const long long Ty = (long long)d[IR_TY], Tx = (long long)d[IR_TX], oc = (long long)d[IR_OC], tiles = (long long)d[IR_TILES];
    const int filter = (int)d[IR_FILTER], kind = (int)d[IR_AVG];
    const bool ok = H >= 1 && W >= 1 && H <= kImreadMaxSide && W <= kImreadMaxSide && Ho >= 1 && Wo >= 1 && Ho <= kImreadMaxSide &&
                    Wo <= kImreadMaxSide && d[IR_PIX] >= 0 && d[IR_OUT] >= 0 && d[IR_TAB] == (double)tab && d[IR_PART] == (double)part &&
                    tiles == (Wo + kImreadTW - 1) / kImreadTW && d[IR_RY] > 0 && d[IR_RX] > 0 && d[IR_RY] <= kImreadMaxRatio &&
                    d[IR_RX] <= kImreadMaxRatio && d[IR_SY] >= 1 && d[IR_SX] >= 1 &&
                    (filter == XM_IMREAD_BOX || filter == XM_IMREAD_BILINEAR || filter == XM_IMREAD_BICUBIC) &&
                    Ty == imread_tap_count(filter, d[IR_SY]) && Tx == imread_tap_count(filter, d[IR_SX]) &&
                    oc == imread_chunk_rows(d[IR_RY], (int)Ty, (int)Ho) && oc >= 1 && kind >= 0 && kind <= 2 &&
                    (d[IR_CONTRAST] != 0) == contrast && kind == (int)rows[IR_AVG];
    if (!ok) return fail(XM_EINVAL, "imread_transform_batch: row %d is not a row of xm_imread_plan", i);
    if (kind && !avg) return fail(XM_EINVAL, "imread_transform_batch: the rows subtract an average and avg is NULL");
    if (kind == 2 && (Ho != (long long)rows[IR_HO] || Wo != (long long)rows[IR_WO]))
      return fail(XM_EINVAL, "imread_transform_batch: an average image needs outputs of one size (row %d)", i);
    tab += Ho * Ty + Wo * Tx + Ho + Wo;
    part += 3 * tiles;
    maxtiles = std::max(maxtiles, tiles);
    maxout = std::max(maxout, std::max(Ho, Wo));
    maxpix = std::max(maxpix, Ho * Wo);
  }
  hipStream_t st = (hipStream_t)stream;
  WsCarver ws;
  const int rc = ws.init(WsCarver::need((size_t)tab, 4) + WsCarver::need((size_t)part, 4), st);
  if (rc != XM_OK) return rc;
  float *table = ws.take<float>((size_t)tab);
  float *partial = ws.take<float>((size_t)part);
  {
    ProfScope ps(prof_key(kProfImread, 0), 0, st);
    hipLaunchKernelGGL(imread_table_kernel, dim3((unsigned)((maxout + 255) / 256), (unsigned)(2 * N)), dim3(256), 0, st, desc, table);
    XM_LAUNCH_CHECK();
  }
  {
    ProfScope ps(prof_key(kProfImread, contrast ? 2 : 1), 0, st);
    const dim3 grid((unsigned)maxtiles, (unsigned)N);
    if (contrast)
      hipLaunchKernelGGL(imread_resample_kernel<true>, grid, dim3(256), 0, st, pixels, desc, table, avg, out, partial);
    else
      hipLaunchKernelGGL(imread_resample_kernel<false>, grid, dim3(256), 0, st, pixels, desc, table, avg, out, partial);
    XM_LAUNCH_CHECK();
  }
  if (contrast) {
    ProfScope ps(prof_key(kProfImread, 3), 0, st);
    hipLaunchKernelGGL(imread_colour_kernel, dim3((unsigned)((maxpix + 255) / 256), (unsigned)N), dim3(256), 0, st, desc, partial, out);
    XM_LAUNCH_CHECK();
  }
  return XM_OK;
}

}  // extern "C"

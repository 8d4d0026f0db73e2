// vl_nnaffinegrid / vl_nnbilinearsampler (MatConvNet) and the fused FER+ batch of getBatchFerPlus on gfx950
// (teacher/ferplus_baselines.m:153-221).  All HBM-bound: a thread per output pixel (four in the fused batch kernel),
// writes coalesced along the first MATLAB dimension.  Semantics and the determinism of each output: include/xmodal.h,
// DESIGN.md section 7.
#include "xm_common.h"

namespace xm {

// linspace(-1, 1, n)(i) with MATLAB's linspace(-1, 1, 1) = 1: one correctly rounded division of two exact integers
__device__ __forceinline__ float lin11(int i, int n) {
  return n == 1 ? 1.f : (float)(2 * i - (n - 1)) / (float)(n - 1);
}

// grid(1) = c1 y + c3 x + c5 (Y), grid(2) = c2 y + c4 x + c6 (X); the one expression both the standalone grid and the
// fused batch kernel evaluate
__device__ __forceinline__ void affine_yx(const float *__restrict__ c, float y, float x, float &gy, float &gx) {
  gy = __fmaf_rn(c[0], y, __fmaf_rn(c[2], x, c[4]));
  gx = __fmaf_rn(c[1], y, __fmaf_rn(c[3], x, c[5]));
}

// normalised coordinate -> pixel coordinate p = (g + 1)(S - 1) / 2, in double from the fp32 grid value.  A position
// within (S - 1) 2^-25 of an integer -- twice the largest error an fp32 grid value carries -- is taken AS that
// integer, so that the identity grid lands exactly on the pixels (and returns X bit for bit) although its fp32
// linspace values are not exact.  (g + 1) * h is one add and one multiply: no contraction, the same double on the host.
struct Tap {
  int s;     // floor(p)
  float w;   // p - s
  bool out;  // no tap of this pixel is inside 0 <= s, s + 1 < S+1 (far outside, or a non-finite coordinate)
};
__device__ __forceinline__ Tap pix_tap(float g, int S) {
  const double h = 0.5 * (double)(S - 1);
  double p = ((double)g + 1.0) * h;
  const double r = rint(p);
  if (fabs(p - r) <= (double)(S - 1) * 0x1p-25) p = r;
  Tap t;
  t.out = !(p > -2.0 && p < (double)S + 1.0);
  const double s = t.out ? 0.0 : floor(p);
  t.s = (int)s;
  t.w = (float)(p - s);
  return t;
}

__global__ void __launch_bounds__(256)
affinegrid_kernel(const float *__restrict__ A, float *__restrict__ grid, int Ho, int Wo, int total) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int HW = Ho * Wo;
  const int n = idx / HW, q = idx - n * HW;
  const int j = q / Ho, i = q - j * Ho;
  float gy, gx;
  affine_yx(A + 6 * (size_t)n, lin11(i, Ho), lin11(j, Wo), gy, gx);
  grid[2 * (size_t)idx] = gy;
  grid[2 * (size_t)idx + 1] = gx;
}

// dA(:, n) = sum over the Ho x Wo pixels of [dG1 y, dG2 y, dG1 x, dG2 x, dG1, dG2]: one block per sample, per-thread
// partials in a fixed stride, wave shuffles, then the four waves in order through LDS -- no atomics, fixed bits
__global__ void __launch_bounds__(256)
affinegrid_backward_kernel(const float *__restrict__ dgrid, float *__restrict__ dA, int Ho, int Wo) {
  const int n = blockIdx.x;
  const int HW = Ho * Wo;
  const float *g = dgrid + 2 * (size_t)HW * n;
  float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int q = threadIdx.x; q < HW; q += 256) {
    const int j = q / Ho, i = q - j * Ho;
    const float y = lin11(i, Ho), x = lin11(j, Wo);
    const float d1 = g[2 * q], d2 = g[2 * q + 1];
    s[0] += d1 * y;
    s[1] += d2 * y;
    s[2] += d1 * x;
    s[3] += d2 * x;
    s[4] += d1;
    s[5] += d2;
  }
#pragma unroll
  for (int k = 0; k < 6; ++k)
    for (int off = 32; off > 0; off >>= 1) s[k] += __shfl_down(s[k], off, 64);
  __shared__ float part[4][6];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0)
    for (int k = 0; k < 6; ++k) part[wave][k] = s[k];
  __syncthreads();
  if (threadIdx.x < 6) {
    const int k = threadIdx.x;
    dA[6 * (size_t)n + k] = ((part[0][k] + part[1][k]) + part[2][k]) + part[3][k];
  }
}

// Y(i, j, c, m) = sum_{a,b} wy_a wx_b X(sy + a, sx + b, c, m / k), taps outside the image contribute 0
__global__ void __launch_bounds__(256)
sampler_forward_kernel(const float *__restrict__ x, const float *__restrict__ grid, float *__restrict__ y, int H, int W,
                       int C, int Ho, int Wo, int k, int total) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int HWo = Ho * Wo;
  const int m = idx / HWo, q = idx - m * HWo;
  const Tap ty = pix_tap(grid[2 * (size_t)idx], H), tx = pix_tap(grid[2 * (size_t)idx + 1], W);
  float *yo = y + (size_t)m * C * HWo + q;
  const bool out = ty.out || tx.out;
  // tap weights and offsets, hoisted out of the channel loop; an outside tap keeps weight 0 and offset 0
  float w[4];
  int o[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int a = t & 1, b = t >> 1;
    const int sy = ty.s + a, sx = tx.s + b;
    const bool in = !out && sy >= 0 && sy < H && sx >= 0 && sx < W;
    w[t] = in ? (a ? ty.w : 1.f - ty.w) * (b ? tx.w : 1.f - tx.w) : 0.f;
    o[t] = in ? sy + H * sx : 0;
  }
  const size_t HW = (size_t)H * W;
  const float *xi = x + (size_t)(m / k) * C * HW;
  for (int c = 0; c < C; ++c) {
    const float *p = xi + c * HW;
    float v = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (w[t] != 0.f) v += w[t] * p[o[t]];
    yo[(size_t)c * HWo] = v;
  }
}

// dX: w dY scattered into the taps with no-return global_atomic_add_f32 (arrival order decides the last bits);
// dGrid: the derivative of the forward formula with sy, sx held fixed, summed over C inside the thread (fixed bits)
__global__ void __launch_bounds__(256)
sampler_backward_kernel(const float *__restrict__ x, const float *__restrict__ grid, const float *__restrict__ dy,
                        float *__restrict__ dx, float *__restrict__ dgrid, int H, int W, int C, int Ho, int Wo, int k,
                        int total) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int HWo = Ho * Wo;
  const int m = idx / HWo, q = idx - m * HWo;
  const Tap ty = pix_tap(grid[2 * (size_t)idx], H), tx = pix_tap(grid[2 * (size_t)idx + 1], W);
  const bool out = ty.out || tx.out;
  float w[4];
  int o[4];
  bool in[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int a = t & 1, b = t >> 1;
    const int sy = ty.s + a, sx = tx.s + b;
    in[t] = !out && sy >= 0 && sy < H && sx >= 0 && sx < W;
    w[t] = in[t] ? (a ? ty.w : 1.f - ty.w) * (b ? tx.w : 1.f - tx.w) : 0.f;
    o[t] = in[t] ? sy + H * sx : 0;
  }
  const size_t HW = (size_t)H * W;
  const size_t img = (size_t)(m / k) * C * HW;
  const float *d = dy + (size_t)m * C * HWo + q;
  float gy = 0.f, gx = 0.f;
  for (int c = 0; c < C; ++c) {
    const float g = d[(size_t)c * HWo];
    if (dx) {
      float *p = dx + img + c * HW;
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (w[t] != 0.f) atomicAdd(p + o[t], w[t] * g);
    }
    if (dgrid && !out) {
      const float *p = x + img + c * HW;
      const float v00 = in[0] ? p[o[0]] : 0.f, v10 = in[1] ? p[o[1]] : 0.f;
      const float v01 = in[2] ? p[o[2]] : 0.f, v11 = in[3] ? p[o[3]] : 0.f;
      // d/dwy and d/dwx of the four-tap sum (tap t = a + 2 b: (sy + a, sx + b))
      gy += g * ((1.f - tx.w) * (v10 - v00) + tx.w * (v11 - v01));
      gx += g * ((1.f - ty.w) * (v01 - v00) + ty.w * (v11 - v10));
    }
  }
  if (dgrid) {
    dgrid[2 * (size_t)idx] = out ? 0.f : gy * (0.5f * (float)(H - 1));
    dgrid[2 * (size_t)idx + 1] = out ? 0.f : gx * (0.5f * (float)(W - 1));
  }
}

// getBatchFerPlus in one pass: grey H x W x 1 x N (0..255) -> optional fliplr -> grey x 3 minus averageImage ->
// affine grid of c1..c6 -> bilinear sampler, Ho x Wo x 3 x N.  The normalisation of the reference comes BEFORE the
// zero padding, so out_c = sum_in w (g - avg_c) = S - avg_c Omega over the in-bounds taps: sample once, write three.
__device__ __forceinline__ void ferplus_pixel(const float *__restrict__ p, const float *__restrict__ c, bool fl, int i,
                                              int j, int H, int W, int Ho, int Wo, float &S, float &Om) {
  float gy, gx;
  affine_yx(c, lin11(i, Ho), lin11(j, Wo), gy, gx);
  const Tap ty = pix_tap(gy, H), tx = pix_tap(gx, W);
  S = 0.f;
  Om = 0.f;
  if (ty.out || tx.out) return;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int a = t & 1, b = t >> 1;
    const int sy = ty.s + a, sx = tx.s + b;
    if (sy < 0 || sy >= H || sx < 0 || sx >= W) continue;
    const float w = (a ? ty.w : 1.f - ty.w) * (b ? tx.w : 1.f - tx.w);
    if (w == 0.f) continue;
    S += w * p[sy + H * (fl ? W - 1 - sx : sx)];
    Om += w;
  }
}

// one thread per output pixel (any Ho)
__global__ void __launch_bounds__(256)
ferplus_batch_kernel(const float *__restrict__ grey, const int *__restrict__ flip, const float *__restrict__ A,
                     float *__restrict__ out, int H, int W, int Ho, int Wo, int total, float a0, float a1, float a2) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int HWo = Ho * Wo;
  const int n = idx / HWo, q = idx - n * HWo;
  const int j = q / Ho, i = q - j * Ho;
  float S, Om;
  ferplus_pixel(grey + (size_t)H * W * n, A + 6 * (size_t)n, flip && flip[n], i, j, H, W, Ho, Wo, S, Om);
  float *o = out + (size_t)n * 3 * HWo + q;
  o[0] = S - a0 * Om;
  o[HWo] = S - a1 * Om;
  o[2 * (size_t)HWo] = S - a2 * Om;
}

// Ho % 4 == 0 and a 16-byte aligned output: four consecutive pixels of one column per thread, float4 stores
__global__ void __launch_bounds__(256)
ferplus_batch4_kernel(const float *__restrict__ grey, const int *__restrict__ flip, const float *__restrict__ A,
                      float *__restrict__ out, int H, int W, int Ho, int Wo, int total4, float a0, float a1, float a2) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total4) return;
  const int HWo4 = (Ho >> 2) * Wo;
  const int n = idx / HWo4, q4 = idx - n * HWo4;
  const int q = 4 * q4;
  const int j = q / Ho, i0 = q - j * Ho;
  const float *p = grey + (size_t)H * W * n;
  const float *c = A + 6 * (size_t)n;
  const bool fl = flip && flip[n];
  float S[4], Om[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) ferplus_pixel(p, c, fl, i0 + u, j, H, W, Ho, Wo, S[u], Om[u]);
  const size_t HWo = (size_t)Ho * Wo;
  float4 *o = reinterpret_cast<float4 *>(out + (size_t)n * 3 * HWo + q);
  o[0] = make_float4(S[0] - a0 * Om[0], S[1] - a0 * Om[1], S[2] - a0 * Om[2], S[3] - a0 * Om[3]);
  o[HWo / 4] = make_float4(S[0] - a1 * Om[0], S[1] - a1 * Om[1], S[2] - a1 * Om[2], S[3] - a1 * Om[3]);
  o[HWo / 2] = make_float4(S[0] - a2 * Om[0], S[1] - a2 * Om[1], S[2] - a2 * Om[2], S[3] - a2 * Om[3]);
}

static unsigned blocks_for(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace xm

using namespace xm;

extern "C" {

int xm_nnaffinegrid(const float *A, int N, int Ho, int Wo, float *grid, void *stream) {
  if (N <= 0 || Ho <= 0 || Wo <= 0) return fail(XM_EINVAL, "vl_nnaffinegrid: empty output");
  if (!A || !grid) return fail(XM_EINVAL, "vl_nnaffinegrid: NULL tensor");
  if (too_big(2, Ho, Wo, N)) return fail(XM_ETOOBIG, "vl_nnaffinegrid: grid with >= 2^31 elements");
  const int total = Ho * Wo * N;
  hipLaunchKernelGGL(affinegrid_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, A, grid, Ho, Wo,
                     total);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_nnaffinegrid_backward(const float *dgrid, int N, int Ho, int Wo, float *dA, void *stream) {
  if (N <= 0 || Ho <= 0 || Wo <= 0) return fail(XM_EINVAL, "vl_nnaffinegrid: empty output");
  if (!dgrid || !dA) return fail(XM_EINVAL, "vl_nnaffinegrid: NULL tensor");
  if (too_big(2, Ho, Wo, N)) return fail(XM_ETOOBIG, "vl_nnaffinegrid: grid with >= 2^31 elements");
  hipLaunchKernelGGL(affinegrid_backward_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, dgrid, dA, Ho,
                     Wo);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

static int sampler_check(const float *x, int H, int W, int C, int N, const float *grid, int Ho, int Wo, int No) {
  if (H <= 0 || W <= 0 || C <= 0 || N <= 0 || Ho <= 0 || Wo <= 0 || No <= 0)
    return fail(XM_EINVAL, "vl_nnbilinearsampler: empty tensor");
  if (No % N) return fail(XM_EINVAL, "vl_nnbilinearsampler: %d grids for %d images (must be a multiple)", No, N);
  if (!x || !grid) return fail(XM_EINVAL, "vl_nnbilinearsampler: NULL tensor");
  if (too_big(H, W, C, N) || too_big(Ho, Wo, C, No) || too_big(2, Ho, Wo, No))
    return fail(XM_ETOOBIG, "vl_nnbilinearsampler: tensor with >= 2^31 elements");
  return XM_OK;
}

int xm_nnbilinearsampler(const float *x, int H, int W, int C, int N, const float *grid, int Ho, int Wo, int No,
                         float *y, void *stream) {
  if (int rc = sampler_check(x, H, W, C, N, grid, Ho, Wo, No)) return rc;
  if (!y) return fail(XM_EINVAL, "vl_nnbilinearsampler: NULL tensor");
  const int total = Ho * Wo * No;
  hipLaunchKernelGGL(sampler_forward_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, x, grid, y,
                     H, W, C, Ho, Wo, No / N, total);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_nnbilinearsampler_backward(const float *x, int H, int W, int C, int N, const float *grid, int Ho, int Wo,
                                  int No, const float *dy, float *dx, float *dgrid, void *stream) {
  if (int rc = sampler_check(x, H, W, C, N, grid, Ho, Wo, No)) return rc;
  if (!dy) return fail(XM_EINVAL, "vl_nnbilinearsampler: NULL DY");
  if (!dx && !dgrid) return XM_OK;
  if (dx) XM_HIP(hipMemsetAsync(dx, 0, sizeof(float) * (size_t)H * W * C * N, (hipStream_t)stream));
  const int total = Ho * Wo * No;
  hipLaunchKernelGGL(sampler_backward_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, x, grid, dy,
                     dx, dgrid, H, W, C, Ho, Wo, No / N, total);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_ferplus_batch(const float *grey, int H, int W, int N, const int *flip, const float *A, int Ho, int Wo,
                     const float *avg3, float *out, void *stream) {
  if (H <= 0 || W <= 0 || N <= 0 || Ho <= 0 || Wo <= 0) return fail(XM_EINVAL, "ferplus_batch: empty tensor");
  if (!grey || !A || !avg3 || !out) return fail(XM_EINVAL, "ferplus_batch: NULL tensor");
  if (too_big(H, W, 1, N) || too_big(Ho, Wo, 3, N)) return fail(XM_ETOOBIG, "ferplus_batch: tensor too large");
  const int total = Ho * Wo * N;
  if (Ho % 4 == 0 && ((uintptr_t)out & 15) == 0)
    hipLaunchKernelGGL(ferplus_batch4_kernel, dim3(blocks_for(total / 4)), dim3(256), 0, (hipStream_t)stream, grey,
                       flip, A, out, H, W, Ho, Wo, total / 4, avg3[0], avg3[1], avg3[2]);
  else
    hipLaunchKernelGGL(ferplus_batch_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, grey, flip,
                       A, out, H, W, Ho, Wo, total, avg3[0], avg3[1], avg3[2]);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

}  // extern "C"

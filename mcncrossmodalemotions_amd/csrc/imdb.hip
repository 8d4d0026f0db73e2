// The logit bookkeeping of emoVoxCeleb/fetch_emovoxceleb_imdb.m:119-148 and emoVoxCeleb/sample_audio.m:69-74 on gfx950
// (the grouping itself, xm_group_rows, sits next to the radix passes it uses in roc.hip).
//
// xm_scatter_rows / xm_gather_rows: `logits(batch, :) = out'` (:130-131) and its inverse.  The packed side is
// 1 x 1 x E x n (a sample's E logits contiguous), the matrix is F x E column-major.  One thread per row walks the E
// columns.  On the matrix side consecutive lanes touch consecutive floats of a column when the rows are consecutive
// (a row list makes it a gather).  On the packed side the lanes of ONE load or store are E floats apart, so no single
// instruction is coalesced there; a wave's 64 E floats are contiguous only over the whole e loop and reach HBM as
// full lines through the cache.  Both run once per build (DESIGN.md section 10 has the measured cost).
//
// xm_track_peaks: one wave per track.  Lane l owns positions l, l + 64, ... of the track; per column the lanes read
// consecutive floats (contiguous tracks), keep a running fmaxf and the first strictly larger entry, then the column
// maximum is reduced with six xor shuffles and, once per track, the peak with six shuffle steps on the order
// (value, then lower emotion, then lower position).  Only comparisons: any reduction order gives the same bits.
#include "xm_common.h"

namespace xm {

constexpr int kRowThreads = 256;
constexpr int kPeakWaves = 4;   // tracks per workgroup

__global__ void __launch_bounds__(kRowThreads)
gather_rows_kernel(const float *__restrict__ mat, int F, int E, int row0, const int *__restrict__ rows, int n,
                   float *__restrict__ packed) {
  const size_t i = blockIdx.x * (size_t)kRowThreads + threadIdx.x;
  if (i >= (size_t)n) return;
  const long long row = rows ? (long long)rows[i] - 1 : (long long)row0 + (long long)i;
  const bool ok = row >= 0 && row < F;
  float *dst = packed + (size_t)E * i;
  for (int e = 0; e < E; ++e) dst[e] = ok ? mat[(size_t)row + (size_t)F * e] : __uint_as_float(0x7fc00000u);
}

__global__ void __launch_bounds__(kRowThreads)
scatter_rows_kernel(const float *__restrict__ packed, int n, int E, float *__restrict__ mat, int F, int row0,
                    const int *__restrict__ rows) {
  const size_t i = blockIdx.x * (size_t)kRowThreads + threadIdx.x;
  if (i >= (size_t)n) return;
  const long long row = rows ? (long long)rows[i] - 1 : (long long)row0 + (long long)i;
  if (row < 0 || row >= F) return;
  const float *src = packed + (size_t)E * i;
  for (int e = 0; e < E; ++e) mat[(size_t)row + (size_t)F * e] = src[e];
}

// (v, e, p) comes before (bv, be, bp): strictly larger, or equal and earlier in column-major order.  Neither value is
// ever NaN: a best starts at -Inf and is replaced only where v > best holds.
__device__ __forceinline__ bool peak_before(float v, int e, int p, float bv, int be, int bp) {
  return v > bv || (v == bv && (e < be || (e == be && p < bp)));
}

__global__ void __launch_bounds__(64 * kPeakWaves)
track_peaks_kernel(const float *__restrict__ lg, int F, int E, const int *__restrict__ offsets,
                   const int *__restrict__ rows, int T, int *__restrict__ frame_idx, int *__restrict__ tag,
                   float *__restrict__ maxed) {
  const int lane = threadIdx.x & 63;
  const size_t t = blockIdx.x * (size_t)kPeakWaves + (threadIdx.x >> 6);   // wave-uniform
  if (t >= (size_t)T) return;
  int a = offsets[t], b = offsets[t + 1];
  if (!rows) {
    a = max(a, 0);
    b = min(b, F);
  }
  const int len = (a >= 0 && b > a) ? b - a : 0;
  // the peak this lane has seen: value, emotion, position (0-based); "nothing above -Inf yet" = (-Inf, E, len)
  float bv = -INFINITY;
  int be = E, bp = len;
  float keep = -INFINITY;   // lane (e mod 64) keeps column e's maximum until it is stored
  for (int e = 0; e < E; ++e) {
    const float *col = lg + (size_t)F * e;
    float m = -INFINITY;
    for (int p = lane; p < len; p += 64) {
      long long row = rows ? (long long)rows[a + p] - 1 : (long long)a + p;
      if (row < 0 || row >= F) continue;
      const float v = col[row];
      m = fmaxf(m, v);
      if (v > bv) {   // positions ascend within a lane and columns ascend: the first strictly larger entry stays
        bv = v;
        be = e;
        bp = p;
      }
    }
    m = xm_wave_max(m);
    if ((e & 63) == lane) keep = m;
    if ((e & 63) == 63 || e == E - 1) {
      const int e0 = e & ~63;
      if (e0 + lane <= e) maxed[(size_t)E * t + e0 + lane] = keep;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oe = __shfl_xor(be, o, 64), op = __shfl_xor(bp, o, 64);
    if (peak_before(ov, oe, op, bv, be, bp)) {
      bv = ov;
      be = oe;
      bp = op;
    }
  }
  if (lane == 0) {
    // no entry above -Inf: max(x(:)) of MATLAB returns index 1 (all -Inf, or NaN passed over) -> frame 1, emotion 1
    const bool none = be == E;
    frame_idx[t] = len == 0 ? 0 : (none ? 1 : bp + 1);
    tag[t] = len == 0 ? 0 : (none ? 1 : be + 1);
  }
}

}  // namespace xm

using namespace xm;

extern "C" {

static int rows_args(const char *who, int n, int E, int F, int row0, const int *rows, const void *a, const void *b) {
  if (n < 0 || E < 1 || F < 1 || row0 < 0)
    return fail(XM_EINVAL, "%s: need n >= 0, E >= 1, F >= 1, row0 >= 0 (got n=%d E=%d F=%d row0=%d)", who, n, E, F, row0);
  if (n > 0 && (!a || !b)) return fail(XM_EINVAL, "%s: NULL tensor", who);
  if (!rows && (long long)row0 + n > F)
    return fail(XM_EINVAL, "%s: rows %d .. %lld do not fit a matrix of %d rows", who, row0 + 1, (long long)row0 + n, F);
  if (too_big(F, E) || too_big(n, E))
    return fail(XM_ENOTSUP, "%s: supported up to F * E < 2^31 and n * E < 2^31 (got F=%d n=%d E=%d)", who, F, n, E);
  return XM_OK;
}

int xm_gather_rows(const float *mat, int F, int E, int row0, const int *rows, int n, float *packed, void *stream) {
  int rc = rows_args("gather_rows", n, E, F, row0, rows, mat, packed);
  if (rc || n == 0) return rc;
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)(((size_t)n + kRowThreads - 1) / kRowThreads)),
                     dim3(kRowThreads), 0, (hipStream_t)stream, mat, F, E, row0, rows, n, packed);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_scatter_rows(const float *packed, int n, int E, float *mat, int F, int row0, const int *rows, void *stream) {
  int rc = rows_args("scatter_rows", n, E, F, row0, rows, packed, mat);
  if (rc || n == 0) return rc;
  hipLaunchKernelGGL(scatter_rows_kernel, dim3((unsigned)(((size_t)n + kRowThreads - 1) / kRowThreads)),
                     dim3(kRowThreads), 0, (hipStream_t)stream, packed, n, E, mat, F, row0, rows);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_track_peaks(const float *logits, int F, int E, const int *offsets, const int *rows, int T, int *frame_idx,
                   int *tag, float *maxed, void *stream) {
  if (F < 1 || E < 1 || T < 0)
    return fail(XM_EINVAL, "track_peaks: need F >= 1, E >= 1, T >= 0 (got F=%d E=%d T=%d)", F, E, T);
  if (T == 0) return XM_OK;
  if (!logits || !offsets || !frame_idx || !tag || !maxed) return fail(XM_EINVAL, "track_peaks: NULL tensor");
  if (too_big(F, E) || too_big(T, E))
    return fail(XM_ENOTSUP, "track_peaks: supported up to F * E < 2^31 and T * E < 2^31 (got F=%d T=%d E=%d)", F, T, E);
  hipLaunchKernelGGL(track_peaks_kernel, dim3((unsigned)(((size_t)T + kPeakWaves - 1) / kPeakWaves)),
                     dim3(64 * kPeakWaves), 0, (hipStream_t)stream, logits, F, E, offsets, rows, T, frame_idx, tag,
                     maxed);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

}  // extern "C"

// The pixel column of a FER2013-style CSV, parsed on gfx950 into the image array getBatchFerPlus gathers from
// (imdb = getFerPlusImdb(opts.dataDir), ferplus_baselines.m:103-110,181; benchmark_ferplus_models.m:15-17).
// include/xmodal.h documents the descriptor, the layout and the status words.
//
// xm_pixcsv_plan (host, no device call) is csrc/pixcsv_plan.h behind the C ABI.  xm_pixcsv_decode_batch is ONE launch of
//   pixcsv_decode_kernel  one block of 256 threads per row.  The field [begin, end) is walked in passes of kPixPass bytes
//                         that start at the 16-byte boundary at or below `begin`; a thread loads one aligned 16-byte
//                         vector per pass -- its index clamped to the vectors that hold bytes of the field -- and turns
//                         every byte outside the field into a space, the byte AT `end` included: that is the separator
//                         which closes a number the field ends with.  A number is counted where it ends: at a byte that
//                         is no digit and follows one.  The thread then looks BACK at most four bytes (three digits, and
//                         a fourth that makes the run too long), so all it needs from its neighbour is the last dword of
//                         the vector before its own: s_tail[t + 1] holds thread t's, s_tail[0] the last thread's of the
//                         pass before.  The running count, the tail and the flags are the whole carry between passes.
//                         popcount of the end marks, a wave scan with shuffles and a scan of the four wave totals give
//                         every number its index k.  An image of up to kPixStage floats is assembled in LDS -- the
//                         transposed position is an LDS address, the zeros of missing numbers too -- and leaves with
//                         consecutive lanes on consecutive floats; a larger one is stored from the threads directly.
//                         No atomics, no workspace; every output float has exactly one writer.
#include <algorithm>

#include "pixcsv_plan.h"
#include "prof.h"
#include "xm_common.h"

namespace xm {

constexpr int kPixThreads = 256;
constexpr int kPixPass = kPixThreads * 16;   // bytes per pass
constexpr int kPixStage = 4096;              // floats of an image assembled in LDS (16 KiB); FER's 48 x 48 is 2304
constexpr uint32_t kPixSpaces = 0x20202020u;

// the bytes [lo, hi) of a dword (both clamped to 0 .. 4) as a mask of 0xFF
__device__ __forceinline__ uint32_t pix_keep(int lo, int hi) {
  lo = min(max(lo, 0), 4);
  hi = min(max(hi, 0), 4);
  const uint32_t below_hi = hi >= 4 ? 0xFFFFFFFFu : ((1u << (8 * hi)) - 1u);
  const uint32_t below_lo = lo >= 4 ? 0xFFFFFFFFu : ((1u << (8 * lo)) - 1u);
  return below_hi & ~below_lo;
}

__device__ __forceinline__ long long pix_pos(long long k, int H, int W, int transpose) {
  if (!transpose) return k;
  if (k <= 0x7FFFFFFFLL) {   // the usual case in 32-bit arithmetic
    const unsigned r = (unsigned)k / (unsigned)W;
    return (long long)((unsigned)k - r * (unsigned)W) * H + r;
  }
  const long long r = k / W;
  return (k - r * W) * H + r;
}

__global__ void __launch_bounds__(kPixThreads)
pixcsv_decode_kernel(const uint4 *__restrict__ vecs, long long nbytes, const long long *__restrict__ desc, int H, int W,
                     int transpose, float *__restrict__ out, long long out_floats, int *__restrict__ status) {
  __shared__ uint32_t s_tail[kPixThreads + 1];
  __shared__ int s_wsum[kPixThreads / 64];
  __shared__ float s_img[kPixStage];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long long row = blockIdx.x;
  const long long *d = desc + row * XM_PIX_DESC;
  const long long img = d[PD_OUT];
  const long long HW = (long long)H * W;
  // block-uniform: a skipped row, or an image that does not lie inside [0, out_floats) (the host entry cannot see the
  // device descriptor; such a row writes no pixel and is flagged)
  if (img < 0 || img > (out_floats - HW) / HW) {
    if (t == 0) {
      status[2 * row] = 0;
      status[2 * row + 1] = img < 0 ? 0 : XM_PIX_NOFIT;
    }
    return;
  }
  float *__restrict__ dst = out + img * HW;
  const long long b = min(max(d[PD_BEGIN], 0LL), nbytes), e = min(max(d[PD_END], b), nbytes);
  const long long vmin = b >> 4, vmax = e > b ? (e - 1) >> 4 : vmin;   // the vectors that hold bytes of the field
  const long long a0 = b & ~15LL;
  const long long npass = (e - a0) / kPixPass + 1;                       // positions a0 .. e, the closing separator included
  const bool staged = HW <= kPixStage;
  long long running = 0;
  int flags = 0;
  if (t == 0) s_tail[0] = kPixSpaces;
  for (long long pass = 0; pass < npass; ++pass) {
    const long long A = a0 + pass * kPixPass + 16LL * t;                 // address of this thread's first byte
    uint32_t w[5];
    w[1] = w[2] = w[3] = w[4] = kPixSpaces;
    if (A < e && A + 16 > b) {
      const uint4 v = vecs[min(max(A >> 4, vmin), vmax)];
      const int lo = (int)max(b - A, 0LL), hi = (int)min(e - A, 16LL);
      const uint32_t raw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t m = pix_keep(lo - 4 * q, hi - 4 * q);
        w[1 + q] = (raw[q] & m) | (kPixSpaces & ~m);
      }
    }
    s_tail[t + 1] = w[4];
    __syncthreads();
    w[0] = s_tail[t];
    // bit j of dig: byte j of the 20-byte window (4 bytes of the neighbour, then the thread's 16) is a digit
    uint32_t dig = 0, bad = 0;
#pragma unroll
    for (int j = 0; j < 20; ++j) {
      const uint32_t c = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
      const bool isd = c - '0' <= 9u;
      dig |= (isd ? 1u : 0u) << j;
      if (j >= 4 && !isd && c != ' ' && c != '\t') bad = 1;
    }
    if (bad) flags |= XM_PIX_BADCHAR;
    const uint32_t marks = (~dig >> 4) & (dig >> 3) & 0xFFFFu;           // own byte i is no digit, the one before it is
    const int cnt = __popc(marks);
    int incl = cnt;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const int o = __shfl_up(incl, s, 64);
      if (lane >= s) incl += o;
    }
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int q = 0; q < kPixThreads / 64; ++q) {
      const int sq = s_wsum[q];
      if (q < wave) before += sq;
      total += sq;
    }
    if (t == kPixThreads - 1) s_tail[0] = w[4];                          // read by thread 0 behind the next pass's barrier
    long long k = running + before + (incl - cnt);
    running += total;
    if (marks) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (!((marks >> i) & 1u)) continue;
        // the number ends at window byte 3 + i
        const uint32_t c1 = (w[(3 + i) >> 2] >> (8 * ((3 + i) & 3))) & 0xFFu;
        const uint32_t c2 = (w[(2 + i) >> 2] >> (8 * ((2 + i) & 3))) & 0xFFu;
        const uint32_t c3 = (w[(1 + i) >> 2] >> (8 * ((1 + i) & 3))) & 0xFFu;
        int v = (int)(c1 - '0');
        if ((dig >> (2 + i)) & 1u) {
          v += 10 * (int)(c2 - '0');
          if ((dig >> (1 + i)) & 1u) {
            v += 100 * (int)(c3 - '0');
            if ((dig >> i) & 1u) v = 256;                                // a run of more than three digits
          }
        }
        if (v > 255) {
          v = 255;
          flags |= XM_PIX_RANGE;
        }
        if (k < HW) {
          const long long p = pix_pos(k, H, W, transpose);
          if (staged) s_img[p] = (float)v; else dst[p] = (float)v;
        }
        ++k;
      }
    }
  }
  // positions the field has no number for
  for (long long k = running + t; k < HW; k += kPixThreads) {
    const long long p = pix_pos(k, H, W, transpose);
    if (staged) s_img[p] = 0.0f; else dst[p] = 0.0f;
  }
  const int any_bad = __syncthreads_or(flags & XM_PIX_BADCHAR);          // also orders s_img before the copy below
  const int any_range = __syncthreads_or(flags & XM_PIX_RANGE);
  if (staged)
    for (int p = t; p < (int)HW; p += kPixThreads) dst[p] = s_img[p];
  if (t == 0) {
    status[2 * row] = (int)min(running, 2147483647LL);
    status[2 * row + 1] = (any_bad ? XM_PIX_BADCHAR : 0) | (any_range ? XM_PIX_RANGE : 0) | (running != HW ? XM_PIX_COUNT : 0);
  }
}

}  // namespace xm

using namespace xm;

extern "C" {

int xm_pixcsv_plan(const unsigned char *bytes, long long nbytes, long long *desc, long long max_rows, long long *sizes) {
  char msg[256];
  msg[0] = 0;
  const int rc = pixcsv_plan(bytes, nbytes, desc, max_rows, sizes, msg, (int)sizeof msg);
  return rc ? fail(rc, "%s", msg) : XM_OK;
}

int xm_pixcsv_geometry(int *bytes_per_pass, int *launches) {
  if (bytes_per_pass) *bytes_per_pass = kPixPass;
  if (launches) *launches = 1;
  return XM_OK;
}

int xm_pixcsv_decode_batch(const unsigned char *bytes, long long nbytes, const long long *desc, int N, int H, int W,
                           int transpose, float *out, long long out_floats, int *status, void *stream) {
  if (N < 0 || nbytes < 0 || out_floats < 0 || H < 0 || W < 0)
    return fail(XM_EINVAL, "pixcsv_decode_batch: need N, nbytes, H, W, out_floats >= 0 (got N=%d nbytes=%lld H=%d W=%d out_floats=%lld)",
                N, nbytes, H, W, out_floats);
  if (transpose != 0 && transpose != 1) return fail(XM_EINVAL, "pixcsv_decode_batch: transpose must be 0 or 1 (got %d)", transpose);
  if (N == 0) return XM_OK;
  if ((long long)H * W <= 0) return fail(XM_EINVAL, "pixcsv_decode_batch: an image of %d x %d has no pixel", H, W);
  if (!desc || !out || !status || (!bytes && nbytes > 0)) return fail(XM_EINVAL, "pixcsv_decode_batch: NULL argument");
  if (((uintptr_t)bytes & 15) || ((uintptr_t)desc & 7) || ((uintptr_t)out & 3) || ((uintptr_t)status & 3))
    return fail(XM_EINVAL, "pixcsv_decode_batch: bytes must be 16-byte aligned, desc 8-byte, out and status 4-byte aligned");
  if (out_floats < (long long)H * W)
    return fail(XM_EINVAL, "pixcsv_decode_batch: out_floats = %lld holds no image of %d x %d", out_floats, H, W);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(prof_key(kProfPixcsv), 0, st);
  hipLaunchKernelGGL(pixcsv_decode_kernel, dim3((unsigned)N), dim3(kPixThreads), 0, st, (const uint4 *)bytes, nbytes, desc, H, W,
                     transpose, out, out_floats, status);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

}  // extern "C"

// The whole-clip audio front-end of external/compute_audio_feats.m:160-185 for a batch of clips of different lengths:
// runSpec (pre-emphasis, Hamming window, 1024-point DFT magnitude), mean / unbiased std of every frequency row over ALL
// frames of the clip, and the centre crop to the bucket width -- xm_spec_bucket_batch (include/xmodal.h, ABI 112).
//
// The arithmetic is one GEMM, (all frames of all clips) x taps x 2B, whose frame operand is a Hankel view of the
// samples (row j = the samples shifted by hop * j) and is never written out.  Four launches whatever N and the lengths:
//   spec_bank_kernel    the filter bank (taps x 2B, tap fastest) transposed to [tap][column] so that the 32 columns of
//                       an MFMA B operand are 128 contiguous bytes; rows taps .. Kp - 1 are zero (Kp = taps made even)
//   spec_plan_kernel    frames and 64-frame tiles per clip from the descriptor table, exclusive prefix sum (one block)
//   spec_gemm_kernel    G blocks, block g owns the contiguous tile range [g q, (g + 1) q) of the flat (clip, tile) list
//                       (q = ceil(tiles / G)): equal work per block whatever the clip lengths are
//   spec_finish_kernel  statistics of a clip from the partial sums of the blocks that touched it, then every output
//                       element once: (mag - mu) / sd
// A tile is 64 frames x 2B columns.  The block stages the tile's contiguous sample span (63 hop + taps samples, 42 KB)
// in LDS once; sample s lives at s + floor(s / hop), so that frame i, tap k is at (hop + 1) i + k + floor(k / hop): the
// 32 frames of an A operand are hop + 1 = 161 words apart, an odd stride (hop itself, 160 = 32 mod 64, would put 16
// lanes on one bank).  Wave w computes, for the 32-bin tiles w, w + 4, w + 8, w + 12, the Re and Im columns of the
// same bins into accumulators of identical layout (v_mfma_f32_32x32x2_f32, frame on the row, bin on the lane), so the
// magnitude is an elementwise epilogue.
// Statistics: a lane sees 32 frames of one bin per tile; it takes their mean, then the centred sum of squares, in fp32
// (as spec_rownorm_kernel does over a whole row), and merges (count, mean, M2) into fp64 running values with Chan's
// update while the block stays inside one clip.  When the clip changes (and at the end of its range) the block writes
// (mean, M2) per bin to partial slot clip + block -- distinct for every (block, clip) pair because both grow along
// the tile list, and at most N + G of them -- and spec_finish_kernel merges a clip's slots in block order in fp64.  No
// atomics anywhere: the result is the same run to run.  The magnitudes inside the crop wait in the workspace for their
// statistics; frames outside it never leave the registers.
#include "prof.h"
#include "xm_common.h"

namespace xm {

typedef float spec_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kSpecFT = 64;        // frames per tile
constexpr int kSpecBins = 512;     // bins B the kernels are built for (2B = 1024 bank columns)
constexpr int kSpecPasses = kSpecBins / 128;
constexpr int kSpecChunk = 7;      // rounds of eight taps whose products form one fmaf chain
constexpr int kSpecOcc = 2;        // blocks per CU the grid is sized for (241 registers: two waves per SIMD)

// test switch behind xm_debug_set("spec_blocks", v): v >= 1 launches spec_gemm_kernel with min(v, 65535) blocks whatever
// the device is, so that a small input gives a block many tiles (tests/test_gpu_spec_edges.py); 0 = CUs x kSpecOcc
int g_spec_blocks = 0;

// T = floor((len - Nw) / Ns) + 1 frames, 0 for a clip shorter than one frame; len is cut at 2^31 samples
__device__ __forceinline__ long long spec_frames(long long len, int taps, int hop) {
  if (len > (1LL << 31)) len = 1LL << 31;
  return len < taps - 1 ? 0 : (len - (taps - 1)) / hop + 1;
}

__global__ void __launch_bounds__(256)
spec_bank_kernel(const float *__restrict__ bank, float *__restrict__ bT, int taps, int Kp, int cols) {
  __shared__ float tile[32][33];
  const int k0 = blockIdx.x * 32, c0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int c = c0 + r, k = k0 + tx;
    tile[r][tx] = (c < cols && k < taps) ? bank[k + (size_t)taps * c] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int k = k0 + r, c = c0 + tx;
    if (k < Kp && c < cols) bT[(size_t)k * cols + c] = tile[tx][r];
  }
}

__global__ void __launch_bounds__(1024)
spec_plan_kernel(const long long *__restrict__ desc, int N, int taps, int hop, long long *__restrict__ tile_start) {
  __shared__ long long scan[1024];
  const int tid = threadIdx.x, per = (N + 1023) / 1024;
  const int n0 = min(N, tid * per), n1 = min(N, n0 + per);
  long long sum = 0;
  for (int n = n0; n < n1; ++n) sum += (spec_frames(desc[3 * (size_t)n + 1], taps, hop) + kSpecFT - 1) / kSpecFT;
  scan[tid] = sum;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const long long v = tid >= o ? scan[tid - o] : 0;
    __syncthreads();
    scan[tid] += v;
    __syncthreads();
  }
  long long at = scan[tid] - sum;
  for (int n = n0; n < n1; ++n) {
    tile_start[n] = at;
    at += (spec_frames(desc[3 * (size_t)n + 1], taps, hop) + kSpecFT - 1) / kSpecFT;
  }
  if (tid == 1023) tile_start[N] = scan[1023];
}

// Chan's update of (count, mean, M2) by a group of nb values with mean mb and centred squares Mb
__device__ __forceinline__ void spec_merge(double &c, double &m, double &M2, double nb, double mb, double Mb) {
  if (nb <= 0.0) return;
  const double tot = c + nb, d = mb - m;
  m += d * (nb / tot);
  M2 += Mb + d * d * (c * nb / tot);
  c = tot;
}

__global__ void __launch_bounds__(256, 2)
spec_gemm_kernel(const float *__restrict__ wav, long long wav_len, const long long *__restrict__ desc, int N, int rsize,
                 const float *__restrict__ bT, int taps, int hop, const long long *__restrict__ tile_start,
                 double *__restrict__ part, float *__restrict__ raw) {
  extern __shared__ float smp[];
  constexpr int B = kSpecBins;
  const long long total = tile_start[N];
  const long long q = (total + gridDim.x - 1) / gridDim.x;
  const long long w0 = (long long)blockIdx.x * q, w1 = w0 + q < total ? w0 + q : total;
  if (w0 >= w1) return;
  int lo = 0, hi = N;                      // first index whose start is beyond w0; the clip of w0 is the one before
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tile_start[mid] > w0) hi = mid; else lo = mid + 1;
  }
  int n = lo - 1;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
  const int Kp = (taps + 1) & ~1, span = (kSpecFT - 1) * hop + taps;
  double rc[kSpecPasses], rm[kSpecPasses], rM[kSpecPasses];
#pragma unroll
  for (int p = 0; p < kSpecPasses; ++p) rc[p] = rm[p] = rM[p] = 0.0;

  for (long long w = w0;; ++w) {
    if (w == w1 || w >= tile_start[n + 1]) {           // the clip ends here for this block: its partial sums go out
      double *slot = part + ((size_t)n + blockIdx.x) * 2 * B;
#pragma unroll
      for (int p = 0; p < kSpecPasses; ++p) {
        const double oc = __shfl_xor(rc[p], 32, 64), om = __shfl_xor(rm[p], 32, 64), oM = __shfl_xor(rM[p], 32, 64);
        spec_merge(rc[p], rm[p], rM[p], oc, om, oM);
        if (h == 0) {
          const int b = 32 * (wv + 4 * p) + r;
          slot[b] = rm[p];
          slot[B + b] = rM[p];
        }
        rc[p] = rm[p] = rM[p] = 0.0;
      }
      if (w == w1) break;
      while (w >= tile_start[n + 1]) ++n;              // clips without a frame own no tile
    }
    const long long src = desc[3 * (size_t)n], f0 = desc[3 * (size_t)n + 2];
    long long len = desc[3 * (size_t)n + 1];
    if (len > (1LL << 31)) len = 1LL << 31;
    const long long T = spec_frames(len, taps, hop), t0 = (w - tile_start[n]) * kSpecFT;
    __syncthreads();                                   // the previous tile has been read
    for (int s = tid; s < span; s += 256) {
      const long long g = t0 * hop - 1 + s;            // sample of the clip; -1 is the rest state of the pre-emphasis
      float v = 0.f;
      if (g >= 0 && g < len) {
        const unsigned long long i = (unsigned long long)src + (unsigned long long)g;
        if (i < (unsigned long long)wav_len) v = wav[i];
      }
      smp[s + s / hop] = v;
    }
    __syncthreads();
    const int valid = T - t0 < kSpecFT ? (int)(T - t0) : kSpecFT;
    const int a0 = (hop + 1) * r, a1 = (hop + 1) * (r + 32);
#pragma unroll
    for (int p = 0; p < kSpecPasses; ++p) {
      const int b = 32 * (wv + 4 * p) + r;
      // acc: the fmaf chain of the current 56 taps (the MFMA's own order); sum: the chunks before it.  One chain over
      // all 401 taps misses a dominant bin's magnitude by about two of its ulps, which the row's std then divides.
      spec_f32x16 acc[2][2], sum[2][2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[i][j][e] = sum[i][j][e] = 0.f;
      int round = 0;
      const float *bp = bT + (size_t)h * 2 * B + b;
      int k = h, kr = h, kq = 0;                         // kq = floor(k / hop), carried along (hop >= 2)
      // four tap pairs per round: their eight LDS and eight global loads are issued before the sixteen MFMAs
      for (int k0 = 0; k0 < Kp; k0 += 8) {
        float xa[4], xb[4], bre[4], bim[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const bool on = k0 + 2 * u < Kp;               // the last round is short (Kp = 402: one pair)
          xa[u] = smp[a0 + k + kq];
          xb[u] = smp[a1 + k + kq];
          // a SELECT, not a product with a zero tap: beyond the staged span (and in the padding word after every
          // `hop` samples, which no tap index maps to) the LDS words were never written and may hold anything
          if (k >= taps || !on) xa[u] = xb[u] = 0.f;
          bre[u] = on ? bp[0] : 0.f;
          bim[u] = on ? bp[B] : 0.f;
          if (on) bp += (size_t)4 * B;
          k += 2;
          kr += 2;
          if (kr >= hop) {
            kr -= hop;
            ++kq;
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[u], bre[u], acc[0][0], 0, 0, 0);
          acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[u], bim[u], acc[0][1], 0, 0, 0);
          acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(xb[u], bre[u], acc[1][0], 0, 0, 0);
          acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(xb[u], bim[u], acc[1][1], 0, 0, 0);
        }
        if (++round == kSpecChunk || k0 + 8 >= Kp) {
          round = 0;
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              sum[i][j] += acc[i][j];
#pragma unroll
              for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
            }
        }
      }
      // magnitude; rows of the accumulator: (e & 3) + 8 (e >> 2) + 4 h (+ 32 i)
      float msum = 0.f;
      int cnt = 0;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = (e & 3) + 8 * (e >> 2) + 4 * h + 32 * i;
          const float re = sum[i][0][e], im = sum[i][1][e];
          const float mag = sqrtf(re * re + im * im);
          acc[i][0][e] = mag;
          if (row < valid) {
            msum += mag;
            ++cnt;
            const long long c = t0 + row - f0;
            if (c >= 0 && c < rsize) raw[((size_t)n * rsize + (size_t)c) * B + b] = mag;
          }
        }
      if (cnt > 0) {
        const float mean = msum / (float)cnt;
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int row = (e & 3) + 8 * (e >> 2) + 4 * h + 32 * i;
            const float d = acc[i][0][e] - mean;
            if (row < valid) ss += d * d;
          }
        spec_merge(rc[p], rm[p], rM[p], (double)cnt, (double)mean, (double)ss);
      }
    }
  }
}

__global__ void __launch_bounds__(256)
spec_finish_kernel(const long long *__restrict__ desc, int N, int rsize, int taps, int hop,
                   const long long *__restrict__ tile_start, const double *__restrict__ part, int G,
                   const float *__restrict__ raw, float *__restrict__ out) {
  constexpr int B = kSpecBins;
  const int n = blockIdx.y, tid = threadIdx.x;
  const long long f0 = desc[3 * (size_t)n + 2], T = spec_frames(desc[3 * (size_t)n + 1], taps, hop);
  const long long ts = tile_start[n], te = tile_start[n + 1], total = tile_start[N];
  const long long q = (total + G - 1) / G;
  const long long g_first = te > ts ? ts / q : 0, g_last = te > ts ? (te - 1) / q : -1;
  float mu[2], inv[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int b = tid + 256 * u;
    double c = 0.0, m = 0.0, M2 = 0.0;
    for (long long g = g_first; g <= g_last; ++g) {
      const long long lo = ts > g * q ? ts : g * q, hi = te < (g + 1) * q ? te : (g + 1) * q;
      const long long end = (hi - ts) * kSpecFT < T ? (hi - ts) * kSpecFT : T;
      const double *slot = part + ((size_t)n + (size_t)g) * 2 * B;
      spec_merge(c, m, M2, (double)(end - (lo - ts) * kSpecFT), slot[b], slot[B + b]);
    }
    // T < 2: NaN, as the std of one sample divides by zero
    mu[u] = T > 0 ? (float)m : __builtin_nanf("");
    inv[u] = (float)(1.0 / sqrt(M2 / (double)(T - 1)));
  }
  const int i1 = min(rsize, (int)(blockIdx.x + 1) * 16);
  for (int i = blockIdx.x * 16; i < i1; ++i) {
    const long long f = f0 + i;
    const bool in = f >= 0 && f < T;
    const size_t at = ((size_t)n * rsize + (size_t)i) * B;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int b = tid + 256 * u;
      out[at + b] = ((in ? raw[at + b] : 0.f) - mu[u]) * inv[u];
    }
  }
}

}  // namespace xm

using namespace xm;

extern "C" {

int xm_spec_bucket_batch(const float *wav, long long wav_len, const long long *desc, int N, int rsize, const float *bank,
                         int taps, int hop, int B, float *out, void *stream) {
  if (N < 0 || rsize <= 0 || wav_len < 0 || taps < 2 || hop < 2 || B <= 0)
    return fail(XM_EINVAL, "spec_bucket_batch: bad sizes");
  if (N == 0) return XM_OK;
  if (!wav || !desc || !bank || !out) return fail(XM_EINVAL, "spec_bucket_batch: NULL tensor");
  if (N > 65535) return fail(XM_ETOOBIG, "spec_bucket_batch: more than 65535 clips per call");
  const int Kp = (taps + 1) & ~1;
  // frame 63, tap Kp + 7 (the short last round of the tap loop reads on, and discards) is the last word touched
  const size_t lds = ((size_t)(hop + 1) * (kSpecFT - 1) + (Kp + 8) + (Kp + 8) / hop + 2) * sizeof(float);
  if (B != kSpecBins || lds > 64 * 1024)
    return fail(XM_ENOTSUP, "spec_bucket_batch: built for %d bins and a 64-frame sample span of at most 64 KB", kSpecBins);
  hipStream_t st = (hipStream_t)stream;
  int dev = 0, cus = 0;
  XM_HIP(hipGetDevice(&dev));
  XM_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const int G = g_spec_blocks >= 1 ? std::min(g_spec_blocks, 65535) : cus * kSpecOcc;
  const size_t slots = (size_t)N + G;
  WsCarver ws;
  int rc = ws.init(WsCarver::need((size_t)Kp * 2 * B, 4) + WsCarver::need((size_t)N + 1, 8) +
                       WsCarver::need(slots * 2 * B, 8) + WsCarver::need((size_t)N * rsize * B, 4), st);
  if (rc != XM_OK) return rc;
  float *bT = ws.take<float>((size_t)Kp * 2 * B);
  long long *tile_start = ws.take<long long>((size_t)N + 1);
  double *part = ws.take<double>(slots * 2 * B);
  float *raw = ws.take<float>((size_t)N * rsize * B);
  {
    ProfScope ps(prof_key(kProfSpec, 0), 0, st);
    hipLaunchKernelGGL(spec_bank_kernel, dim3((Kp + 31) / 32, 2 * B / 32), dim3(256), 0, st, bank, bT, taps, Kp, 2 * B);
  }
  XM_LAUNCH_CHECK();
  {
    ProfScope ps(prof_key(kProfSpec, 1), 0, st);
    hipLaunchKernelGGL(spec_plan_kernel, dim3(1), dim3(1024), 0, st, desc, N, taps, hop, tile_start);
  }
  XM_LAUNCH_CHECK();
  {
    ProfScope ps(prof_key(kProfSpec, 2), 0, st);
    hipLaunchKernelGGL(spec_gemm_kernel, dim3(G), dim3(256), lds, st, wav, wav_len, desc, N, rsize, bT, taps, hop,
                       tile_start, part, raw);
  }
  XM_LAUNCH_CHECK();
  {
    ProfScope ps(prof_key(kProfSpec, 3), 0, st);
    hipLaunchKernelGGL(spec_finish_kernel, dim3((rsize + 15) / 16, N), dim3(256), 0, st, desc, N, rsize, taps, hop,
                       tile_start, part, G, raw, out);
  }
  XM_LAUNCH_CHECK();
  return XM_OK;
}

}  // extern "C"

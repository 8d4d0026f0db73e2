// vl_nnconv forward / backward on gfx950 -- host-side planning + C ABI.
// Replaces MatConvNet's vl_nnconv MEX (matlab/src/vl_nnconv.cu, bits/nnconv.cu: im2row + SGEMM
// per image) behind the same operator contract; see include/xmodal.h and conv_kernels.h.
#include <dlfcn.h>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "conv_kernels.h"
#include "conv_tune.h"
#include "prof.h"

namespace xm {

// ---- small helper kernels -------------------------------------------------------------------

// zero-pad the filter bank [M][R] to [M][Rp] (only needed when R % 16 != 0: the two conv1 layers)
__global__ void pad_filter_kernel(const float *__restrict__ f, float *__restrict__ o, int M, int R,
                                  int Rp) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= (size_t)M * Rp) return;
  int r = (int)(i % Rp);
  size_t m = i / Rp;
  o[i] = r < R ? f[m * R + r] : 0.f;
}

// dgrad operand for one stride-parity class: At[c][iu + nU*(iv + nV*k)] = F[u(iu), v(iv), c, k]
// with u(iu) = u0 + iu*ustep (the taps whose u*dil == a mod sy), zero padded to lda columns.
// A (c <-> k) transpose of T-float elements through LDS: reads are contiguous runs of TS*T floats
// per output channel, writes contiguous runs of TS*nT floats per input channel.
// index arithmetic through magic-number division: with runtime `/` and `%` the kernel was bound by the integer
// division sequences (5 per element), 20 us per launch instead of the few us the bytes take
struct PrepDiv {
  FastDiv tsT, T, tsNT, nT, nU, padc, rows;
};
__global__ void __launch_bounds__(256)
prep_dgrad_filter_kernel(const float *__restrict__ f, float *__restrict__ o, int FH, int FW, int FC,
                         int Kg, int u0, int ustep, int nU, int v0, int vstep, int nV, int lda,
                         int TS, int fold, PrepDiv dv) {
  extern __shared__ float tile[];  // [kl][cl][t], kl pitch TS*T + 1
  const int T = FH * FW, nT = nU * nV;
  const int c0 = blockIdx.x * TS, k0 = blockIdx.y * TS;
  const int pitch = TS * T + 1;
  for (int i = threadIdx.x; i < TS * TS * T; i += 256) {
    int kl = (int)xm_div((uint32_t)i, dv.tsT), rem = i - kl * (TS * T);
    int cl = (int)xm_div((uint32_t)rem, dv.T);
    int c = c0 + cl, k = k0 + kl;
    tile[kl * pitch + rem] = (c < FC && k < Kg) ? f[(size_t)rem + (size_t)T * (c0 + (size_t)FC * k)] : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < TS * TS * nT; i += 256) {
    int cl = (int)xm_div((uint32_t)i, dv.tsNT), rem = i - cl * (TS * nT);
    int kl = (int)xm_div((uint32_t)rem, dv.nT), tt = rem - kl * nT;
    int iv = (int)xm_div((uint32_t)tt, dv.nU), iu = tt - iv * nU;
    int t = (u0 + iu * ustep) + FH * (v0 + iv * vstep);
    int c = c0 + cl, k = k0 + kl;
    if (c < FC && k < Kg) {
      // fold: one GEMM row per (filter row u, channel c); the reduction keeps only (iv, k)
      size_t dst = fold ? (size_t)(iu + nU * c) * lda + (size_t)nV * k + iv
                        : (size_t)c * lda + (size_t)nT * k + tt;
      o[dst] = tile[kl * pitch + cl * T + t];
    }
  }
  if (blockIdx.y == 0) {  // zero the K padding columns
    const int used = (fold ? nV : nT) * Kg, rows = fold ? nU : 1;
    int padc = lda - used;
    for (int i = threadIdx.x; i < TS * rows * padc; i += 256) {
      int rl = (int)xm_div((uint32_t)i, dv.padc), rr = used + (i - rl * padc);
      int cl = (int)xm_div((uint32_t)rl, dv.rows), ul = rl - cl * rows;
      if (c0 + cl < FC) o[((size_t)(c0 + cl) * rows + ul) * lda + rr] = 0.f;
    }
  }
}

// The FC-shaped layers' dgrad operand is a plain matrix transpose: At[r][k] = F[k][r] for a 1 x 1 filter (r = c) and for
// an H-collapsing FH x 1 filter folded into the GEMM rows (r = u + FH c) -- 110 of the 130 MB the student's filter
// preparation moves per step (fc6: 4096 x 2304, fc7: 1024 x 4096).  64 x 64 tiles through LDS, 16-byte accesses on both
// sides (the generic kernel above walks T-float runs element by element: ~1 TB/s).
__global__ void __launch_bounds__(256)
transpose_filter_kernel(const float *__restrict__ f, float *__restrict__ o, int K, int R, int ldo) {
  __shared__ float tile[64][65];
  const int r0 = blockIdx.x * 64, k0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;   // 16 float4 columns x 16 rows per pass
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int k = k0 + ty + 16 * p, r = r0 + 4 * tx;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k < K && r < R) v = *reinterpret_cast<const float4 *>(f + (size_t)k * R + r);   // R % 4 == 0
    tile[ty + 16 * p][4 * tx + 0] = v.x;
    tile[ty + 16 * p][4 * tx + 1] = v.y;
    tile[ty + 16 * p][4 * tx + 2] = v.z;
    tile[ty + 16 * p][4 * tx + 3] = v.w;
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int r = r0 + ty + 16 * p, k = k0 + 4 * tx;
    if (r < R && k < K) {                                                                // K % 4 == 0
      float4 v = make_float4(tile[4 * tx + 0][ty + 16 * p], tile[4 * tx + 1][ty + 16 * p],
                             tile[4 * tx + 2][ty + 16 * p], tile[4 * tx + 3][ty + 16 * p]);
      *reinterpret_cast<float4 *>(o + (size_t)r * ldo + k) = v;
    }
  }
}

// out[i] = sum_z part[z][i] in a FIXED order (deterministic): ZL "z-lanes" per output each sum a
// strided subset of the splits with four independent accumulators (loads in flight instead of one
// dependent chain), then the lanes are combined through LDS in lane order.
template <int ZL>
__global__ void __launch_bounds__(256)
reduce_splits_kernel(const float *__restrict__ part, float *__restrict__ out, size_t total, int splits,
                     size_t splitStride) {
  constexpr int OPB = 256 / ZL;
  const int ol = threadIdx.x % OPB, zl = threadIdx.x / OPB;
  const size_t i = blockIdx.x * (size_t)OPB + ol;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (i < total) {
    const float *p = part + i;
    int z = zl;
    for (; z + 3 * ZL < splits; z += 4 * ZL) {
      s0 += p[(size_t)z * splitStride];
      s1 += p[(size_t)(z + ZL) * splitStride];
      s2 += p[(size_t)(z + 2 * ZL) * splitStride];
      s3 += p[(size_t)(z + 3 * ZL) * splitStride];
    }
    for (; z < splits; z += ZL) s0 += p[(size_t)z * splitStride];
  }
  float s = (s0 + s1) + (s2 + s3);
  if (ZL == 1) {
    if (i < total) out[i] = s;
    return;
  }
  __shared__ float red[256];
  red[threadIdx.x] = s;
  __syncthreads();
  if (zl == 0 && i < total) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < ZL; ++k) t += red[k * OPB + ol];
    out[i] = t;
  }
}

static void launch_reduce_splits(const float *part, float *out, size_t total, int splits,
                                 size_t splitStride, hipStream_t st) {
  if (splits >= 64)
    hipLaunchKernelGGL(reduce_splits_kernel<16>, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, st,
                       part, out, total, splits, splitStride);
  else if (splits >= 8)
    hipLaunchKernelGGL(reduce_splits_kernel<4>, dim3((unsigned)((total + 63) / 64)), dim3(256), 0, st,
                       part, out, total, splits, splitStride);
  else
    hipLaunchKernelGGL(reduce_splits_kernel<1>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                       part, out, total, splits, splitStride);
}

// dzdb(k) = sum over pixels and samples of dzdy(:,:,k,:): grid (K, S) partial sums, then a
// fixed-order finalize (deterministic).  vec (the host's: HW % 4 == 0 and dy 16-byte aligned): 16-byte loads, divRun
// divides by HW / 4; else 4-byte loads and divRun divides by HW.
__global__ void __launch_bounds__(256)
bias_grad_partial_kernel(const float *__restrict__ dy, double *__restrict__ part, int HW, int K, int N,
                         int S, int vec, FastDiv divRun) {
  int k = blockIdx.x, sp = blockIdx.y;
  double s = 0.0;
  // flat (sample, position) index: FC-shaped layers (H*W = 8) keep all lanes busy
  const int nper = (N - sp + S - 1) / S;
  const int run = vec ? HW >> 2 : HW;
  for (int j = threadIdx.x; j < nper * run; j += 256) {
    const int nn = (int)xm_div((uint32_t)j, divRun), i = j - nn * run;
    const float *p = dy + (size_t)HW * (k + (size_t)K * (sp + nn * S));
    if (vec) {
      float4 v = reinterpret_cast<const float4 *>(p)[i];
      s += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
    } else {
      s += (double)p[i];
    }
  }
  __shared__ double red[4];
  s = xm_wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)k * S + sp] = red[0] + red[1] + red[2] + red[3];
}

__global__ void __launch_bounds__(256)
bias_grad_finalize_kernel(const double *__restrict__ part, float *__restrict__ db, int K, int S) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;  // one wave per channel
  if (k >= K) return;
  double s = 0.0;
  for (int i = lane; i < S; i += 64) s += part[(size_t)k * S + i];
  s = xm_wave_sum_d(s);
  if (lane == 0) db[k] = (float)s;
}

// batch moments from the convolution epilogue's partial sums (ConvGemmArgs::statPart, [pixel tile][row] pairs of fp32
// {sum, sum of squares} over <= 256 values each): fp64 accumulation over the pixel tiles in a fixed order.
// mom = [mean, sqrt(var + eps)] (M x 2).  Block = 8 channels x 32 tile lanes (a wave reads eight runs of 8 consecutive
// pairs): with 32 channels per block a 96-channel layer ran on THREE blocks whose lanes each walked ncg / 8 dependent
// loads -- 21-34 us for 0.5-2 MB.  grid (ceil(M / 8), S): S > 1 splits the tiles, the partial fp64 sums go to
// part2[s][M][2] and conv_stats_finalize2_kernel adds them.
__global__ void __launch_bounds__(256)
conv_stats_reduce_kernel(const float *__restrict__ part, float *__restrict__ mom, double *__restrict__ part2, int M,
                         int ncg, int S, double m, float eps) {
  const int cl = threadIdx.x & 7, j = threadIdx.x >> 3;
  const int c = blockIdx.x * 8 + cl, s = blockIdx.y;
  const int chunk = (ncg + S - 1) / S, g0 = s * chunk, g1 = min(ncg, g0 + chunk);
  double a = 0.0, b = 0.0;
  if (c < M)
    for (int g = g0 + j; g < g1; g += 32) {
      const float2 v = *reinterpret_cast<const float2 *>(part + ((size_t)g * M + c) * 2);
      a += (double)v.x;
      b += (double)v.y;
    }
  __shared__ double ra[32][8], rb[32][8];
  ra[j][cl] = a;
  rb[j][cl] = b;
  __syncthreads();
  if (j == 0 && c < M) {
#pragma unroll
    for (int k = 1; k < 32; ++k) a += ra[k][cl], b += rb[k][cl];
    if (S == 1) {
      const double mu = a / m;
      double var = b / m - mu * mu;
      var = var < 0.0 ? 0.0 : var;
      mom[c] = (float)mu;
      mom[M + c] = (float)sqrt(var + (double)eps);
    } else {
      part2[2 * ((size_t)s * M + c)] = a;
      part2[2 * ((size_t)s * M + c) + 1] = b;
    }
  }
}
__global__ void __launch_bounds__(256)
conv_stats_finalize2_kernel(const double *__restrict__ part2, float *__restrict__ mom, int M, int S, double m, float eps) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= M) return;
  double a = 0.0, b = 0.0;
  for (int s = 0; s < S; ++s) {
    a += part2[2 * ((size_t)s * M + c)];
    b += part2[2 * ((size_t)s * M + c) + 1];
  }
  const double mu = a / m;
  double var = b / m - mu * mu;
  var = var < 0.0 ? 0.0 : var;
  mom[c] = (float)mu;
  mom[M + c] = (float)sqrt(var + (double)eps);
}

// ---- tile configuration (the list itself: conv_tune.h) ----------------------------------------
// The eight-wave configuration is a candidate for launches of at least XM_W8_MIN_TILES 128 x 128 tiles (default: two rounds
// of the chip).  Measured (profiles/r04/schedule_experiments.txt): alone it is 3 ... 4 % faster at every size, but next to the
// filter derivatives of the side stream the shorter launches lose more than that (student step at 64 spectrograms - 3 %).
static inline bool w8_ok(long long M, long long NP) {
  static const long long min_tiles = env_int("XM_W8_MIN_TILES", 1024);
  return path_on(kPathW8) && ((M + 127) / 128) * ((NP + 127) / 128) >= min_tiles;
}
static inline unsigned w8_skip(long long M, long long NP) { return w8_ok(M, NP) ? 0u : 1u << 7; }
static inline unsigned cfg_threads(int ci) { return 64u * kCfgs[ci].wgm * kCfgs[ci].wgn; }
// analytic model: relative cost per multiply-add of a configuration (32 x 32 MFMA tiles per block; measured ordering)
static inline double cfg_eff(const Cfg &c) {
  const int t = c.tm * c.tn * c.wgm * c.wgn;
  return c.wgm * c.wgn == 8 ? 0.97 : (t >= 16 ? 1.0 : (t >= 8 ? 1.12 : 1.3));
}

static int g_force_splits = 0;  // test hook
// what the most recent launch_gemm left to conv_splitk_epilogue_kernel: 0 = nothing (the GEMM's own epilogue stored y), z > 0 =
// z partial slabs combined by the 16-byte form, z < 0 = |z| slabs by the scalar form (xm_debug_get("conv_last_combine"): tests)
static int g_last_combine = 0;
// read-only, for the tests of the reduction helpers (xm_debug_get): the final split count of the last wgrad_run /
// launch_wgrad_patch / launch_wgrad_patch_s2 ("wgrad_last_splits"), S of the last bias-derivative launch
// ("bias_grad_last_splits") and of the last forward_stats_reduce ("stats_last_splits": 0 when the most recent forward with
// batch moments took them from a pass over Y instead); "dgrad_last_transpose": 1 when the
// last dgrad filter operand was built by transpose_filter_kernel, 0 by prep_dgrad_filter_kernel; "dgrad_last_prepared": where
// the last dgrad call (not a prepare) had its filter operand from -- 1 the prepared cache, 0 built in the call, -1 a route
// without such an operand (conv_dgrad_s2_kernel, no stride class with taps)
static int g_last_wgrad_splits = 0, g_last_bias_splits = 0, g_last_stats_splits = 0, g_last_dgrad_transpose = 0;
static int g_last_dgrad_prepared = -1;

// With few output tiles the reduction is split over grid.y; the split count fills ONE round of
// 2 co-resident blocks per CU (no tail round).
static int pick_splits(int tiles, int nkt) {
  if (g_force_splits > 0) return std::max(1, std::min(g_force_splits, nkt));
  if (tiles >= 384 || nkt < 16) return 1;
  int s = 512 / tiles;
  s = std::min(s, nkt / 8);  // keep >= 8 stages per split
  return std::max(1, std::min(s, 64));
}

// Time model per tile configuration (seconds, coarse):
//   block time  = 2*BM*BN*16*stages*eff / (157.3 TF / 256 CUs)    (a CU's MFMA pipes are shared by
//                 its co-resident blocks, so >256 blocks cost proportionally more)
//   rounds      = 1 if blocks <= 256 else 2*ceil(blocks/512)
//   split-K adds the slab write + combine pass at HBM speed
static int pick_cfg(long long M, long long NP, int nkt) {
  double best = 1e300;
  int bi = 0;
  for (int i = 0; i < kNumBaseCfg; ++i) {
    if (i == kCfgW8 && !w8_ok(M, NP)) continue;
    const Cfg &c = kCfgs[i];
    long long tiles = ((M + c.bm() - 1) / c.bm()) * ((NP + c.bn() - 1) / c.bn());
    int s = pick_splits((int)std::min<long long>(tiles, 1 << 20), nkt);
    double eff = cfg_eff(c);
    double stages = (double)((nkt + s - 1) / s) + 3.0;  // + prologue / epilogue
    double t_block = 2.0 * c.bm() * c.bn() * 16.0 * stages * eff / (157.3e12 / 256.0);
    double blocks = (double)tiles * s;
    double rounds = blocks <= 256 ? 1.0 : 2.0 * std::ceil(blocks / 512.0);
    double t = rounds * t_block;
    if (s > 1) t += 5e-6 + (double)(s + 1) * M * NP * 4.0 / 4e12;
    if (t < best) {
      best = t;
      bi = i;
    }
  }
  return bi;
}

#ifndef XM_DMA_NST
#define XM_DMA_NST {4, 3, 4, 4}
#endif
#ifndef XM_DMA_PERCU
#define XM_DMA_PERCU {2, 2, 4, 4}
#endif
constexpr int kDmaStages[kNumCfg - kNumBaseCfg] = XM_DMA_NST;   // LDS stages of the LDS-DMA configurations (launch and name)
static void launch_gemm_dma(int ci, const ConvGemmArgs &a, dim3 grid, hipStream_t st) {
  dim3 block(256);
  switch (ci) {
    case kNumBaseCfg + 0: hipLaunchKernelGGL((conv_gemm_dma_kernel<2, 2, 2, 2, kDmaStages[0]>), grid, block, 0, st, a); break;
    case kNumBaseCfg + 1: hipLaunchKernelGGL((conv_gemm_dma_kernel<2, 2, 1, 4, kDmaStages[1]>), grid, block, 0, st, a); break;
    case kNumBaseCfg + 2: hipLaunchKernelGGL((conv_gemm_dma_kernel<1, 2, 2, 2, kDmaStages[2]>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((conv_gemm_dma_kernel<1, 1, 2, 2, kDmaStages[3]>), grid, block, 0, st, a); break;
  }
}

// prof.h: the kernel behind a key of launch_gemm (sub = ci * 2 + mode), wgrad_run (ci * 4 + log2 of the vector width) or
// launch_gemm_multi (ci * 2), for the values those sites can pass
bool conv_cfg_kernel_name(ProfKind kind, int sub, char *buf, int len) {
  const int per = kind == kProfWgrad ? 4 : 2, ci = sub / per, v = sub % per;
  const int ncfg = kind == kProfGemm ? kNumCfg : kind == kProfWgrad ? kNumWgradCfg : kNumBaseCfg;
  if (sub < 0 || ci >= ncfg || v > (kind == kProfGemm ? 1 : kind == kProfWgrad ? 2 : 0)) return false;
  const Cfg &c = kCfgs[ci];
  if (kind == kProfGemm && is_dma_cfg(ci))
    snprintf(buf, len, "conv_gemm_dma_kernel<%d, %d, %d, %d, %d>", c.tm, c.tn, c.wgm, c.wgn, kDmaStages[ci - kNumBaseCfg]);
  else if (kind == kProfGemm)
    snprintf(buf, len, "conv_gemm_kernel<%d, %d, %d, %d, %d>", c.tm, c.tn, c.wgm, c.wgn, v);
  else if (kind == kProfGemmMulti)
    snprintf(buf, len, "conv_gemm_multi_kernel<%d, %d, %d, %d>", c.tm, c.tn, c.wgm, c.wgn);
  else
    snprintf(buf, len, "conv_wgrad_kernel<%d, %d, %d, %d, %d>", c.tm, c.tn, c.wgm, c.wgn, 1 << v);
  return true;
}

template <int MODE>
static void launch_gemm_cfg(int ci, const ConvGemmArgs &a, dim3 grid, hipStream_t st) {
  dim3 block(cfg_threads(ci));
  switch (ci) {
    case 7: hipLaunchKernelGGL((conv_gemm_kernel<1, 2, 4, 2, MODE>), grid, block, 0, st, a); break;
    case 0: hipLaunchKernelGGL((conv_gemm_kernel<2, 2, 2, 2, MODE>), grid, block, 0, st, a); break;
    case 1: hipLaunchKernelGGL((conv_gemm_kernel<2, 2, 1, 4, MODE>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((conv_gemm_kernel<3, 1, 1, 4, MODE>), grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL((conv_gemm_kernel<1, 2, 2, 2, MODE>), grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL((conv_gemm_kernel<1, 1, 2, 2, MODE>), grid, block, 0, st, a); break;
    case 5: hipLaunchKernelGGL((conv_gemm_kernel<1, 1, 4, 1, MODE>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((conv_gemm_kernel<1, 1, 1, 4, MODE>), grid, block, 0, st, a); break;
  }
}

static int g_force_cfg = -1;  // test hook (xm_debug_force_conv_cfg)
int g_force_stem = -1;        // test hook (xm_debug_force_conv_stem): 1 = conv_stem_kernel wherever it can run, 0 = never (xm_common.h: stem_pool.hip reads it)
static int g_force_wgrad_patch = -1; // test hook (xm_debug_force_wgrad_patch)
// Execution hint of the HOST (xm_set_exec_hint, include/xmodal.h): XM_EXEC_SINGLE_STREAM = every operator call of the
// process arrives on one stream, so a kernel has the chip to itself -- conv_wgrad_patch_kernel (48 KB of LDS per block,
// three blocks per CU for its whole life) is a candidate only then (next to another stream's kernels it
// loses).  An explicit statement of the caller, never inferred: the kernel a shape gets is a function of (shape, table,
// hint) and of nothing the process did before.
static unsigned g_exec_hint = 0;
static int g_force_halo = -1; // test hook (xm_debug_force_conv_halo): 1 = halo-patch kernel wherever it can run, 0 = never
static unsigned long long *g_dbg_cycles = nullptr;  // device buffer, set by xm_debug_conv_cycles(1)

// co-resident blocks per CU of the register-staged configurations (VGPR-limited: 222 / 232 / 186 / 140 / 116 / 134 / 122 /
// 128 with eight waves)
static const int kCfgOcc[kNumBaseCfg] = {2, 2, 2, 3, 4, 3, 4, 2};

// Hybrid schedule (ConvGemmArgs::hyS): a launch of more than one round of the chip whose LAST round is partly filled
// computes the full rounds tile by tile and splits the remaining tiles along the reduction so that they fill the last
// round with short blocks -- 3.06 rounds cost 3.06 + 1/S instead of 4.  Returns the split count of the remainder (1: plain).
static int hybrid_plan(const ConvGemmArgs &a, int ci, int *full_out) {
  const bool off = !path_on(kPathHybrid);
  *full_out = 0;
  if (off || is_dma_cfg(ci) || g_force_splits > 0) return 1;
  if (a.rsOn) return 1;       // (a strided-residual launch keeps ONE reduction chain per output: see gemm_slab_floats)
  if (a.statPart && (!a.vecStore || a.relu || a.resid)) return 1;   // conv_splitk_epilogue_stats_kernel's case only
  const int tiles = a.nbm * a.nbn, slots = 256 * kCfgOcc[ci];
  if (tiles <= slots || a.nkt < 16) return 1;
  int full = tiles / slots * slots;
  full -= full % a.nbm;                       // the remainder is a whole range of pixel tiles
  const int rem = tiles - full;
  if (rem <= 0 || rem * 5 > slots * 4) return 1;     // a last round that is > 80 % full is left alone
  const int S = std::min(std::min(slots / rem, a.nkt / 8), 16);
  if (S < 2) return 1;
  *full_out = full;
  return S;
}

static size_t gemm_slab_floats(const ConvGemmArgs &a, int ci, int *splits_out) {
  const Cfg &c = kCfgs[ci];
  int nbm = (a.M + c.bm() - 1) / c.bm(), nbn = (a.NP + c.bn() - 1) / c.bn();
  int splits = pick_splits(nbm * nbn, a.Rp / kBK);
  // A strided-residual launch is the full-extent layer computed at a quarter (1 / s^2) of its pixels, and it has to give those
  // pixels the values the full-extent launch gives them.  That launch has tiles enough to run unsplit, so neither the fewer
  // tiles of the pruned launch (split-K) nor a partly filled last round (hybrid_plan) may cut its reduction into partial sums:
  // with a configuration of the same chain structure (one accumulator chain, or the two of the 1 x 1 wave tiles) the results
  // are then the same bits.  The launch is a few hundred short blocks either way.  (The test hook still forces a split.)
  if (a.rsOn && g_force_splits <= 0) splits = 1;
  *splits_out = splits;
  size_t need = splits > 1 ? (size_t)splits * a.M * ((a.NP + 3) & ~3) : 0;
  if (splits == 1 && !is_dma_cfg(ci)) {
    // hybrid remainder: at most one round of tiles, up to 16 partial copies of each
    ConvGemmArgs t = a;
    t.nbm = nbm, t.nbn = nbn, t.nkt = a.Rp / kBK;
    t.statPart = nullptr;
    int full;
    const int S = hybrid_plan(t, ci, &full);
    if (S > 1) need = std::max(need, (size_t)S * a.M * ((size_t)(nbm * nbn - full) / nbm * c.bn() + 4));
  }
  return need;
}

// combines the z partial slabs over `np` pixels in a fixed order (vec: pixel quads)
static void launch_splitk_epilogue(const ConvGemmArgs &a, int z, int np, bool vec, hipStream_t st) {
  const int cols = vec ? np / 4 : np;
  const dim3 grid((unsigned)(((size_t)a.M * cols + 255) / 256));
  if (vec) hipLaunchKernelGGL(conv_splitk_epilogue_kernel<true>, grid, dim3(256), 0, st, a, z, make_fastdiv((uint32_t)cols));
  else hipLaunchKernelGGL(conv_splitk_epilogue_kernel<false>, grid, dim3(256), 0, st, a, z, make_fastdiv((uint32_t)cols));
}

static int launch_gemm(ConvGemmArgs &a, int mode, int ci, int splits, float *slab, hipStream_t st) {
  if (is_dma_cfg(ci) && !a.dmaOk) ci = base_cfg(ci);   // forced configuration on a geometry it cannot run
  if (ci == kCfgW8 && !path_on(kPathW8)) ci = 0;
  const Cfg &c = kCfgs[ci];
  a.nbm = (a.M + c.bm() - 1) / c.bm();
  a.nbn = (a.NP + c.bn() - 1) / c.bn();
  a.nkt = a.Rp / kBK;
  a.tilesPerSplit = (a.nkt + splits - 1) / splits;
  splits = (a.nkt + a.tilesPerSplit - 1) / a.tilesPerSplit;
  a.NPs = (a.NP + 3) & ~3;
  a.slab = splits > 1 ? slab : nullptr;
  a.dbgCycles = g_dbg_cycles;
  a.hyS = 1, a.hyFull = 0, a.hyTps = 0, a.hyP0 = 0;
  dim3 grid(a.nbm * a.nbn, splits);
  int hyS = 1;
  if (splits == 1 && slab) {
    int full;
    hyS = hybrid_plan(a, ci, &full);
    if (hyS > 1) {
      a.hyFull = full;
      a.hyTps = (a.nkt + hyS - 1) / hyS;
      hyS = (a.nkt + a.hyTps - 1) / a.hyTps;
      a.hyS = hyS;
      a.hyP0 = full / a.nbm * c.bn();
      a.NPs = (a.NP - a.hyP0 + 3) & ~3;
      a.slab = slab;
      grid = dim3(full + (a.nbm * a.nbn - full) * hyS, 1);
    }
  }
  {
    const double abytes = (double)a.xBytes + 4.0 * a.M * a.Rtrue + 4.0 * a.M * (double)a.NP * (a.resid ? 2 : 1);
    ProfScope ps(prof_key(kProfGemm, ci * 2 + mode), a.algoFlops > 0 ? a.algoFlops : 2.0 * a.M * (double)a.NP * a.Rtrue, st,
                 abytes);
    if (is_dma_cfg(ci)) {
      // persistent: one round of co-resident blocks (a multiple of 8 so that every XCD gets the same share)
      static const int per_cu_tab[] = XM_DMA_PERCU;          // co-resident blocks per CU (LDS-limited)
      const int slots = std::max(8, 256 * per_cu_tab[ci - kNumBaseCfg] / std::max(1, splits));
      const int ntl = a.nbm * a.nbn;
      const int g = ntl <= slots ? ntl : slots - slots % 8;
      launch_gemm_dma(ci, a, dim3(std::max(1, g), splits), st);
    } else if (mode)
      launch_gemm_cfg<1>(ci, a, grid, st);
    else
      launch_gemm_cfg<0>(ci, a, grid, st);
  }
  XM_LAUNCH_CHECK();
  g_last_combine = 0;
  if (splits > 1 || hyS > 1) {
    const int z = splits > 1 ? splits : hyS;
    const int np = a.NP - a.hyP0;                       // pixels the slabs cover
    const bool vec = a.vecStore && (np & 3) == 0 && (a.hyP0 & 3) == 0 && (a.NPs & 3) == 0 && ((uintptr_t)a.slab & 15) == 0;
    if (hyS > 1 && a.statPart) {
      // the full rounds left their partial sums per pixel tile; the remainder's come from the combine kernel
      const int cols = np / 4, chunks = (cols + 255) / 256, statBase = a.hyFull / a.nbm;
      if (!vec) return fail(XM_EINVAL, "vl_nnconv: hybrid schedule with statistics needs vector stores");
      hipLaunchKernelGGL(conv_splitk_epilogue_stats_kernel, dim3(chunks, a.M), dim3(256), 0, st, a, z, cols, statBase);
      a.statNcg = statBase + chunks;
    } else
      launch_splitk_epilogue(a, z, np, vec, st);
    g_last_combine = vec ? z : -z;
    XM_LAUNCH_CHECK();
  }
  return XM_OK;
}

static void launch_gemm_multi_cfg(int ci, const ConvGemmMulti &m, dim3 grid, hipStream_t st) {
  dim3 block(cfg_threads(ci));
  switch (ci) {
    case 7: hipLaunchKernelGGL((conv_gemm_multi_kernel<1, 2, 4, 2>), grid, block, 0, st, m); break;
    case 0: hipLaunchKernelGGL((conv_gemm_multi_kernel<2, 2, 2, 2>), grid, block, 0, st, m); break;
    case 1: hipLaunchKernelGGL((conv_gemm_multi_kernel<2, 2, 1, 4>), grid, block, 0, st, m); break;
    case 2: hipLaunchKernelGGL((conv_gemm_multi_kernel<3, 1, 1, 4>), grid, block, 0, st, m); break;
    case 3: hipLaunchKernelGGL((conv_gemm_multi_kernel<1, 2, 2, 2>), grid, block, 0, st, m); break;
    case 4: hipLaunchKernelGGL((conv_gemm_multi_kernel<1, 1, 2, 2>), grid, block, 0, st, m); break;
    case 5: hipLaunchKernelGGL((conv_gemm_multi_kernel<1, 1, 4, 1>), grid, block, 0, st, m); break;
    default: hipLaunchKernelGGL((conv_gemm_multi_kernel<1, 1, 1, 4>), grid, block, 0, st, m); break;
  }
}

// up to 4 masked (MODE 1) implicit GEMMs without split-K in one launch, same tile configuration
static int launch_gemm_multi(const std::vector<ConvGemmArgs> &args, int ci, hipStream_t st) {
  ci = base_cfg(ci);
  if (ci == kCfgW8 && !path_on(kPathW8)) ci = 0;
  const Cfg &c = kCfgs[ci];
  ConvGemmMulti m{};
  int maxTiles = 0;
  double flops = 0, abytes = args.empty() ? 0.0 : (double)args[0].xBytes;   // the classes share one source tensor
  for (size_t i = 0; i < args.size(); ++i) {
    ConvGemmArgs a = args[i];
    a.nbm = (a.M + c.bm() - 1) / c.bm();
    a.nbn = (a.NP + c.bn() - 1) / c.bn();
    a.nkt = a.Rp / kBK;
    a.tilesPerSplit = a.nkt;
    a.NPs = (a.NP + 3) & ~3;
    a.slab = nullptr;
    maxTiles = std::max(maxTiles, a.nbm * a.nbn);
    flops += a.algoFlops > 0 ? a.algoFlops : 2.0 * a.M * (double)a.NP * a.Rtrue;
    abytes += 4.0 * a.M * a.Rtrue + 4.0 * a.M * (double)a.NP * (a.resid ? 2 : 1);
    m.c[i] = a;
  }
  {
    ProfScope ps(prof_key(kProfGemmMulti, ci * 2), flops, st, abytes);
    launch_gemm_multi_cfg(ci, m, dim3(maxTiles, 1, (unsigned)args.size()), st);
  }
  XM_LAUNCH_CHECK();
  return XM_OK;
}

// ---- halo-patch kernels (conv_halo_kernel / conv_halo_multi_kernel): <= 3 x 3 taps, unit pixel stride ---------------
// Variants: 0 = 128-row tiles (2 x 2 wave tiles), patch 512;  1 = 96-row tiles (3 x 1), patch 512;
//           2 = 96-row tiles, patch 1024 (tall columns: the student's conv2 dgrad classes have 65-row patch columns)
struct HaloVar {
  int bm, ps;
};
static const HaloVar kHaloVars[] = {{128, 512}, {96, 512}, {96, 1024}};
static const float kHaloMargin = (float)env_double("XM_HALO_MARGIN", 0.04);

// fills the patch geometry of `a` (an implicit-GEMM problem already described by its tap / gather fields) and returns
// the patch floats per channel the widest 128-pixel tile needs (0: the kernel cannot run this problem): taps in an
// nU x nV <= 3 x 3 arrangement of 9 / 6 / 4, adjacent rows / columns, unit pixel stride, channels a multiple of 8.
static int halo_setup(ConvGemmArgs &a, int nSamples) {
  const bool off = !path_on(kPathHalo);
  const int T = a.nU * a.nV;
  if (off || a.nU < 1 || a.nU > 3 || a.nV < 1 || a.nV > 3 || (T != 9 && T != 6 && T != 4)) return 0;
  if (a.gsy != 1 || a.gsx != 1 || std::abs(a.dus) != 1 || std::abs(a.dvs) != 1) return 0;
  const int KS = kHaloCB * T;
  if (a.Rtrue % KS != 0 || a.Rtrue < KS || (a.lda & 3) || ((uintptr_t)a.A & 15)) return 0;
  if (a.divMU.d != 1) return 0;
  const int rlo = a.gh0 + a.du0 + std::min(0, (a.nU - 1) * a.dus), clo = a.gw0 + a.dv0 + std::min(0, (a.nV - 1) * a.dvs);
  a.hpRmin = rlo;
  a.hpCmin = clo;
  a.hpHP = a.PI + a.nU - 1;
  a.hpWP = a.PJ + a.nV - 1;
  a.hpN = nSamples;
  for (int iv = 0; iv < a.nV; ++iv)
    for (int iu = 0; iu < a.nU; ++iu) {
      const int su = a.gh0 + a.du0 + iu * a.dus - rlo, sv = a.gw0 + a.dv0 + iv * a.dvs - clo;
      a.hpSh[iu + a.nU * iv] = (su + a.hpHP * sv) * 4;
    }
  a.hpDivHP = make_fastdiv((uint32_t)a.hpHP);
  a.hpDivWP = make_fastdiv((uint32_t)a.hpWP);
  // widest patch over all 128-pixel tiles: padded columns of the first and the last pixel of the tile + the taps
  const int BN = 128, pij = a.PI * a.PJ;
  int worst = 0;
  for (long long p0 = 0; p0 < a.NP; p0 += BN) {
    const long long p1 = std::min<long long>(p0 + BN - 1, a.NP - 1);
    const long long c0 = (p0 / pij) * a.hpWP + (p0 % pij) / a.PI, c1 = (p1 / pij) * a.hpWP + (p1 % pij) / a.PI;
    worst = std::max(worst, (int)(c1 - c0) + a.nV);
  }
  return worst * a.hpHP;
}
// Tall pixel grids (the student's conv2 dgrad classes: 63 / 62 rows) put 3-4 columns + taps + a sample gap under a
// 128-pixel tile -- more than 512 patch floats.  Enumerating the pixels with PI rounded up to a multiple of 32 makes a tile
// a whole number of columns (2 of 64): the patch shrinks below 512 floats and the 96-row / 512 variant (3 blocks per CU,
// half the patch loads) applies; the non-existent rows (1.6 %) are computed and dropped in the epilogue (piReal).
// Only for scalar-store problems whose padding waste stays under 4 %.
static int halo_setup_padded(ConvGemmArgs &a, int nSamples) {
  int need = halo_setup(a, nSamples);
  if (need <= 512 || a.vecStore || a.slab) return need;
  const int piv = (a.PI + 31) / 32 * 32;
  if (piv == a.PI || (piv - a.PI) * 25 > piv || (long long)piv * a.PJ * nSamples >= (1LL << 31)) return need;
  ConvGemmArgs b = a;
  b.piReal = a.PI;
  b.PI = piv;
  b.NP = piv * a.PJ * nSamples;
  b.divPI = make_fastdiv((uint32_t)piv);
  b.divPIJ = make_fastdiv((uint32_t)(piv * a.PJ));
  const int need2 = halo_setup(b, nSamples);
  if (need2 > 0 && need2 <= 512) {
    a = b;
    return need2;
  }
  return need;
}

static bool halo_var_ok(const ConvGemmArgs &a, int need, int v) {
  if (need <= 0 || need > kHaloVars[v].ps) return false;
  if (v == 2 && need <= 512) return false;                       // variant 1 covers it with half the patch loads
  if (kHaloVars[v].bm == 96 && (a.M % 96 != 0)) return false;    // 96-row tiles only where they waste nothing
  return true;
}

// split-K: stages of 8 T reduction steps; one round of 2 blocks per CU, >= 4 stages per split
static int halo_splits(const ConvGemmArgs &a, int v) {
  const int bm = kHaloVars[v].bm;
  const int tiles = ((a.M + bm - 1) / bm) * ((a.NP + 127) / 128), nst = a.Rtrue / (kHaloCB * a.nU * a.nV);
  if (tiles >= 384 || nst < 8) return 1;
  return std::max(1, std::min(std::min(512 / tiles, nst / 4), 16));
}
static size_t halo_slab_floats(const ConvGemmArgs &a) {
  int sp = 1;
  for (int v = 0; v < 3; ++v) sp = std::max(sp, halo_splits(a, v));
  return sp > 1 ? (size_t)sp * a.M * ((a.NP + 3) & ~3) : 0;
}

static void halo_prepare(ConvGemmArgs &a, int v) {
  const int bm = kHaloVars[v].bm;
  a.nbm = (a.M + bm - 1) / bm, a.nbn = (a.NP + 127) / 128;
  a.nkt = a.Rtrue / (kHaloCB * a.nU * a.nV);   // stages (the split-K bookkeeping of the kernel counts in these)
  a.tilesPerSplit = a.nkt, a.NPs = (a.NP + 3) & ~3, a.slab = nullptr, a.dbgCycles = nullptr;
}

// test hook: xm_debug_force_conv_halo(1 + v) asks for variant v, any other runnable one if v cannot take the problem
static int forced_halo_variant(const bool *hok) {
  if (g_force_halo >= 1 && g_force_halo <= 3 && hok[g_force_halo]) return g_force_halo;
  return hok[2] ? 2 : (hok[1] ? 1 : 3);
}
static int halo_forced(const bool *hok) { return g_force_halo < 0 ? -1 : (g_force_halo == 0 ? 0 : forced_halo_variant(hok)); }

static int launch_halo(ConvGemmArgs a, int v, float *slab, hipStream_t st) {
  halo_prepare(a, v);
  int splits = slab ? halo_splits(a, v) : 1;
  a.tilesPerSplit = (a.nkt + splits - 1) / splits;
  splits = (a.nkt + a.tilesPerSplit - 1) / a.tilesPerSplit;
  a.slab = splits > 1 ? slab : nullptr;
  if (a.slab) a.statPart = nullptr;
  {
    const double abytes = (double)a.xBytes + 4.0 * a.M * a.Rtrue + 4.0 * a.M * (double)a.NP * (a.resid ? 2 : 1);
    ProfScope ps(prof_key(kProfHalo, v), a.algoFlops > 0 ? a.algoFlops : 2.0 * a.M * (double)a.NP * a.Rtrue, st, abytes);
    const dim3 grid(a.nbm * a.nbn, splits), block(256);
    if (v == 0) hipLaunchKernelGGL((conv_halo_kernel<2, 2, 2, 2, 512>), grid, block, 0, st, a);
    else if (v == 1) hipLaunchKernelGGL((conv_halo_kernel<3, 1, 1, 4, 512>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((conv_halo_kernel<3, 1, 1, 4, 1024>), grid, block, 0, st, a);
  }
  XM_LAUNCH_CHECK();
  if (splits > 1) {
    launch_splitk_epilogue(a, splits, a.NP, a.vecStore && (a.NP & 3) == 0 && ((uintptr_t)a.slab & 15) == 0, st);
    XM_LAUNCH_CHECK();
  }
  return XM_OK;
}

// the stride-parity classes of a strided dgrad in one launch (no split-K), all through halo variant v
static int launch_halo_multi(const std::vector<ConvGemmArgs> &args, int v, hipStream_t st) {
  ConvGemmMulti m{};
  int maxTiles = 0;
  double flops = 0, abytes = args.empty() ? 0.0 : (double)args[0].xBytes;
  for (size_t i = 0; i < args.size(); ++i) {
    ConvGemmArgs a = args[i];
    halo_prepare(a, v);
    maxTiles = std::max(maxTiles, a.nbm * a.nbn);
    flops += a.algoFlops > 0 ? a.algoFlops : 2.0 * a.M * (double)a.NP * a.Rtrue;
    abytes += 4.0 * a.M * a.Rtrue + 4.0 * a.M * (double)a.NP * (a.resid ? 2 : 1);
    m.c[i] = a;
  }
  {
    ProfScope ps(prof_key(kProfHaloMulti, v), flops, st, abytes);
    const dim3 grid(maxTiles, 1, (unsigned)args.size()), block(256);
    if (v == 0) hipLaunchKernelGGL((conv_halo_multi_kernel<2, 2, 2, 2, 512>), grid, block, 0, st, m);
    else if (v == 1) hipLaunchKernelGGL((conv_halo_multi_kernel<3, 1, 1, 4, 512>), grid, block, 0, st, m);
    else hipLaunchKernelGGL((conv_halo_multi_kernel<3, 1, 1, 4, 1024>), grid, block, 0, st, m);
  }
  XM_LAUNCH_CHECK();
  return XM_OK;
}

// ---- measured tile selection ("find mode") ---------------------------------------------------
// The first time a (direction, geometry) is seen, every tile configuration is timed on the
// caller's stream (HIP events, 2 launches each, best of) and the winner is cached for the life of
// the process.  Happens during warm-up; results are identical for every configuration.
// XM_AUTOTUNE=0 falls back to the analytic model above.
static TuneTable g_tune;   // the process-wide table (keys, file format, load / save: conv_tune.h)

static std::string tune_default_path() {
  if (const char *e = getenv("XM_TUNE_FILE")) return e;
  Dl_info info;
  if (dladdr((const void *)&tune_default_path, &info) && info.dli_fname) {
    std::string p(info.dli_fname);
    size_t k = p.find_last_of('/');
    return (k == std::string::npos ? std::string(".") : p.substr(0, k)) + "/tune_gfx950.txt";
  }
  return "tune_gfx950.txt";
}
static void tune_load_once() {
  if (g_tune.loaded) return;
  g_tune.loaded = true;
  const char *e = getenv("XM_TUNE_FILE");
  if (e && !e[0]) return;  // XM_TUNE_FILE="" : no persistent table
  int n = g_tune.load(tune_default_path().c_str());
  if (getenv("XM_TUNE_VERBOSE")) fprintf(stderr, "[xm tune] %d entries from %s\n", n, tune_default_path().c_str());
}
static int autotune_enabled() {
  static int on = -1;
  if (on < 0) {
    const char *e = getenv("XM_AUTOTUNE");
    on = (e && e[0] == '0') ? 0 : 1;
  }
  return on;
}
// The gate in front of both measuring routines.  true: nothing is recorded under `key` and the candidates may be timed now.
// false: *pick is the answer -- the table's entry, or what the caller put there (find mode off, or `st` is being captured).
static bool tune_must_measure(const TuneKey &key, hipStream_t st, int *pick) {
  if (!autotune_enabled()) return false;
  tune_load_once();
  if (const int *hit = g_tune.find(key)) {
    *pick = *hit;
    return false;
  }
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return !(hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone);
}
// The event pair of a measurement.
struct TuneTimer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  bool ok;
  TuneTimer() {
    ok = hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
    // The candidates are timed on an otherwise idle device: whatever the other streams of the step had queued is drained first
    // (the host thread is in here, so nothing new arrives).  Timed next to a neighbour's kernels the choice depended on what
    // happened to be running -- the shipped table differed from one generation to the next.
    if (ok) (void)hipDeviceSynchronize();
  }
  ~TuneTimer() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
  // milliseconds of one launch() on `st`; negative: it failed, or could not be timed
  template <class L>
  float time_once(hipStream_t st, L &&launch) {
    float ms = 0.f;
    (void)hipEventRecord(e0, st);
    if (launch() != XM_OK) return -1.f;
    (void)hipEventRecord(e1, st);
    if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return -1.f;
    return ms;
  }
};

// XM_TUNE_REPS (default 2) consecutive launches per configuration, best of; one that fails disqualifies its configuration.
template <class F>
static int tune_cfg(const TuneKey &key, int fallback, hipStream_t st, F &&launch, int ncfg = kNumBaseCfg,
                    unsigned skip = 0 /* bit ci: configuration not eligible for this launch */) {
  if (g_force_cfg >= 0) return g_force_cfg < ncfg ? g_force_cfg : base_cfg(g_force_cfg);
  int bi = fallback;
  if (!tune_must_measure(key, st, &bi)) return bi;
  TuneTimer timer;
  if (!timer.ok) return fallback;
  static const bool verbose = getenv("XM_TUNE_VERBOSE") != nullptr;
  static const int reps = getenv("XM_TUNE_REPS") ? std::max(1, atoi(getenv("XM_TUNE_REPS"))) : 2;
  float best = 1e30f;
  for (int ci = 0; ci < ncfg; ++ci) {
    if (skip >> ci & 1u) continue;
    float tmin = 1e30f;
    for (int rep = 0; rep < reps; ++rep) {
      const float ms = timer.time_once(st, [&] { return launch(ci); });
      if (ms < 0.f) {
        tmin = 1e30f;
        break;
      }
      tmin = std::min(tmin, ms);
    }
    if (verbose) fprintf(stderr, " cfg%d %.3f", ci, tmin);
    if (tmin < best) {
      best = tmin;
      bi = ci;
    }
  }
  g_tune.record(key, bi);
  if (verbose)
    fprintf(stderr, "  -> [xm tune] kind %d M %d NP %d Rp %d (%d %d %d %d %d): cfg%d %.3f ms\n", key.kind, key.M,
            key.NP, key.Rp, key.mode, key.a, key.b, key.c, key.d, bi, best);
  return bi;
}

// Incumbent (0) against challengers (1 .. n - 1): all are timed ALTERNATELY, four rounds, best-of each (the first round
// is a warm-up), and the best challenger has to win by `margin` -- a choice within the noise of two timed launches
// flipped between processes, and an alternative that is only as fast in isolation loses when its blocks share the chip
// (larger LDS footprint).  `ok[i]` = false skips a challenger.
template <class F>
static int tune_challengers(const TuneKey &key, hipStream_t st, F &&launch, int n, const bool *ok, float margin) {
  int pick = 0;
  if (!tune_must_measure(key, st, &pick)) return (pick < n && (pick == 0 || ok[pick])) ? pick : 0;   // a stored arm has to be runnable still
  TuneTimer timer;
  if (!timer.ok) return 0;
  float tmin[8];
  for (int i = 0; i < 8; ++i) tmin[i] = 1e30f;
  for (int rep = 0; rep < 4; ++rep)
    for (int ci = 0; ci < n && ci < 8; ++ci) {
      if (ci > 0 && !ok[ci]) continue;
      const float ms = timer.time_once(st, [&] { return launch(ci); });
      if (rep > 0 && ms >= 0.f) tmin[ci] = std::min(tmin[ci], ms);
    }
  float best = (1.f - margin) * tmin[0];
  for (int ci = 1; ci < n && ci < 8; ++ci)
    if (tmin[ci] < best) best = tmin[ci], pick = ci;
  g_tune.record(key, pick);
  if (getenv("XM_TUNE_VERBOSE"))
    fprintf(stderr, "[xm tune] kind %d M %d NP %d Rp %d: incumbent %.3f ms, challengers %.3f %.3f %.3f -> %d\n", key.kind,
            key.M, key.NP, key.Rp, tmin[0], tmin[1], tmin[2], tmin[3], pick);
  return pick;
}
// The one selection routine behind every "incumbent against challengers" choice: arm 0 is the best implicit-GEMM
// configuration, arms 1 .. n - 1 the special-purpose kernels with ok[i].  Returns the arm a force hook names (`forced` >= 0),
// else the measured pick under `base` with its kind replaced (0 with find mode off).  The caller runs the pick.
template <class F>
static int select_arm(int kind, TuneKey base, hipStream_t st, int n, const bool *ok, float margin, int forced, F &&launch) {
  bool any = false;
  for (int i = 1; i < n; ++i) any = any || ok[i];
  if (!any) return 0;          // no challenger can run: nothing to choose, nothing to record
  if (forced >= 0) return forced;
  base.kind = kind;
  return tune_challengers(base, st, launch, n, ok, margin);
}
static const bool kOneChallenger[2] = {true, true};

template <int AV>
static void launch_wgrad_av(int ci, const WgradArgs &a, dim3 grid, hipStream_t st) {
  dim3 block(256);
  switch (ci) {
    case 0: hipLaunchKernelGGL((conv_wgrad_kernel<2, 2, 2, 2, AV>), grid, block, 0, st, a); break;
    case 1: hipLaunchKernelGGL((conv_wgrad_kernel<2, 2, 1, 4, AV>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((conv_wgrad_kernel<3, 1, 1, 4, AV>), grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL((conv_wgrad_kernel<1, 2, 2, 2, AV>), grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL((conv_wgrad_kernel<1, 1, 2, 2, AV>), grid, block, 0, st, a); break;
    case 5: hipLaunchKernelGGL((conv_wgrad_kernel<1, 1, 4, 1, AV>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((conv_wgrad_kernel<1, 1, 1, 4, AV>), grid, block, 0, st, a); break;
  }
}

// dY staging width: 4 / 2 consecutive pixels per load when groups cannot straddle two samples
// (Ho*Wo % AV == 0) and the rows are AV*4-byte aligned
static int wgrad_av(const WgradArgs &a) {
  const int hw = a.Ho * a.Wo;
  const uintptr_t p = (uintptr_t)a.dY;
  if (hw % 4 == 0 && (p & 15) == 0) return 4;
  if (hw % 2 == 0 && (p & 7) == 0) return 2;
  return 1;
}
static void launch_wgrad_cfg(int ci, const WgradArgs &a, dim3 grid, hipStream_t st) {
  switch (wgrad_av(a)) {
    case 4: launch_wgrad_av<4>(ci, a, grid, st); break;
    case 2: launch_wgrad_av<2>(ci, a, grid, st); break;
    default: launch_wgrad_av<1>(ci, a, grid, st); break;
  }
}

// ---- geometry shared by the three directions (struct Geo: conv_plan.h) ------------------------
static_assert(sizeof(Tap2) == sizeof(int2) && alignof(Tap2) <= alignof(int2), "Tap2 has the layout of int2: {x, y}");
static_assert(sizeof(Tap4) == sizeof(int4) && alignof(Tap4) <= alignof(int4), "Tap4 has the layout of int4: {x, y, z, w}");

int make_geo(Geo &g, int H, int W, int C, int N, int FH, int FW, int FC, int K, int sy,
             int sx, int pt, int pb, int pl, int pr, int dy, int dx) {
  if (H <= 0 || W <= 0 || C <= 0 || N <= 0 || FH <= 0 || FW <= 0 || FC <= 0 || K <= 0)
    return fail(XM_EINVAL, "vl_nnconv: empty tensor (X %dx%dx%dx%d, F %dx%dx%dx%d)", H, W, C, N, FH,
                FW, FC, K);
  if (sy < 1 || sx < 1 || dy < 1 || dx < 1 || pt < 0 || pb < 0 || pl < 0 || pr < 0)
    return fail(XM_EINVAL, "vl_nnconv: stride/dilate must be >= 1 and pad >= 0");
  if (C % FC) return fail(XM_EINVAL, "vl_nnconv: size(F,3)=%d does not divide size(X,3)=%d", FC, C);
  int G = C / FC;
  if (K % G) return fail(XM_EINVAL, "vl_nnconv: %d filters not divisible into %d groups", K, G);
  int Ho = out_size(H, pt, pb, FH, dy, sy), Wo = out_size(W, pl, pr, FW, dx, sx);
  if (Ho <= 0 || Wo <= 0)
    return fail(XM_EINVAL, "vl_nnconv: filter (%dx%d, dilate %dx%d) larger than padded input (%dx%d)",
                FH, FW, dy, dx, H + pt + pb, W + pl + pr);
  // gathers go through 32-bit-offset buffer descriptors: every tensor must stay below 4 GiB
  if ((long long)H * W * C * N >= (1LL << 30) || (long long)Ho * Wo * K * N >= (1LL << 30) ||
      (long long)FH * FW * FC * K >= (1LL << 30))
    return fail(XM_ETOOBIG, "vl_nnconv: tensor with >= 2^30 elements (4 GiB)");
  g = Geo{H, W, C, N, FH, FW, FC, K, G, K / G, Ho, Wo, FH * FW * FC, sy, sx, pt, pb, pl, pr, dy, dx};
  return XM_OK;
}

// the planning tables (conv_plan.h) on the device, cached by content
static const int2 *device_taps(const std::vector<Tap2> &t) {
  return (const int2 *)cached_device_table(t.data(), t.size() * sizeof(Tap2));
}
static const int4 *device_taps(const std::vector<Tap4> &t) {
  return (const int4 *)cached_device_table(t.data(), t.size() * sizeof(Tap4));
}

// ---- skinny fully-connected layers ------------------------------------------------------------
// vl_nnconv with a 1 x 1 filter over few output values: the SE gates (1 x 1 x C x N), the teacher's classifier
// (2048 -> 8), the student's fc8.  y[m, p] = act(b[m] + sum_k F[k + K m] X[p, k]).  An MFMA tile would be > 90 %
// padding and a single block would walk K alone (31 us for 2048 -> 8 at 32 samples).  Here one BLOCK owns one output
// row m and a chunk of <= 32 pixels: its 1-4 waves split K (VEC: 4 consecutive k per lane, 16-byte loads of the
// filter row and of every pixel's channel run -- needs H*W == 1; otherwise one k per lane), 32 accumulators per
// lane, a transposing butterfly (63 shuffles instead of 32 x 6) leaves the sum of pixel j in lanes 2j, 2j + 1,
// and the waves' partials are added in wave order through LDS.  ACT: 0 none, 1 relu, 2 sigmoid.
template <int ACT, bool VEC>
__global__ void __launch_bounds__(256)
fc_skinny_kernel(const float *__restrict__ x, const float *__restrict__ f, const float *__restrict__ b,
                 float *__restrict__ y, int K, int M, int HW, int NP, int chunks, FastDiv divChunks, FastDiv divHW,
                 const float *__restrict__ scale, const float *__restrict__ shift) {
  __shared__ float red[4][32];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  const int m = (int)xm_div(blockIdx.x, divChunks);
  const int p0 = ((int)blockIdx.x - m * chunks) * 32;
  int xb[32];
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const int p = min(p0 + j, NP - 1);
    const int n = (int)xm_div((uint32_t)p, divHW);
    xb[j] = (p - n * HW) + HW * K * n;
  }
  float acc[32];
#pragma unroll
  for (int j = 0; j < 32; ++j) acc[j] = 0.f;
  const float *fr = f + (size_t)K * m;
  if (VEC) {
    for (int k = (wv * 64 + lane) * 4; k < K; k += nw * 256) {
      const float4 w = *reinterpret_cast<const float4 *>(fr + k);
      // all loads of a half first, then the arithmetic: left alone, the scheduler pairs every load with its use
      // (two loads in flight, 32 serial round trips -- 20 us per call)
#pragma unroll
      for (int jh = 0; jh < 32; jh += 16) {
        f32x4 v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = *reinterpret_cast<const f32x4 *>(x + xb[jh + j] + k);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 16; ++j) asm volatile("" : "+v"(v[j]));  // pins the uses behind all 16 loads
#pragma unroll
        for (int j = 0; j < 16; ++j)
          acc[jh + j] = fmaf(w.w, v[j].w, fmaf(w.z, v[j].z, fmaf(w.y, v[j].y, fmaf(w.x, v[j].x, acc[jh + j]))));
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  } else {
    for (int k = wv * 64 + lane; k < K; k += nw * 64) {
      const float w = fr[k];
      const float *xk = x + (size_t)HW * k;
      float v[32];
#pragma unroll
      for (int j = 0; j < 32; ++j) v[j] = xk[xb[j]];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 32; ++j) asm volatile("" : "+v"(v[j]));
#pragma unroll
      for (int j = 0; j < 32; ++j) acc[j] = fmaf(w, v[j], acc[j]);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // stage (o, h): lanes with bit o set keep the upper h values, the others the lower h, and add the partner's
#pragma unroll
  for (int s = 0; s < 5; ++s) {
    const int o = 32 >> s, h = 16 >> s;
    const bool up = (lane & o) != 0;
#pragma unroll
    for (int i = 0; i < h; ++i) {
      // (selecting which ELEMENT to send would halve the shuffles, but the compiler turns `up ? acc[i + h] : acc[i]`
      // into a runtime-indexed register array: 5000 compare / select instructions)
      const float lo = acc[i] + __shfl_xor(acc[i], o, 64);
      const float hi = acc[i + h] + __shfl_xor(acc[i + h], o, 64);
      acc[i] = up ? hi : lo;
    }
  }
  float v = acc[0] + __shfl_xor(acc[0], 1, 64);
  if ((lane & 1) == 0) red[wv][lane >> 1] = v;
  __syncthreads();
  const int p = p0 + (int)threadIdx.x;
  if (threadIdx.x < 32 && p < NP) {
    v = red[0][threadIdx.x];
    for (int w = 1; w < nw; ++w) v += red[w][threadIdx.x];
    if (b) v += b[m];
    if (scale) v = v * scale[m] + shift[m];     // folded test-mode bnorm: (conv + b) .* scale + shift
    if (ACT == 1) v = fmaxf(v, 0.f);
    if (ACT == 2) v = 1.f / (1.f + expf(-v));
    const int n = (int)xm_div((uint32_t)p, divHW);
    y[(p - n * HW) + (size_t)HW * (m + (size_t)M * n)] = v;
  }
}
// The same for FOUR output rows and a chunk of 16 pixels per block (H*W == 1, 16-byte loads): a block of the one-row
// kernel reads its 32 pixels' whole channel runs, i.e. the input is read M times from the L2s (512 MB for the student's
// fc7 at 32 clips: 22 us); four rows per block share every load.  64 accumulators per lane (row r, pixel j -> 16 r + j),
// the transposing butterfly over all six lane bits leaves value i in lane i, the waves' partials meet in LDS.
template <int ACT>
__global__ void __launch_bounds__(256)
fc_skinny4_kernel(const float *__restrict__ x, const float *__restrict__ f, const float *__restrict__ b,
                  float *__restrict__ y, int K, int M, int NP, int chunks, FastDiv divChunks,
                  const float *__restrict__ scale, const float *__restrict__ shift) {
  __shared__ float red[4][64];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  const int mg = (int)xm_div(blockIdx.x, divChunks);
  const int p0 = ((int)blockIdx.x - mg * chunks) * 16, m0 = 4 * mg;
  int xb[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) xb[j] = K * min(p0 + j, NP - 1);
  float acc[64];
#pragma unroll
  for (int i = 0; i < 64; ++i) acc[i] = 0.f;
  const float *fr = f + (size_t)K * m0;
  for (int k = (wv * 64 + lane) * 4; k < K; k += nw * 256) {
    f32x4 w[4], v[16];
#pragma unroll
    for (int r = 0; r < 4; ++r) w[r] = *reinterpret_cast<const f32x4 *>(fr + (size_t)K * r + k);
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = *reinterpret_cast<const f32x4 *>(x + xb[j] + k);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < 16; ++j) asm volatile("" : "+v"(v[j]));   // pins the uses behind all the loads (see fc_skinny_kernel)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int j = 0; j < 16; ++j)
        acc[16 * r + j] = fmaf(w[r].w, v[j].w, fmaf(w[r].z, v[j].z, fmaf(w[r].y, v[j].y, fmaf(w[r].x, v[j].x, acc[16 * r + j]))));
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    const int o = 32 >> s, h = 32 >> s;
    const bool up = (lane & o) != 0;
#pragma unroll
    for (int i = 0; i < h; ++i) {
      const float lo = acc[i] + __shfl_xor(acc[i], o, 64);
      const float hi = acc[i + h] + __shfl_xor(acc[i + h], o, 64);
      acc[i] = up ? hi : lo;
    }
  }
  red[wv][lane] = acc[0];
  __syncthreads();
  if (threadIdx.x < 64) {
    float v = red[0][threadIdx.x];
    for (int w = 1; w < nw; ++w) v += red[w][threadIdx.x];
    const int m = m0 + (int)(threadIdx.x >> 4), p = p0 + (int)(threadIdx.x & 15);
    if (b) v += b[m];
    if (scale) v = v * scale[m] + shift[m];
    if (ACT == 1) v = fmaxf(v, 0.f);
    if (ACT == 2) v = 1.f / (1.f + expf(-v));
    if (p < NP) y[m + (size_t)M * p] = v;
  }
}
static bool fc_skinny_ok(const Geo &g, bool dgrad = false) {
  const bool off = !path_on(kPathSkinny);
  if (off || g.FH != 1 || g.FW != 1 || g.sy != 1 || g.sx != 1 || g.dy != 1 || g.dx != 1 || g.G != 1) return false;
  if (g.pt | g.pb | g.pl | g.pr) return false;
  const long long NP = (long long)g.Ho * g.Wo * g.N;
  // A wide FC layer over many samples is a GEMM again (the student's fc7, 4096 -> 1024: forward 19.7 / 22.5 / 41.5 / 60.9 us
  // here against 38 / 40 / 42 / 46.6 us on the MFMA path at 32 / 64 / 128 / 256 samples; as dX = W' dY 28.6 / 39.6 / 67.7 / 111 us
  // against 30 / 32.5 / 40.6 / 59 us): every 16-sample chunk re-reads the 16 MB of weights.  The SE layers (<= 0.26 M weights)
  // stay here at every batch.
  if ((long long)g.C * g.K >= (1ll << 20) && NP > (dgrad ? 32 : 128)) return false;
  const bool rows4 = g.H * g.W == 1 && (g.C & 3) == 0 && (g.K & 3) == 0;   // fc_skinny4_kernel's geometry
  if (!(g.K <= 16 || NP <= (rows4 ? 512 : 128))) return false;
  return (long long)g.K * ((NP + 31) / 32) <= 65535 && (long long)g.H * g.W * g.C * g.N < (1ll << 31);
}
static int fc_skinny_forward(const float *x, const float *f, const float *b, float *y, const Geo &g, int act,
                             hipStream_t st, const float *scale = nullptr, const float *shift = nullptr) {
  const int HW = g.H * g.W, NP = HW * g.N, chunks = (NP + 31) / 32;
  const bool vec = HW == 1 && (g.C & 3) == 0 && (((uintptr_t)x | (uintptr_t)f) & 15) == 0;
  const int units = vec ? g.C / 4 : g.C;   // k positions handed out per lane step
  const int nw = std::max(1, std::min(4, (units + 63) / 64));
  const bool no4 = !path_on(kPathSkinny4);
  if (vec && (g.K & 3) == 0 && g.K >= 16 && !no4) {
    const int ch = (NP + 15) / 16;
    dim3 grid4((unsigned)(g.K / 4 * ch)), block4(64 * nw);
    FastDiv dc4 = make_fastdiv((uint32_t)ch);
#define XM_FC4_LAUNCH(A) \
  hipLaunchKernelGGL((fc_skinny4_kernel<A>), grid4, block4, 0, st, x, f, b, y, g.C, g.K, NP, ch, dc4, scale, shift)
    if (act == 2) XM_FC4_LAUNCH(2);
    else if (act == 1) XM_FC4_LAUNCH(1);
    else XM_FC4_LAUNCH(0);
#undef XM_FC4_LAUNCH
    XM_LAUNCH_CHECK();
    return XM_OK;
  }
  dim3 grid(g.K * chunks), block(64 * nw);
  FastDiv dc = make_fastdiv((uint32_t)chunks), dh = make_fastdiv((uint32_t)HW);
#define XM_FC_LAUNCH(A, V) \
  hipLaunchKernelGGL((fc_skinny_kernel<A, V>), grid, block, 0, st, x, f, b, y, g.C, g.K, HW, NP, chunks, dc, dh, scale, shift)
  if (vec) {
    if (act == 2) XM_FC_LAUNCH(2, true);
    else if (act == 1) XM_FC_LAUNCH(1, true);
    else XM_FC_LAUNCH(0, true);
  } else {
    if (act == 2) XM_FC_LAUNCH(2, false);
    else if (act == 1) XM_FC_LAUNCH(1, false);
    else XM_FC_LAUNCH(0, false);
  }
#undef XM_FC_LAUNCH
  XM_LAUNCH_CHECK();
  return XM_OK;
}

// ---- single-channel stem (conv_stem_kernel) ----------------------------------------------------------------------
// Forward convolutions over ONE input channel with <= 8 x 7 taps, stride 1 / 2 along H, <= 96 filters, source columns of
// <= 512 rows (the student's conv1 over 512-bin spectrograms).  `f` is the caller's filter bank, unpadded.
static bool forced_tiling() { return g_force_cfg >= 0 || g_force_splits > 0; }   // a test asked for one implicit-GEMM launch
static bool fills_chip(const Geo &g) { return (long long)g.Ho * g.Wo * g.N >= 128 * 512; }   // >= one round of the chip
static unsigned epilogue_flags(const ConvGemmArgs &a, bool stats) {
  return (a.vecStore ? kEpiVecStore : 0u) | (a.scale ? kEpiScale : 0u) | (a.resid ? kEpiResid : 0u) |
         (a.gate ? kEpiGate : 0u) | (a.relu ? kEpiRelu : 0u) | (stats ? kEpiStats : 0u);
}
static bool stem_ok(const ConvGemmArgs &a, const Geo &g, const float *x, bool stats) {
  if (!path_on(kPathStem) || forced_tiling()) return false;
  if (!stem_fwd_can(g, (uintptr_t)x, epilogue_flags(a, stats))) return false;
  return g_force_stem == 1 || fills_chip(g);
}

static int stem_grid(int NP) { return std::min(256 * XM_STEM_OCC, ((NP + 127) / 128 + 7) / 8 * 8); }

static int launch_stem(ConvGemmArgs a, const float *f, int R, hipStream_t st) {
  a.A = f, a.lda = R, a.nbm = 1, a.nbn = (a.NP + 127) / 128, a.slab = nullptr;
  a.hyS = 1, a.hyFull = 0, a.hyTps = 0, a.hyP0 = 0, a.piReal = 0;
  a.dbgCycles = g_dbg_cycles;
  const double abytes = (double)a.xBytes + 4.0 * a.M * a.Rtrue + 4.0 * a.M * (double)a.NP;
  ProfScope ps(prof_key(kProfStem), 2.0 * a.M * (double)a.NP * a.Rtrue, st, abytes);
  const int grid = stem_grid(a.NP);
  if (a.gsy == 2) hipLaunchKernelGGL(conv_stem_kernel<2>, dim3(grid), dim3(256), 0, st, a, a.nbn);
  else hipLaunchKernelGGL(conv_stem_kernel<1>, dim3(grid), dim3(256), 0, st, a, a.nbn);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

// ---- three-channel stem (conv_stem3_kernel): 7 x 7 / stride 2 over RGB images, 64 filters -- the teachers' conv1 --------------
static int g_force_stem3 = -1;   // test hook (xm_debug_force_conv_stem3)
static bool stem3_ok(const ConvGemmArgs &a, const Geo &g, const float *x, bool stats) {
  if (!path_on(kPathStem3) || forced_tiling()) return false;
  if (!stem3_can(g, (uintptr_t)x, epilogue_flags(a, stats))) return false;
  return g_force_stem3 == 1 || fills_chip(g);
}
static int launch_stem3(ConvGemmArgs a, const float *f, int R, hipStream_t st) {
  a.A = f, a.lda = R, a.nbm = 1, a.nbn = a.NP / 128, a.slab = nullptr;
  const double abytes = (double)a.xBytes + 4.0 * a.M * a.Rtrue + 4.0 * a.M * (double)a.NP;
  // 256-pixel block tiles (four accumulator chains per wave) where they divide a sample and span <= 4 output columns
  static const bool wide_on = env_int("XM_STEM3_WIDE", 1) != 0;
  const int pij = (int)a.divPIJ.d, pi = (int)a.divPI.d;
  const bool wide = wide_on && pij % 256 == 0 && pi >= 86;
  if (wide) a.nbn = a.NP / 256;
  ProfScope ps(prof_key(kProfStem3, wide ? 1 : 0), 2.0 * a.M * (double)a.NP * a.Rtrue, st, abytes);
  const int grid = std::min(512, (a.nbn + 7) / 8 * 8);
  if (wide) hipLaunchKernelGGL(conv_stem3_kernel<2>, dim3(grid), dim3(256), 0, st, a, a.nbn);
  else hipLaunchKernelGGL(conv_stem3_kernel<1>, dim3(grid), dim3(256), 0, st, a, a.nbn);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

// scratch for the split-K slab of whichever of the first `ncfg` tile configurations (or halo variant: nU x nV taps over
// Rtrue reduction steps) ends up running an M x NP problem
static size_t slab_floats(int M, int NP, int Rp, int ncfg, int nU, int nV, int Rtrue) {
  ConvGemmArgs proto{};
  proto.M = M, proto.NP = NP, proto.Rp = Rp;
  size_t need = 0;
  for (int c = 0; c < ncfg; ++c) {
    int sp;
    need = std::max(need, gemm_slab_floats(proto, c, &sp));
  }
  if (nU <= 3 && nV <= 3 && nU * nV >= 4 && Rtrue % (kHaloCB * nU * nV) == 0) {   // halo-patch kernel splits
    proto.Rtrue = Rtrue, proto.nU = nU, proto.nV = nV;
    need = std::max(need, halo_slab_floats(proto));
  }
  return need;
}

// what every filter group of a forward call shares
struct FwdOperands {
  const float *x, *A, *b, *scale, *shift, *resid, *gate;
  float *y;
  const int2 *taps;
  int lda, Rp, relu;
  bool bigTaps, dma_ok;
  // the residual's own geometry: extent rH x rW (x K x N), sampled at (oy * rsy, ox * rsx).  rH == Ho, rW == Wo, unit strides
  // is the plain residual at output extent.
  int rH = 0, rW = 0, rsy = 1, rsx = 1;
  bool resid_strided(const Geo &g) const { return resid && (rH != g.Ho || rW != g.Wo || rsy != 1 || rsx != 1); }
};

// the implicit-GEMM problem of filter group `grp`
static ConvGemmArgs forward_args(const Geo &g, int grp, const FwdOperands &o) {
  ConvGemmArgs a{};
  const size_t xoff = (size_t)grp * g.FC * g.H * g.W, yoff = (size_t)grp * g.Kg * g.Ho * g.Wo;
  a.A = o.A + (size_t)grp * g.Kg * o.lda, a.lda = o.lda, a.aBytes = (unsigned)((size_t)g.Kg * o.lda * 4);
  a.X = o.x + xoff, a.xBytes = (unsigned)((x_elements(g) - xoff) * 4), a.xSampleStride = g.H * g.W * g.C;
  a.Y = o.y + yoff, a.taps = o.taps, a.tapStride = (unsigned)((size_t)g.H * g.W * 4);
  a.bias = o.b ? o.b + grp * g.Kg : nullptr;
  a.scale = o.scale ? o.scale + grp * g.Kg : nullptr, a.shift = o.shift ? o.shift + grp * g.Kg : nullptr;
  a.resid = o.resid ? o.resid + yoff : nullptr, a.relu = o.relu;
  if (o.resid_strided(g)) {
    // the residual's own group offset and strides; the epilogues fetch it pixel by pixel (ConvGemmArgs::rsOn)
    a.resid = o.resid + (size_t)grp * g.Kg * o.rH * o.rW;
    a.rsOn = 1, a.rsy = o.rsy, a.rsx = o.rsx, a.rH = o.rH;
    a.rChanStride = o.rH * o.rW, a.rSampleStride = o.rH * o.rW * g.K;
  }
  a.gate = o.gate ? o.gate + (size_t)grp * g.Kg : nullptr, a.gateStride = g.K;
  a.M = g.Kg, a.Rp = o.Rp, a.Rtrue = g.R;
  a.PI = g.Ho, a.PJ = g.Wo, a.NP = g.Ho * g.Wo * g.N;
  a.divPIJ = make_fastdiv((uint32_t)(g.Ho * g.Wo)), a.divPI = make_fastdiv((uint32_t)g.Ho);
  a.gsy = g.sy, a.gsx = g.sx, a.gh0 = -g.pt, a.gw0 = -g.pl, a.LimH = g.H, a.LimW = g.W;
  a.nU = o.bigTaps ? 1 : g.FH, a.nV = o.bigTaps ? 1 : g.FW;   // mask construction only looks at tap (0,0) then (always valid)
  a.du0 = 0, a.dus = g.dy, a.dv0 = 0, a.dvs = g.dx;
  a.osy = 1, a.osx = 1, a.oh0 = 0, a.ow0 = 0, a.OH = g.Ho;
  a.oChanStride = g.Ho * g.Wo, a.oSampleStride = g.Ho * g.Wo * g.K, a.divMU = make_fastdiv(1), a.oUStride = 0;
  // 4 consecutive output pixels are contiguous (same sample) and every tile starts on a multiple
  // of 32 pixels; 16-byte alignment of (y, residual) rows needs Ho*Wo % 4 == 0
  // (a strided residual is read with 4-byte loads: its alignment does not matter)
  a.vecStore = ((g.Ho * g.Wo) % 4 == 0 && (((uintptr_t)a.Y | (a.rsOn ? 0 : (uintptr_t)a.resid)) & 15) == 0) ? 1 : 0;
  // the LDS-DMA kernel only carries the 16-byte-store epilogue, and no strided residual
  a.dmaOk = (o.dma_ok && a.vecStore && !a.rsOn) ? 1 : 0;
  return a;
}

// Batch statistics riding in the epilogue of the launch: `ok` = this group's launch may carry them (16-byte-store
// epilogue, no relu / residual), `part` = room for the partial sums, `ncg` = partial rows per channel the launch that
// ran LAST left behind (0: none -- split-K, or a kernel without the epilogue).
struct FwdStats {
  bool ok;
  float *part;
  int ncg;
};
static ConvGemmArgs stats_args(const ConvGemmArgs &a, FwdStats &s, int ncg) {
  ConvGemmArgs aa = a;
  s.ncg = ncg;
  if (ncg > 0) aa.statPart = s.part, aa.statNcg = ncg;
  return aa;
}
// [mean, sqrt(var + eps)] from the partial sums (fp64 across the partial rows, fixed order)
static int forward_stats_reduce(const FwdStats &s, double *part2, float *moments_out, int K, int NP, float eps, hipStream_t st) {
  const int S = std::max(1, std::min(64, s.ncg / 768));   // one launch up to ~1500 partial rows per channel
  g_last_stats_splits = S;
  hipLaunchKernelGGL(conv_stats_reduce_kernel, dim3((K + 7) / 8, S), dim3(256), 0, st, s.part, moments_out, part2, K, s.ncg, S,
                     (double)NP, eps);
  XM_LAUNCH_CHECK();
  if (S > 1) {
    hipLaunchKernelGGL(conv_stats_finalize2_kernel, dim3((K + 255) / 256), dim3(256), 0, st, part2, moments_out, K, S,
                       (double)NP, eps);
    XM_LAUNCH_CHECK();
  }
  return XM_OK;
}

// Selection and launch of one group's forward problem: the best implicit-GEMM configuration, then ONE family of
// special-purpose kernels against it (measured once per shape, alternating launches, the challenger must win by a margin).
static int forward_run(const Geo &g, const ConvGemmArgs &a, const float *x, const float *f, int mode, float *slab,
                       FwdStats &s, hipStream_t st) {
  auto gemm = [&](int ci) {
    int sp;
    ci = a.dmaOk ? ci : base_cfg(ci);
    gemm_slab_floats(a, ci, &sp);
    const bool carry = s.ok && sp == 1 && g_force_splits <= 1;
    ConvGemmArgs aa = stats_args(a, s, carry ? (a.NP + kCfgs[ci].bn() - 1) / kCfgs[ci].bn() : 0);
    const int rc_ = launch_gemm(aa, mode, ci, sp, slab, st);
    if (aa.statPart) s.ncg = aa.statNcg;     // (hybrid schedule: full pixel tiles + the combine kernel's chunks)
    return rc_;
  };
  // the launch with fused batch statistics is its own entry: it excludes the LDS-DMA configurations and carries a
  // longer epilogue, so whichever variant reached a shape first must not fix the choice for the other
  const TuneKey key = tune_key_forward(0, g, a.M, a.NP, a.Rp, mode + (s.ok ? 4 : 0));
  const int ci = tune_cfg(key, pick_cfg(a.M, a.NP, a.Rp / kBK), st, gemm, a.dmaOk ? kNumCfg : kNumBaseCfg, w8_skip(a.M, a.NP));
  // a strided residual is known to the implicit-GEMM epilogue and the split-K combine only: no stem, no halo arm
  if (!a.rsOn && stem_ok(a, g, x, s.ok)) {     // the single-channel stem kernel: one partial row per (persistent) block
    auto arm = [&](int h) { return h ? launch_stem(stats_args(a, s, s.ok ? stem_grid(a.NP) : 0), f, g.R, st) : gemm(ci); };
    return arm(select_arm(7, key, st, 2, kOneChallenger, kHaloMargin, g_force_stem, arm));
  }
  if (!a.rsOn && stem3_ok(a, g, x, s.ok)) {    // the three-channel stem kernel
    auto arm = [&](int h) { return h ? launch_stem3(a, f, g.R, st) : gemm(ci); };
    return arm(select_arm(12, key, st, 2, kOneChallenger, kHaloMargin, g_force_stem3, arm));
  }
  // <= 3 x 3 taps / unit stride: the halo-patch kernel variants
  ConvGemmArgs ah = a;
  const int hneed = (forced_tiling() || a.rsOn) ? 0 : halo_setup(ah, g.N);
  const bool hok[4] = {true, halo_var_ok(ah, hneed, 0), halo_var_ok(ah, hneed, 1), halo_var_ok(ah, hneed, 2)};
  auto arm = [&](int h) {
    if (!h) return gemm(ci);
    const bool carry = s.ok && halo_splits(ah, h - 1) == 1;
    return launch_halo(stats_args(ah, s, carry ? (a.NP + 127) / 128 : 0), h - 1, slab, st);
  };
  return arm(select_arm(4, key, st, 4, hok, kHaloMargin, halo_forced(hok), arm));
}

static bool fwd_dma_ok(const Geo &g, const float *x, const float *f, bool need_pad, int mode) {
  return !need_pad && mode == 0 && g.FH == 1 && g.FW == 1 && g.sy == 1 && g.sx == 1 && g.dy == 1 &&
         g.dx == 1 && (g.H * g.W) % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)f & 15) == 0 &&
         g.R % kBK == 0 && path_on(kPathDma);
}

// moments_out != NULL: also the batch moments [mean, sqrt(var + eps)] of Y (the statistics half of the train-mode
// vl_nnbnorm that follows the convolution), from per-wave partial sums of the GEMM epilogue when the launch allows it
// (16-byte-store epilogue, no split-K, no filter groups), else by a pass over Y.
static int conv_forward(const float *x, const float *f, const float *b, float *y, const Geo &g,
                        const float *scale, const float *shift, const float *resid, int relu,
                        hipStream_t st, float *moments_out = nullptr, float eps = 0.f, const float *gate = nullptr,
                        int res_H = 0, int res_W = 0, int res_sy = 1, int res_sx = 1) {
  // The (u,v) validity mask has 63 bits.  Without spatial padding every tap is inside the image, so
  // larger filters (the 1 x 401 STFT bank of batch.runSpec) simply do not use it.
  const bool padded = (g.pt | g.pb | g.pl | g.pr) != 0;
  const bool bigTaps = g.FH * g.FW > 63;
  if (bigTaps && padded)
    return fail(XM_ENOTSUP, "vl_nnconv: padded filters with more than 63 spatial taps (%dx%d) are not built",
                g.FH, g.FW);
  const int Rp = (g.R + kBK - 1) / kBK * kBK;
  const bool need_pad = (g.R % kBK) != 0 || ((uintptr_t)f & 15);
  const int mode = (padded || Rp != g.R) ? 1 : 0;
  const int NP = g.Ho * g.Wo * g.N;
  const size_t slabf = slab_floats(g.Kg, NP, Rp, kNumCfg, g.FH, g.FW, g.R);
  // LDS-DMA eligibility: a plain GEMM in memory (1x1, unit stride, no padding), pixel quads inside one sample,
  // 16-byte aligned operands
  const bool dma_ok = fwd_dma_ok(g, x, f, need_pad, mode);
  const bool want_stats = moments_out != nullptr && g.G == 1 && path_on(kPathFusedStats);
  // partial sums: one {sum, sum sq} pair per row and per pixel tile (>= 32 pixels), + 64 fp64 slabs for the reduction
  // (the persistent stem kernel leaves one row per block: stem_grid(NP) can exceed NP / 32 on small problems)
  const size_t statf = want_stats ? (size_t)2 * g.K * std::max((NP + 31) / 32, stem_grid(NP)) : 0;
  const size_t stat2 = want_stats ? (size_t)2 * g.K * 64 : 0;
  WsCarver ws;
  int rc = ws.init(WsCarver::need(need_pad ? (size_t)g.K * Rp : 0, 4) + WsCarver::need(slabf, 4) +
                       WsCarver::need(statf, 4) + WsCarver::need(stat2, 8), st);
  if (rc) return rc;
  FwdOperands o{x, f, b, scale, shift, resid, gate, y, device_taps(fwd_tap_table(g, Rp, bigTaps)), g.R, Rp, relu, bigTaps, dma_ok};
  if (!o.taps) return fail(XM_ENOMEM, "vl_nnconv: tap table allocation failed");
  if (resid) o.rH = res_H > 0 ? res_H : g.Ho, o.rW = res_W > 0 ? res_W : g.Wo, o.rsy = res_sy, o.rsx = res_sx;
  if (need_pad) {
    float *Ap = ws.take<float>((size_t)g.K * Rp);
    size_t n = (size_t)g.K * Rp;
    hipLaunchKernelGGL(pad_filter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, f, Ap,
                       g.K, g.R, Rp);
    XM_LAUNCH_CHECK();
    o.A = Ap;
    o.lda = Rp;
  }
  float *slab = slabf ? ws.take<float>(slabf) : nullptr;
  float *statp = statf ? ws.take<float>(statf) : nullptr;
  double *statp2 = stat2 ? ws.take<double>(stat2) : nullptr;
  bool stats_done = false;
  if (moments_out) g_last_stats_splits = 0;   // stays 0 when the moments come from the pass over Y below
  for (int grp = 0; grp < g.G; ++grp) {
    ConvGemmArgs a = forward_args(g, grp, o);
    FwdStats s{want_stats && a.vecStore && !relu && !resid, statp, 0};
    if (s.ok) a.dmaOk = 0;                  // the partial sums ride in the register-staged kernel's epilogue
    rc = forward_run(g, a, x, f, mode, slab, s, st);
    if (rc) return rc;
    if (s.ncg > 0) {
      rc = forward_stats_reduce(s, statp2, moments_out, g.K, NP, eps, st);
      if (rc) return rc;
      stats_done = true;
    }
  }
  if (moments_out && !stats_done) return bn_batch_moments(y, g.Ho, g.Wo, g.K, g.N, eps, moments_out, st);
  return XM_OK;
}

// ---- forward on an output lattice (xm_nnconv_forward_lattice) -------------------------------------------------------------
// The layer computed only at the output pixels (ly i, lx j) and stored at those positions of the full-extent Y: the same
// implicit GEMM over N * PI * PJ lattice pixels, the gather walking X with step (ly sy, lx sx), the scalar-store epilogue
// with the output strides (ly, lx).  Every lattice pixel has to get the BITS the full-extent launch gives it, and the bits
// follow the structure of the reduction: the launch therefore takes the tile configuration, the split-K
// cut points and the hybrid cut of the FULL-EXTENT layer, looked up under the full-extent key -- never its own.
struct FullExtentPlan {
  int ci;      // register-staged configuration with the chain structure of the full-extent launch
  int tps;     // reduction stages per split-K slab (nkt: unsplit)
  int hyS, hyTps, hyP0;   // hybrid remainder: the full-extent pixels from hyP0 on are hyS-way sums of hyTps stages
};
// 1 while the most recent xm_nnconv_forward_lattice call computed the lattice only, 0 when it ran the layer at full extent
// (xm_debug_get("conv_last_lattice"): tests)
static int g_last_lattice = 0;

// What forward_run does with the full-extent problem `a` of a group, WITHOUT launching.  false: not known without a
// measurement (find mode on, shape not in the table), or not an implicit-GEMM launch (a stem or halo-patch kernel: another
// summation order) -- the caller then runs the layer at full extent, which also records the measurement.
static bool full_extent_plan(const Geo &g, const ConvGemmArgs &a, const float *x, int mode, bool have_slab, hipStream_t st,
                             FullExtentPlan &p) {
  if (stem_ok(a, g, x, false) || stem3_ok(a, g, x, false)) return false;
  const TuneKey key = tune_key_forward(0, g, a.M, a.NP, a.Rp, mode);
  int ci = pick_cfg(a.M, a.NP, a.Rp / kBK);
  const int ncfg = a.dmaOk ? kNumCfg : kNumBaseCfg;
  if (g_force_cfg >= 0) ci = g_force_cfg < ncfg ? g_force_cfg : base_cfg(g_force_cfg);
  else if (tune_must_measure(key, st, &ci)) return false;
  ConvGemmArgs ah = a;
  const int hneed = forced_tiling() ? 0 : halo_setup(ah, g.N);
  const bool hok[4] = {true, halo_var_ok(ah, hneed, 0), halo_var_ok(ah, hneed, 1), halo_var_ok(ah, hneed, 2)};
  if (hok[1] || hok[2] || hok[3]) {
    int arm = halo_forced(hok);
    if (arm < 0) {
      TuneKey k4 = key;
      k4.kind = 4;
      arm = 0;
      if (tune_must_measure(k4, st, &arm)) return false;
      if (arm < 0 || arm >= 4 || !hok[arm]) arm = 0;
    }
    if (arm != 0) return false;
  }
  // forward_run's gemm(ci), then launch_gemm
  ci = a.dmaOk ? ci : base_cfg(ci);
  int sp;
  gemm_slab_floats(a, ci, &sp);
  if (ci == kCfgW8 && !path_on(kPathW8)) ci = 0;
  const Cfg &c = kCfgs[ci];
  ConvGemmArgs t = a;
  t.nbm = (a.M + c.bm() - 1) / c.bm(), t.nbn = (a.NP + c.bn() - 1) / c.bn(), t.nkt = a.Rp / kBK;
  t.statPart = nullptr;
  p.tps = (t.nkt + sp - 1) / sp;
  p.hyS = 1, p.hyTps = 0, p.hyP0 = 0;
  if (p.tps >= t.nkt && have_slab) {
    int full;
    const int hyS = hybrid_plan(t, ci, &full);
    if (hyS > 1) {
      p.hyTps = (t.nkt + hyS - 1) / hyS;
      p.hyS = (t.nkt + p.hyTps - 1) / p.hyTps;
      p.hyP0 = full / t.nbm * c.bn();
    }
  }
  // Every LDS-DMA kernel sums each output in ONE accumulator chain, in k order -- also 11, whose register-staged base
  // <1,1,2,2> has the two chains of the 1 x 1 wave tiles: that one maps to the one-chain <1,2,2,2>, the others to their bases
  p.ci = !is_dma_cfg(ci) ? ci : (kCfgs[ci].tm * kCfgs[ci].tn == 1 ? 3 : base_cfg(ci));
  return true;
}

// One implicit-GEMM launch of lattice problem `a` with a GIVEN split of the reduction (tps stages per slab); the slabs are
// combined over the pixels [p0, NP) only (p0 > 0: the launch began at a sample boundary below the hybrid cut).
static int launch_gemm_lattice(ConvGemmArgs a, int mode, int ci, int tps, float *slab, int p0, hipStream_t st) {
  const Cfg &c = kCfgs[ci];
  a.nbm = (a.M + c.bm() - 1) / c.bm();
  a.nbn = (a.NP + c.bn() - 1) / c.bn();
  a.nkt = a.Rp / kBK;
  a.tilesPerSplit = std::min(tps, a.nkt);
  const int splits = (a.nkt + a.tilesPerSplit - 1) / a.tilesPerSplit;
  a.NPs = (a.NP + 3) & ~3;
  a.slab = splits > 1 ? slab : nullptr;
  a.dbgCycles = g_dbg_cycles;
  a.hyS = 1, a.hyFull = 0, a.hyTps = 0, a.hyP0 = 0;
  if (splits > 1 && !slab) return fail(XM_EINVAL, "vl_nnconv(lattice): split launch without a slab");
  {
    const double abytes = (double)a.xBytes + 4.0 * a.M * a.Rtrue + 4.0 * a.M * (double)a.NP;
    ProfScope ps(prof_key(kProfGemm, ci * 2 + mode), 2.0 * a.M * (double)a.NP * a.Rtrue, st, abytes);
    const dim3 grid(a.nbm * a.nbn, splits);
    if (mode) launch_gemm_cfg<1>(ci, a, grid, st);
    else launch_gemm_cfg<0>(ci, a, grid, st);
  }
  XM_LAUNCH_CHECK();
  g_last_combine = 0;
  if (splits > 1) {
    a.slab += p0, a.hyP0 = p0;       // the combine kernel reads the slabs relative to hyP0
    launch_splitk_epilogue(a, splits, a.NP - p0, false, st);
    g_last_combine = -splits;
    XM_LAUNCH_CHECK();
  }
  return XM_OK;
}

// *ran = 0: the layer's full-extent bits cannot be reproduced on the lattice (full_extent_plan); nothing was launched
static int conv_forward_lattice(const float *x, const float *f, const float *b, float *y, const Geo &g, const float *scale,
                                const float *shift, int relu, int ly, int lx, hipStream_t st, int *ran) {
  *ran = 0;
  const bool padded = (g.pt | g.pb | g.pl | g.pr) != 0;
  const bool bigTaps = g.FH * g.FW > 63;
  if (bigTaps && padded) return XM_OK;          // (the full-extent call reports it)
  // filter groups: forward_run selects per group (the alignment of a group's slice of Y decides its candidates); not
  // worth a plan per group -- such a layer stays at full extent
  if (g.G != 1) return XM_OK;
  const int Rp = (g.R + kBK - 1) / kBK * kBK;
  const bool need_pad = (g.R % kBK) != 0 || ((uintptr_t)f & 15);
  const int mode = (padded || Rp != g.R) ? 1 : 0;
  const int NP = g.Ho * g.Wo * g.N;
  const bool have_slab = slab_floats(g.Kg, NP, Rp, kNumCfg, g.FH, g.FW, g.R) > 0;
  const int PI = lattice_extent(g.Ho, ly), PJ = lattice_extent(g.Wo, lx), NPl = PI * PJ * g.N;
  FwdOperands o{x, f, b, scale, shift, nullptr, nullptr, y, nullptr, g.R, Rp, relu, bigTaps, fwd_dma_ok(g, x, f, need_pad, mode)};
  FullExtentPlan p;
  if (!full_extent_plan(g, forward_args(g, 0, o), x, mode, have_slab, st, p)) return XM_OK;
  const int nkt = Rp / kBK;
  const int z = p.hyS > 1 ? p.hyS : (nkt + p.tps - 1) / p.tps;       // slabs of the split launch (1: none)
  const long long cut = p.hyS > 1 ? lattice_pixels_below(p.hyP0, g.Ho, g.Wo, ly, lx) : 0;   // lattice pixels of the unsplit prefix
  const int n0 = (int)(cut / (PI * PJ));                // the split launch of a hybrid plan starts at this sample
  const int NPz = NPl - n0 * PI * PJ;                   // ... and covers this many lattice pixels
  const size_t slabf = z > 1 ? (size_t)z * g.Kg * ((NPz + 3) & ~3) : 0;
  WsCarver ws;
  int rc = ws.init(WsCarver::need(need_pad ? (size_t)g.K * Rp : 0, 4) + WsCarver::need(slabf, 4), st);
  if (rc) return rc;
  o.taps = device_taps(fwd_tap_table(g, Rp, bigTaps));
  if (!o.taps) return fail(XM_ENOMEM, "vl_nnconv: tap table allocation failed");
  if (need_pad) {
    float *Ap = ws.take<float>((size_t)g.K * Rp);
    const size_t n = (size_t)g.K * Rp;
    hipLaunchKernelGGL(pad_filter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, f, Ap, g.K, g.R, Rp);
    XM_LAUNCH_CHECK();
    o.A = Ap;
    o.lda = Rp;
  }
  float *slab = slabf ? ws.take<float>(slabf) : nullptr;
  for (int grp = 0; grp < g.G; ++grp) {
    ConvGemmArgs a = forward_args(g, grp, o);
    a.PI = PI, a.PJ = PJ, a.NP = NPl;
    a.divPIJ = make_fastdiv((uint32_t)(PI * PJ)), a.divPI = make_fastdiv((uint32_t)PI);
    a.gsy = g.sy * ly, a.gsx = g.sx * lx;       // the gather origin of lattice pixel (i, j) is that of output pixel (ly i, lx j)
    a.osy = ly, a.osx = lx;                     // ... and that is where it is stored (OH, channel and sample strides: full extent)
    a.vecStore = 0, a.dmaOk = 0;                // lattice neighbours are never adjacent in Y
    if (p.hyS <= 1) {
      rc = launch_gemm_lattice(a, mode, p.ci, p.tps, slab, 0, st);
      if (rc) return rc;
      continue;
    }
    // hybrid plan: the lattice pixels below the cut are one chain each, the others hyS-way sums with the hybrid's cut points
    if (cut > 0) {
      ConvGemmArgs a1 = a;
      a1.NP = (int)cut;
      rc = launch_gemm_lattice(a1, mode, p.ci, nkt, nullptr, 0, st);
      if (rc) return rc;
    }
    if (cut < NPl) {
      // the kernels enumerate pixels from 0: the split launch starts at the sample that holds the cut and its combine
      // skips the pixels below it (they are computed twice, less than one sample)
      ConvGemmArgs a2 = a;
      const size_t xskip = (size_t)n0 * g.H * g.W * g.C;
      a2.X += xskip, a2.xBytes -= (unsigned)(xskip * 4), a2.Y += (size_t)n0 * a.oSampleStride;
      a2.NP = NPz;
      rc = launch_gemm_lattice(a2, mode, p.ci, p.hyTps, slab, (int)(cut - (long long)n0 * PI * PJ), st);
      if (rc) return rc;
    }
  }
  *ran = 1;
  return XM_OK;
}

// ---- prepared dgrad operands ------------------------------------------------------------------
// The dgrad GEMM reads the filter bank transposed / split by stride parity (prep_dgrad_filter_kernel).  In a
// training step that is ~20 us per layer ON THE CRITICAL PATH of the backward pass.  xm_nnconv_prepare_backward
// lets the host run the transposition early -- typically while the forward pass of the same step runs, on a
// side stream -- into a persistent buffer; the backward call then finds it and skips the kernel.  An entry is
// valid while the parameter version it was built at is current (xm_sgd_update / xm_solver_update / xm_average_update /
// xm_params_changed bump the version) and the geometry matches.
struct PrepKey {
  const float *f;
  int FH, FW, FC, K, G, sy, sx, dy, dx, pt, pl, H, W, fold;   // (N, pb, pr do not shape the operand; C does through G)
  bool operator<(const PrepKey &o) const { return memcmp(this, &o, sizeof(PrepKey)) < 0; }
};
struct PrepEntry {
  float *buf = nullptr;
  size_t bytes = 0;
  unsigned long long version = ~0ull;
  hipEvent_t ev = nullptr;
  hipStream_t st = nullptr;
};
static std::map<PrepKey, PrepEntry> g_prep;
unsigned long long g_param_version = 1;   // bumped by every parameter update (misc.hip)
static PrepKey prep_key(const float *f, const Geo &g, bool fold) {
  PrepKey k;
  memset(&k, 0, sizeof k);
  k.f = f, k.FH = g.FH, k.FW = g.FW, k.FC = g.FC, k.K = g.K, k.G = g.G, k.sy = g.sy, k.sx = g.sx, k.dy = g.dy, k.dx = g.dx;
  k.pt = g.pt, k.pl = g.pl, k.H = g.H, k.W = g.W, k.fold = fold ? 1 : 0;
  return k;
}

// ---- dgrad of 5 x 5 / stride 2 layers with both row parities per wave (conv_dgrad_s2_kernel, round 5) ---------------------
static int g_force_dgrad_s2 = -1;   // test hook (xm_debug_force_dgrad_s2): 0 = never, 1 / -1 = wherever it can run
static bool dgrad_s2_ok(const Geo &g, const float *dzdy, const float *dxo, const float *accum) {
  if (!path_on(kPathDgradS2) || g_force_dgrad_s2 == 0 || forced_tiling()) return false;
  if (!dgrad_s2_can(g, (uintptr_t)dzdy, (uintptr_t)dxo, accum != nullptr)) return false;
  if (g_force_dgrad_s2 == 1) return true;
  // Its blocks are large (two output columns x 64 row pairs x all filters: ~0.4 ms of a CU slot) and there are 37 of them per
  // 126 x 73 sample, so small batches pay the partly filled last round -- 32 spectrograms: 1.54 rounds of 768 slots cost 2
  // (90 against 95 TFLOP/s for the merged launch), 64: 3.08 rounds cost 4 and the 40 KB blocks are poor neighbours of the
  // filter derivative on the side stream (student step - 4 %); 256: 12.3 rounds, 124 against 115 TFLOP/s and - 0.5 ms per
  // step.  A function of the shape only: launches of at least XM_DGRAD_S2_MIN_BLOCKS blocks (default 6 rounds of the chip).
  static const long long min_blocks = env_int("XM_DGRAD_S2_MIN_BLOCKS", 6 * 768);
  const long long per_sample = (long long)((g.W + 3) / 4 + (g.W + 2) / 4) * (((g.H + 1) / 2 + 63) / 64) * ((g.C + kDgS2Rows - 1) / kDgS2Rows);
  return per_sample * g.N >= min_blocks;
}
static int launch_dgrad_s2(const float *dzdy, const float *f, float *dxo, const Geo &g, hipStream_t st) {
  DgradS2Args a{};
  a.dY = dzdy;
  a.dX = dxo;
  a.dyBytes = (unsigned)((size_t)g.Ho * g.Wo * g.K * g.N * 4);
  a.C = g.C, a.K = g.K, a.H = g.H, a.W = g.W, a.Ho = g.Ho, a.Wo = g.Wo;
  a.pl = g.pl;
  a.nbm = (g.C + kDgS2Rows - 1) / kDgS2Rows;
  a.nkg = g.K / 8;
  a.nmt = ((g.H + 1) / 2 + 63) / 64;
  int blocks = 0;
  for (int px = 0; px < 2; ++px) {
    a.xfirst[px] = ((px - g.pl) % 2 + 2) % 2;               // columns x with (x + pl) % 2 == px
    const int ncols = a.xfirst[px] < g.W ? (g.W - a.xfirst[px] + 1) / 2 : 0;
    a.ncg[px] = (ncols + 1) / 2;
    a.nv[px] = px == 0 ? 3 : 2;                              // v = px, px + 2, (px + 4)
    blocks += a.ncg[px] * a.nmt * a.nbm;
  }
  const size_t fdFloats = (size_t)a.nbm * 2 * 3 * a.nkg * kDgS2Tile;
  WsCarver ws;
  int rc = ws.init(WsCarver::need(fdFloats, 4), st);
  if (rc) return rc;
  float *Fd = ws.take<float>(fdFloats);
  a.Fd = Fd;
  hipLaunchKernelGGL(prep_dgrad_s2_kernel, dim3((unsigned)std::min<size_t>((fdFloats + 255) / 256, 2048)), dim3(256), 0, st, f,
                     Fd, g.C, g.K, a.nbm, a.nkg, g.pl);
  XM_LAUNCH_CHECK();
  {
    ProfScope ps(prof_key(kProfDgradS2), 2.0 * g.K * (double)g.Ho * g.Wo * g.N * g.R, st,
                 (double)a.dyBytes + 4.0 * g.K * g.R + 4.0 * g.C * (double)g.H * g.W * g.N);
    hipLaunchKernelGGL(conv_dgrad_s2_kernel<1>, dim3((unsigned)(blocks * g.N)), dim3(256), 0, st, a);
  }
  XM_LAUNCH_CHECK();
  return XM_OK;
}

// The dgrad GEMMs' A operands -- the filter bank transposed / split by stride parity, one [FC (* FH)][Rp] block per class
// and group -- in one buffer, and the split-K scratch.
struct DgradFilters {
  char *base = nullptr;
  std::vector<size_t> off;   // byte offset of class ic
  float *slab = nullptr;
  float *of(const Geo &g, const DgradClass &c, size_t ic, int grp, bool foldH) const {
    return (float *)(base + off[ic]) + (size_t)grp * g.FC * (foldH ? g.FH : 1) * c.Rp;
  }
};
// pure transpose (see transpose_filter_kernel): 1 x 1 filters, or an FH x 1 filter folded into the GEMM rows
static bool dgrad_pure_transpose(const Geo &g, const DgradClass &c, bool foldH, const float *f, const float *Ag) {
  const int Rrows = g.FC * (foldH ? g.FH : 1);
  return g.FW == 1 && ((foldH && c.nU == g.FH && c.nV == 1) || (g.FH == 1 && !foldH)) && c.Rp == g.Kg &&
         (Rrows & 3) == 0 && (g.Kg & 3) == 0 && g.G == 1 && (((uintptr_t)f | (uintptr_t)Ag) & 15) == 0 &&
         path_on(kPathFastTranspose);
}
static int launch_dgrad_filter(const float *f, float *Ag, const Geo &g, const DgradClass &c, int grp, bool foldH, hipStream_t st) {
  g_last_dgrad_transpose = dgrad_pure_transpose(g, c, foldH, f, Ag) ? 1 : 0;
  if (g_last_dgrad_transpose) {
    const int Rrows = g.FC * (foldH ? g.FH : 1);
    hipLaunchKernelGGL(transpose_filter_kernel, dim3((Rrows + 63) / 64, (g.Kg + 63) / 64), dim3(256), 0, st, f, Ag,
                       g.Kg, Rrows, c.Rp);
    XM_LAUNCH_CHECK();
    return XM_OK;
  }
  const int T = g.FH * g.FW;
  const int TS = T <= 14 ? 32 : (T <= 56 ? 16 : 8);
  size_t lds = sizeof(float) * (size_t)TS * (TS * T + 1);
  const int nT = c.nU * c.nV, used = (foldH ? c.nV : nT) * g.Kg;
  PrepDiv pd;
  pd.tsT = make_fastdiv((uint32_t)(TS * T)), pd.T = make_fastdiv((uint32_t)T);
  pd.tsNT = make_fastdiv((uint32_t)std::max(1, TS * nT)), pd.nT = make_fastdiv((uint32_t)std::max(1, nT));
  pd.nU = make_fastdiv((uint32_t)std::max(1, c.nU));
  pd.padc = make_fastdiv((uint32_t)std::max(1, c.Rp - used));
  pd.rows = make_fastdiv((uint32_t)(foldH ? std::max(1, c.nU) : 1));
  hipLaunchKernelGGL(prep_dgrad_filter_kernel, dim3((g.FC + TS - 1) / TS, (g.Kg + TS - 1) / TS),
                     dim3(256), lds, st, f + (size_t)g.R * g.Kg * grp, Ag, g.FH, g.FW, g.FC, g.Kg,
                     c.u0, c.ustep, c.nU, c.v0, c.vstep, c.nV, c.Rp, TS, foldH ? 1 : 0, pd);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

// Transposed filters: from the persistent cache when a current entry exists, else built now -- into the cache
// (prepare_only: the entry is then stamped with the parameter version and its event recorded on `st`) or into scratch.
static int dgrad_filter_operand(const float *f, const Geo &g, const std::vector<DgradClass> &cls, bool foldH,
                                size_t slab_floats, bool prepare_only, hipStream_t st, WsCarver &ws, DgradFilters &F) {
  size_t abytes = 0;
  for (const DgradClass &c : cls) {
    F.off.push_back(abytes);
    abytes += WsCarver::need((size_t)g.FC * (foldH ? g.FH : 1) * c.Rp * g.G, 4);
  }
  const PrepKey pkey = prep_key(f, g, foldH);
  PrepEntry *pe = nullptr;
  bool have_prepared = false;
  if (prepare_only) {
    pe = &g_prep[pkey];
    if (pe->bytes < abytes) {
      if (pe->buf) {
        XM_HIP(hipDeviceSynchronize());
        (void)hipFree(pe->buf);
      }
      pe->buf = nullptr;
      XM_HIP(hipMalloc((void **)&pe->buf, abytes));
      pe->bytes = abytes;
    }
    if (!pe->ev) XM_HIP(hipEventCreateWithFlags(&pe->ev, hipEventDisableTiming));
  } else {
    auto it = g_prep.find(pkey);
    if (it != g_prep.end() && it->second.version == g_param_version && it->second.bytes >= abytes) {
      pe = &it->second;
      have_prepared = true;
      if (pe->st != st) XM_HIP(hipStreamWaitEvent(st, pe->ev, 0));
    }
    g_last_dgrad_prepared = have_prepared ? 1 : 0;
  }
  int rc = ws.init((pe ? 0 : abytes) + WsCarver::need(slab_floats, 4), st);
  if (rc) return rc;
  F.base = pe ? (char *)pe->buf : ws.base;
  F.slab = slab_floats ? (float *)(ws.base + (pe ? 0 : abytes)) : nullptr;
  for (size_t ic = 0; ic < cls.size() && !have_prepared; ++ic)
    for (int grp = 0; grp < g.G; ++grp) {
      rc = launch_dgrad_filter(f, F.of(g, cls[ic], ic, grp, foldH), g, cls[ic], grp, foldH, st);
      if (rc) return rc;
    }
  if (prepare_only) {
    pe->version = g_param_version;
    pe->st = st;
    XM_HIP(hipEventRecord(pe->ev, st));
  }
  return XM_OK;
}

// what every class and group of a dgrad call shares
struct DgradOperands {
  const float *dzdy, *accum;
  float *dxo;
  bool foldH;
  double pair_total;   // (pixel, tap) pairs over all classes: apportions the algorithmic work
};

// the implicit-GEMM problem of class `c`, filter group `grp`: dY is the gather source, dX the (strided) destination
static ConvGemmArgs dgrad_args(const Geo &g, const DgradClass &c, int grp, const DgradOperands &o, const float *Ag,
                               const int2 *taps) {
  const bool foldH = o.foldH;
  const DgradGather q = dgrad_gather(g, c, foldH);
  ConvGemmArgs a{};
  const size_t xoff = (size_t)grp * g.Kg * g.Ho * g.Wo, yoff = (size_t)grp * g.FC * g.H * g.W;
  a.A = Ag, a.lda = c.Rp, a.taps = taps;
  a.X = o.dzdy + xoff, a.xBytes = (unsigned)((y_elements(g) - xoff) * 4), a.xSampleStride = g.Ho * g.Wo * g.K;
  a.Y = o.dxo + yoff, a.resid = o.accum ? o.accum + yoff : nullptr;
  a.M = foldH ? g.FC * g.FH : g.FC, a.Rp = c.Rp, a.Rtrue = c.Rc;
  a.PI = foldH ? 1 : c.PI, a.PJ = c.PJ, a.NP = a.PI * c.PJ * g.N;
  a.divPIJ = make_fastdiv((uint32_t)(a.PI * c.PJ)), a.divPI = make_fastdiv((uint32_t)a.PI);
  a.gsy = 1, a.gsx = 1, a.gh0 = q.gh0, a.gw0 = q.gw0, a.LimH = g.Ho, a.LimW = g.Wo;
  a.nU = q.nU, a.nV = c.nV, a.du0 = q.du0, a.dus = q.dus, a.dv0 = q.dv0, a.dvs = q.dvs;
  a.osy = foldH ? 0 : g.sy, a.oh0 = foldH ? 0 : c.hi0;    // foldH: the destination row comes from the GEMM row (m % FH)
  a.osx = g.sx, a.ow0 = c.wi0, a.OH = g.H;
  a.oChanStride = g.H * g.W, a.oSampleStride = g.H * g.W * g.C;
  a.divMU = make_fastdiv(foldH ? (uint32_t)g.FH : 1u), a.oUStride = foldH ? 1 : 0;
  a.vecStore = (!foldH && g.sy == 1 && g.sx == 1 && (c.PI * c.PJ) % 4 == 0 && c.PI == g.H &&
                c.PJ == g.W && (((uintptr_t)a.Y | (uintptr_t)a.resid) & 15) == 0) ? 1 : 0;
  // algorithmic work of dgrad == forward MACs (2*Ho*Wo*N*K*R), apportioned over the classes by
  // their share of (pixel, tap) pairs; masked-out pairs are not work
  a.algoFlops = 2.0 * g.Ho * g.Wo * (double)g.N * g.Kg * g.R * ((double)a.NP * c.Rc) / o.pair_total;
  return a;
}

// FC-shaped layer over few pixels (the student's fc7, the SE gates of a trainable teacher): dX = W^T dY is the
// skinny forward product with the transposed filter bank as its filter -- `gs` is that product's geometry
static bool dgrad_as_skinny_fc(const Geo &g, bool pure_t, bool foldH, const float *accum, Geo &gs) {
  if (!pure_t || foldH || accum || g.FH != 1 || g.sy != 1 || g.sx != 1 || (g.pt | g.pb | g.pl | g.pr) != 0 ||
      g.H * g.W != 1 || (g.FC & 3) != 0 || g.N > 512 || forced_tiling())
    return false;
  gs = g;
  gs.C = gs.FC = g.Kg;
  gs.K = gs.Kg = g.FC;
  gs.R = g.Kg;
  return fc_skinny_ok(gs, true);
}

// one class by itself: the best implicit-GEMM configuration, the halo-patch variants against it
static int dgrad_run_class(const Geo &g, const DgradClass &c, const ConvGemmArgs &a, bool foldH, float *slab, hipStream_t st) {
  auto gemm = [&](int ci) {
    int sp;
    gemm_slab_floats(a, ci, &sp);
    ConvGemmArgs aa = a;
    return launch_gemm(aa, 1, ci, sp, slab, st);
  };
  const TuneKey key = tune_key_class_dgrad(1, g, c, a.M, a.NP, a.PI);
  const int ci = tune_cfg(key, pick_cfg(a.M, a.NP, c.Rp / kBK), st, gemm, kNumBaseCfg, w8_skip(a.M, a.NP));
  ConvGemmArgs ah = a;
  const int hneed = (!forced_tiling() && !foldH) ? halo_setup_padded(ah, g.N) : 0;
  const bool hok[4] = {true, halo_var_ok(ah, hneed, 0), halo_var_ok(ah, hneed, 1), halo_var_ok(ah, hneed, 2)};
  auto arm = [&](int h) { return h ? launch_halo(ah, h - 1, slab, st) : gemm(ci); };
  return arm(select_arm(5, key, st, 4, hok, kHaloMargin, halo_forced(hok), arm));
}

// merged launch: 2-4 classes, no filter groups, and enough tiles per class that none would be split
static bool dgrad_merge_ok(const Geo &g, const std::vector<DgradClass> &cls, bool foldH) {
  if (g.G != 1 || foldH || cls.size() < 2 || cls.size() > 4 || g_force_splits != 0 || !path_on(kPathDgradMerge)) return false;
  // the merged launch never splits K: it needs enough tiles in total to fill the chip by itself
  long long tiles = 0;
  for (const DgradClass &c : cls) tiles += (long long)((g.FC + 127) / 128) * (((long long)c.PI * c.PJ * g.N + 255) / 256);
  return tiles >= 512;
}

// all stride-parity classes in one launch (each alone is a fraction more than one round of the chip)
static int dgrad_run_merged(const Geo &g, const std::vector<ConvGemmArgs> &merged, hipStream_t st) {
  auto gemm = [&](int ci) { return launch_gemm_multi(merged, ci, st); };
  long long npSum = 0;
  int rpMax = 0;
  for (const ConvGemmArgs &a : merged) {
    npSum += a.NP;
    rpMax = std::max(rpMax, a.Rp);
  }
  const TuneKey key = tune_key_merged_dgrad(3, g, merged[0].M, npSum, rpMax, (int)merged.size());
  const int ci = tune_cfg(key, pick_cfg(merged[0].M, npSum, rpMax / kBK), st, gemm, kNumBaseCfg, w8_skip(merged[0].M, npSum));
  // every class a halo-patch problem (unit-stride gathers of <= 3 x 3 taps in dY space)?  Then the same variant for all
  std::vector<ConvGemmArgs> mh = merged;
  bool hok[4] = {true, g_force_cfg < 0, g_force_cfg < 0, g_force_cfg < 0};
  for (ConvGemmArgs &a : mh) {
    const int need = hok[1] || hok[2] || hok[3] ? halo_setup_padded(a, g.N) : 0;
    for (int v = 0; v < 3; ++v) hok[v + 1] = hok[v + 1] && halo_var_ok(a, need, v);
  }
  // the tall-patch variant may serve classes that would also fit the short one (hok[3] && !hok[2]: as it stands);
  // classes of mixed patch height: let the tall variant take them all if each fits 1024
  if (!hok[3]) {
    bool all = g_force_cfg < 0;
    for (ConvGemmArgs &a : mh) {
      ConvGemmArgs t = a;
      const int need = all ? halo_setup_padded(t, g.N) : 0;
      all = all && need > 0 && need <= 1024 && t.M % 96 == 0;
    }
    hok[3] = all && !hok[2];
  }
  auto arm = [&](int h) { return h ? launch_halo_multi(mh, h - 1, st) : gemm(ci); };
  return arm(select_arm(6, key, st, 4, hok, kHaloMargin, halo_forced(hok), arm));
}

// dX: one implicit GEMM per stride-parity class (a, b) of the input pixels (conv_plan.h).
// accum != NULL: dX = dgrad + accum (the derivative another branch of a fork already produced), added in
// the GEMM epilogue instead of by a separate pass
// prepare_only: run just the filter transpositions into the persistent cache (xm_nnconv_prepare_backward)
static int conv_dgrad(const float *f, const float *dzdy, float *dxo, const Geo &g, hipStream_t st,
                      const float *accum = nullptr, bool prepare_only = false) {
  if (!prepare_only) g_last_dgrad_prepared = -1;   // until dgrad_filter_operand says where the operand came from
  if (dgrad_s2_ok(g, dzdy, dxo, accum)) {
    // the student's conv2: both row parities per wave, whole-line stores (conv_dgrad_s2_kernel); its filter operand is laid
    // out by a 3 MB pass inside the call, so there is nothing to prepare ahead
    if (prepare_only) return XM_OK;
    return launch_dgrad_s2(dzdy, f, dxo, g, st);
  }
  // plan
  const bool foldH = dgrad_fold_h(g);
  bool covers_all = true;
  const std::vector<DgradClass> cls = dgrad_classes(g, foldH, &covers_all);
  // pixels whose class has no tap (e.g. 1x1 stride 2) receive no gradient
  if (!prepare_only && (!covers_all || cls.empty())) {
    const size_t bytes = sizeof(float) * x_elements(g);
    if (accum)
      XM_HIP(hipMemcpyAsync(dxo, accum, bytes, hipMemcpyDeviceToDevice, st));
    else
      XM_HIP(hipMemsetAsync(dxo, 0, bytes, st));
  }
  if (cls.empty()) return XM_OK;
  for (const DgradClass &c : cls)
    if (c.nU * c.nV > 63)
      return fail(XM_ENOTSUP, "vl_nnconv: more than 63 spatial taps per stride class is not built");
  size_t slab_max = 0;   // split-K scratch of the largest class (foldH: no halo-patch problem)
  for (const DgradClass &c : cls)
    slab_max = std::max(slab_max, slab_floats(foldH ? g.FC * g.FH : g.FC, (foldH ? 1 : c.PI) * c.PJ * g.N, c.Rp, kNumBaseCfg,
                                              foldH ? 0 : c.nU, foldH ? 0 : c.nV, c.Rc));
  // operands: the transposed filters and the tap tables (both also when only preparing: the backward call finds them)
  WsCarver ws;
  DgradFilters F;
  int rc = dgrad_filter_operand(f, g, cls, foldH, slab_max, prepare_only, st, ws, F);
  if (rc) return rc;
  std::vector<const int2 *> taps;
  for (const DgradClass &c : cls) {
    taps.push_back(device_taps(dgrad_tap_table(g, c, foldH)));
    if (!taps.back()) return fail(XM_ENOMEM, "vl_nnconv: tap table allocation failed");
  }
  if (prepare_only) return XM_OK;
  // launch
  DgradOperands o{dzdy, accum, dxo, foldH, 0.0};
  for (const DgradClass &c : cls) o.pair_total += (double)(foldH ? 1 : c.PI) * c.PJ * g.N * c.Rc;
  const bool merge = dgrad_merge_ok(g, cls, foldH);
  std::vector<ConvGemmArgs> merged;
  for (size_t ic = 0; ic < cls.size(); ++ic)
    for (int grp = 0; grp < g.G; ++grp) {
      const DgradClass &c = cls[ic];
      const float *Ag = F.of(g, c, ic, grp, foldH);
      Geo gs;
      if (dgrad_as_skinny_fc(g, dgrad_pure_transpose(g, c, foldH, f, Ag), foldH, accum, gs)) {
        rc = fc_skinny_forward(dzdy, Ag, nullptr, dxo, gs, 0, st);
        if (rc) return rc;
        continue;
      }
      const ConvGemmArgs a = dgrad_args(g, c, grp, o, Ag, taps[ic]);
      if (merge) {
        merged.push_back(a);
        continue;
      }
      rc = dgrad_run_class(g, c, a, foldH, F.slab, st);
      if (rc) return rc;
    }
  return merge ? dgrad_run_merged(g, merged, st) : XM_OK;
}

// one wgrad launch (+ split reduction) with tile configuration ci; `part` has room for 1024 slabs
static int wgrad_run(const float *x, const float *dzdy, float *dfo, const Geo &g, int ci, float *part,
                     hipStream_t st) {
  ci = wgrad_cfg(ci);
  const Cfg &c = kCfgs[ci];
  const int NP = g.Ho * g.Wo * g.N;
  const int nkt = (NP + kBK - 1) / kBK;
  const int nbm = (g.Kg + c.bm() - 1) / c.bm(), nbn = (g.R + c.bn() - 1) / c.bn();
  const int Rn = nbn * c.bn();
  // split the pixel reduction so that the grid fills one round of the chip (no tail round);
  // smaller tiles co-reside more blocks per CU
  const int tiles = nbm * nbn;
  const int slots = 256 * (c.bm() * c.bn() >= 128 * 128 ? 2 : (c.bm() * c.bn() >= 64 * 128 ? 3 : 6));
  int splits = std::max(1, std::min(nkt / 8, slots / tiles));
  splits = std::min(splits, 1024);
  int tps = (nkt + splits - 1) / splits;
  splits = (nkt + tps - 1) / tps;
  g_last_wgrad_splits = splits;
  const int4 *taps = device_taps(wgrad_tap_table(g, Rn));
  if (!taps) return fail(XM_ENOMEM, "vl_nnconv: tap table allocation failed");
  const size_t slab = (size_t)g.Kg * g.R;
  for (int grp = 0; grp < g.G; ++grp) {
    WgradArgs a{};
    const size_t xoff = (size_t)grp * g.FC * g.H * g.W, doff = (size_t)grp * g.Kg * g.Ho * g.Wo;
    float *dst = dfo + (size_t)grp * g.Kg * g.R;
    a.dY = dzdy + doff, a.dyBytes = (unsigned)((y_elements(g) - doff) * 4);
    a.X = x + xoff, a.xBytes = (unsigned)((x_elements(g) - xoff) * 4);
    a.out = splits > 1 ? part : dst, a.taps = taps;
    a.M = g.Kg, a.R = g.R, a.Rn = Rn, a.ldo = g.R;
    a.Ho = g.Ho, a.Wo = g.Wo, a.NP = NP;
    a.divHW = make_fastdiv((uint32_t)(g.Ho * g.Wo)), a.divHo = make_fastdiv((uint32_t)g.Ho);
    a.sy = g.sy, a.sx = g.sx, a.pt = g.pt, a.pl_ = g.pl, a.H = g.H, a.W = g.W;
    a.xSampleStride = g.H * g.W * g.C, a.dyChanStride = g.Ho * g.Wo, a.dySampleStride = g.Ho * g.Wo * g.K;
    a.nbm = nbm, a.nbn = nbn, a.tilesPerSplit = tps, a.nkt = nkt, a.splitStride = slab;
    {
      const int av = wgrad_av(a);
      ProfScope ps(prof_key(kProfWgrad, ci * 4 + (av == 4 ? 2 : av == 2 ? 1 : 0)), 2.0 * g.Kg * (double)NP * g.R, st,
                   (double)a.xBytes + (double)a.dyBytes + 4.0 * g.Kg * g.R);
      launch_wgrad_cfg(ci, a, dim3(nbm * nbn, splits), st);
    }
    XM_LAUNCH_CHECK();
    if (splits > 1) {
      launch_reduce_splits(part, dst, slab, splits, slab, st);
      XM_LAUNCH_CHECK();
    }
  }
  return XM_OK;
}

// ---- filter derivative of the single-channel stem (conv_stem_wgrad_kernel) ------------------------------------------
static bool stem_wgrad_ok(const Geo &g, const float *x, const float *dzdy) {
  if (!path_on(kPathStem) || !path_on(kPathStemWgrad) || forced_tiling()) return false;
  if (!stem_wgrad_can(g, (uintptr_t)x, (uintptr_t)dzdy)) return false;
  return g_force_stem == 1 || fills_chip(g);
}

// BNP (bnp != NULL): `dzdy` is the convolution's own OUTPUT, the derivative is rebuilt on the fly (StemWgradArgs)
struct StemBnp {
  const float *dP;
  const unsigned char *amax;
  const float *rowc;
  int pHo, pWo;
  float *dbias;      // NULL, or dzdb of the convolution (column R of the partials multiplies ones)
};
static int launch_stem_wgrad(const float *x, const float *dzdy, float *dfo, const Geo &g, float *part, int grid, hipStream_t st,
                             const StemBnp *bnp = nullptr) {
  StemWgradArgs a{};
  a.dY = dzdy, a.X = x, a.part = part;
  a.M = g.Kg, a.R = g.R, a.nU = g.FH, a.nV = g.FW;
  a.PI = g.Ho, a.PJ = g.Wo, a.NP = g.Ho * g.Wo * g.N;
  a.divPIJ = make_fastdiv((uint32_t)(g.Ho * g.Wo)), a.divPI = make_fastdiv((uint32_t)g.Ho);
  a.gsx = g.sx, a.gh0 = -g.pt, a.gw0 = -g.pl, a.LimH = g.H, a.LimW = g.W;
  a.xSampleStride = g.H * g.W, a.dySampleStride = g.Ho * g.Wo * g.K, a.dyChanStride = g.Ho * g.Wo;
  a.onesCol = -1;
  if (bnp) {
    a.dP = bnp->dP, a.amax = bnp->amax, a.rowc = bnp->rowc, a.pHo = bnp->pHo, a.pWo = bnp->pWo;
    const size_t pooled = (size_t)bnp->pHo * bnp->pWo * g.K * g.N;
    a.dpBytes = (unsigned)(pooled * 4);
    a.amBytes = (unsigned)pooled;
    a.dyBytes = (unsigned)((size_t)g.Ho * g.Wo * g.K * g.N * 4);
    if (bnp->dbias) a.onesCol = g.R;
  }
  static bool attr_done = false;
  if (!attr_done) {
    XM_HIP(hipFuncSetAttribute((const void *)conv_stem_wgrad_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, kStemWgSmem));
    XM_HIP(hipFuncSetAttribute((const void *)conv_stem_wgrad_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, kStemWgSmem));
    XM_HIP(hipFuncSetAttribute((const void *)conv_stem_wgrad_bnp_kernel<2, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, kStemWgSmemBnp));
    XM_HIP(hipFuncSetAttribute((const void *)conv_stem_wgrad_bnp_kernel<2, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, kStemWgSmemBnp));
    XM_HIP(hipFuncSetAttribute((const void *)conv_stem_wgrad_bnp_kernel<2, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, kStemWgSmemBnp));
    XM_HIP(hipFuncSetAttribute((const void *)conv_stem_wgrad_bnp_kernel<1, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, kStemWgSmemBnp));
    XM_HIP(hipFuncSetAttribute((const void *)conv_stem_wgrad_bnp_kernel<1, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, kStemWgSmemBnp));
    XM_HIP(hipFuncSetAttribute((const void *)conv_stem_wgrad_bnp_kernel<1, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, kStemWgSmemBnp));
    attr_done = true;
  }
  const int ntiles = (a.NP + 127) / 128;
  {
    // BNP reads the convolution's output once (as the plain kernel reads dY) + the pooled derivative and its table
    const double abytes = 4.0 * g.H * g.W * g.N + 4.0 * a.M * (double)a.NP + 4.0 * a.M * a.R +
                          (bnp ? 5.0 * bnp->pHo * bnp->pWo * (double)g.K * g.N : 0.0);
    ProfScope ps(prof_key(kProfStemWgrad, bnp ? 1 : 0), 2.0 * a.M * (double)a.NP * a.R, st, abytes);
    if (bnp) {
      const int ones = a.onesCol < 0 ? 0 : (a.onesCol < 32 ? 1 : 2);
#define XM_BNP_LAUNCH(SY_, ON_) hipLaunchKernelGGL((conv_stem_wgrad_bnp_kernel<SY_, ON_>), dim3(grid), dim3(256), kStemWgSmemBnp, st, a, ntiles)
      if (g.sy == 2) {
        if (ones == 0) XM_BNP_LAUNCH(2, 0); else if (ones == 1) XM_BNP_LAUNCH(2, 1); else XM_BNP_LAUNCH(2, 2);
      } else {
        if (ones == 0) XM_BNP_LAUNCH(1, 0); else if (ones == 1) XM_BNP_LAUNCH(1, 1); else XM_BNP_LAUNCH(1, 2);
      }
#undef XM_BNP_LAUNCH
    } else {
      if (g.sy == 2) hipLaunchKernelGGL(conv_stem_wgrad_kernel<2>, dim3(grid), dim3(256), kStemWgSmem, st, a, ntiles);
      else hipLaunchKernelGGL(conv_stem_wgrad_kernel<1>, dim3(grid), dim3(256), kStemWgSmem, st, a, ntiles);
    }
  }
  XM_LAUNCH_CHECK();
  hipLaunchKernelGGL(conv_stem_wgrad_reduce_kernel, dim3(a.M), dim3(1024), 0, st, part, dfo, grid, a.M, a.R,
                     bnp ? bnp->dbias : nullptr);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

// ---- filter derivative of 3 x 3 / stride 1 / pad 1 layers from an input patch (conv_wgrad_patch_kernel) -------------------
// Hosts that declared XM_EXEC_SINGLE_STREAM only (xm_set_exec_hint; the reference's own call sequence, cnn_train_dag ->
// vl_nnconv one after the other -- the MEX binding sets it; bench.py --serial): alone the kernel is 11 ... 22 % faster than the generic one (profiles/r04/wgrad_patch_bench.txt), a step on one
// stream 1.7 %; launched on a side stream next to the dgrad of the same layer it fills the chip with three 48 KB blocks per CU
// for its whole life and the pair takes LONGER than with the generic kernel (student step at 64: - 1.5 %).
// The choice depends on the shape, the tuning table and that explicit hint -- never on what the process called before.
static bool wgrad_patch_ok(const Geo &g, const float *x, const float *dzdy) {
  if (!path_on(kPathWgradPatch) || forced_tiling()) return false;
  // a candidate for hosts that declared one stream, and -- whatever the host does -- for launches of at least
  // XM_WGRAD_PATCH_MIN_STAGES output columns (default 4096: the batch-256 layers, which fill the chip for ~2 ms by
  // themselves; like the eight-wave rule "from 1024 tiles" a function of the shape only)
  static const long long min_stages = env_int("XM_WGRAD_PATCH_MIN_STAGES", 4096);
  if (g_force_wgrad_patch < 0 && !(g_exec_hint & XM_EXEC_SINGLE_STREAM) && (long long)g.N * g.W < min_stages) return false;
  if (!wgrad_patch_can(g, (uintptr_t)x, (uintptr_t)dzdy)) return false;
  return (long long)g.N * g.W >= 64;                                    // enough stages to split
}
// stages per split and the split count of a patch wgrad launch: tiles x splits fill one round of 3 blocks per CU
static int patch_splits(int nStages, int tiles, int max_splits, int *stagesPerSplit) {
  static const int slots = std::max(64, (int)env_int("XM_WGRAD_PATCH_SLOTS", 768));
  const int splits = std::max(1, std::min(std::min(nStages / 8, slots / std::max(1, tiles)), max_splits));
  *stagesPerSplit = (nStages + splits - 1) / splits;
  return (nStages + *stagesPerSplit - 1) / *stagesPerSplit;
}
static int launch_wgrad_patch(const float *x, const float *dzdy, float *dfo, const Geo &g, float *part, int max_splits,
                              hipStream_t st) {
  WgradPatchArgs a{};
  a.dY = dzdy, a.dyBytes = (unsigned)(y_elements(g) * 4), a.X = x, a.xBytes = (unsigned)(x_elements(g) * 4);
  a.M = g.Kg, a.R = g.R, a.ldo = g.R, a.C = g.C, a.W = g.W, a.K = g.K;
  a.nStages = g.N * g.W;
  a.nbm = (g.Kg + 127) / 128, a.nbn = (g.R + 127) / 128;
  const int tiles = a.nbm * a.nbn, splits = patch_splits(a.nStages, tiles, max_splits, &a.stagesPerSplit);
  const size_t slab = (size_t)g.Kg * g.R;
  g_last_wgrad_splits = splits;
  a.splitStride = slab;
  a.out = splits > 1 ? part : dfo;
  {
    ProfScope ps(prof_key(kProfWgradPatch), 2.0 * g.Kg * (double)g.Ho * g.Wo * g.N * g.R, st, (double)a.xBytes + (double)a.dyBytes + 4.0 * slab);
    hipLaunchKernelGGL(conv_wgrad_patch_kernel<30>, dim3(tiles, splits), dim3(256), 0, st, a);
  }
  XM_LAUNCH_CHECK();
  if (splits > 1) {
    launch_reduce_splits(part, dfo, slab, splits, slab, st);
    XM_LAUNCH_CHECK();
  }
  return XM_OK;
}

// ---- filter derivative of 5 x 5 / stride 2 layers from an input patch (conv_wgrad_patch_s2_kernel, round 5) ------------------
// The student's conv2 (44 % of its arithmetic).  Unlike the 3 x 3 patch kernel above this one is a candidate for every caller
// (measured once per shape against the best generic configuration): 53 KB of LDS per block, three blocks per CU.
static int g_force_wgrad_patch_s2 = -1; // test hook (xm_debug_force_wgrad_patch_s2)
static bool wgrad_patch_s2_ok(const Geo &g, const float *x, const float *dzdy) {
  if (!path_on(kPathWgradPatchS2) || forced_tiling()) return false;
  if (!wgrad_patch_s2_can(g, (uintptr_t)x, (uintptr_t)dzdy)) return false;
  return (long long)g.N * g.Wo * ((g.Ho + 31) / 32) >= 64;              // enough stages to split
}
static int launch_wgrad_patch_s2(const float *x, const float *dzdy, float *dfo, const Geo &g, float *part, int max_splits,
                                 hipStream_t st) {
  WgradPatchS2Args a{};
  a.dY = dzdy, a.dyBytes = (unsigned)(y_elements(g) * 4), a.X = x, a.xBytes = (unsigned)(x_elements(g) * 4);
  a.M = g.Kg, a.R = g.R, a.ldo = g.R, a.C = g.C;
  a.H = g.H, a.W = g.W, a.Ho = g.Ho, a.Wo = g.Wo, a.K = g.K;
  a.pt = g.pt, a.pl = g.pl;
  a.nSeg = (g.Ho + 31) / 32;
  a.nStages = g.N * g.Wo * a.nSeg;
  a.nbm = (g.Kg + 127) / 128, a.nbn = (g.R + 127) / 128;
  const int tiles = a.nbm * a.nbn, splits = patch_splits(a.nStages, tiles, max_splits, &a.stagesPerSplit);
  a.splits = splits;
  g_last_wgrad_splits = splits;
  const size_t slab = (size_t)g.Kg * g.R;
  a.splitStride = slab;
  a.out = splits > 1 ? part : dfo;
  {
    ProfScope ps(prof_key(kProfWgradPatchS2), 2.0 * g.Kg * (double)g.Ho * g.Wo * g.N * g.R, st, (double)a.xBytes + (double)a.dyBytes + 4.0 * slab);
    hipLaunchKernelGGL((conv_wgrad_patch_s2_kernel<5, 2>), dim3(tiles * splits), dim3(256), 0, st, a);
  }
  XM_LAUNCH_CHECK();
  if (splits > 1) {
    launch_reduce_splits(part, dfo, slab, splits, slab, st);
    XM_LAUNCH_CHECK();
  }
  return XM_OK;
}

static int conv_wgrad(const float *x, const float *dzdy, float *dfo, const Geo &g, hipStream_t st) {
  // analytic fallback: minimal padded work (split-K supplies the parallelism)
  int fb = 0;
  double best = 1e300;
  for (int i = 0; i < kNumWgradCfg; ++i) {
    const Cfg &cc = kCfgs[i];
    const double cost = (double)((g.Kg + cc.bm() - 1) / cc.bm() * cc.bm()) * ((g.R + cc.bn() - 1) / cc.bn() * cc.bn()) * cfg_eff(cc);
    if (cost < best) best = cost, fb = i;
  }
  const int NP = g.Ho * g.Wo * g.N;
  const int nkt = (NP + kBK - 1) / kBK;
  const size_t slab = (size_t)g.Kg * g.R;
  const int max_splits = std::max(1, std::min(1024, nkt / 8));
  const bool stem = stem_wgrad_ok(g, x, dzdy);
  const int stem_grid_ = stem ? stem_grid(NP) : 0;
  WsCarver ws;
  int rc = ws.init(WsCarver::need(slab * max_splits, 4) + WsCarver::need((size_t)stem_grid_ * 96 * 64, 4), st);
  if (rc) return rc;
  float *part = ws.take<float>(slab * max_splits);
  float *spart = stem ? ws.take<float>((size_t)stem_grid_ * 96 * 64) : nullptr;
  auto run = [&](int ci) { return wgrad_run(x, dzdy, dfo, g, ci, part, st); };
  const TuneKey key = tune_key_wgrad(2, g);
  const int ci = tune_cfg(key, fb, st, run, kNumWgradCfg);
  // one special-purpose kernel at the most against the best generic configuration (measured once per shape).  The patch
  // kernels remove work -- gathers and address arithmetic -- so they do not have to clear the margin the equal-work
  // challengers need: DESIGN.md 2.1f
  if (stem) {
    auto arm = [&](int h) { return h ? launch_stem_wgrad(x, dzdy, dfo, g, spart, stem_grid_, st) : run(ci); };
    return arm(select_arm(8, key, st, 2, kOneChallenger, kHaloMargin, g_force_stem, arm));
  }
  if (wgrad_patch_ok(g, x, dzdy)) {
    auto arm = [&](int h) { return h ? launch_wgrad_patch(x, dzdy, dfo, g, part, max_splits, st) : run(ci); };
    return arm(select_arm(9, key, st, 2, kOneChallenger, 0.01f, g_force_wgrad_patch, arm));
  }
  if (wgrad_patch_s2_ok(g, x, dzdy)) {
    auto arm = [&](int h) { return h ? launch_wgrad_patch_s2(x, dzdy, dfo, g, part, max_splits, st) : run(ci); };
    return arm(select_arm(10, key, st, 2, kOneChallenger, 0.01f, g_force_wgrad_patch_s2, arm));
  }
  return run(ci);
}

}  // namespace xm

using namespace xm;

// the test / tools switches behind xm_debug_set / xm_debug_get: name, the global it drives, how a request is normalised
static int norm_tri(int v) { return v < 0 ? -1 : (v ? 1 : 0); }
static const struct DebugSwitch {
  const char *name;
  int *value;
  int (*normalise)(int);
} kDebugSwitches[] = {
    {"conv_cfg", &g_force_cfg, [](int v) { return (v >= 0 && v < kNumCfg) ? v : -1; }},
    {"conv_splits", &g_force_splits, [](int v) { return v > 0 ? v : 0; }},
    {"conv_halo", &g_force_halo, [](int v) { return v < 0 ? -1 : std::min(v, 3); }},
    {"conv_stem", &g_force_stem, norm_tri},         {"conv_stem3", &g_force_stem3, norm_tri},
    {"wgrad_patch", &g_force_wgrad_patch, norm_tri}, {"wgrad_patch_s2", &g_force_wgrad_patch_s2, norm_tri},
    {"dgrad_s2", &g_force_dgrad_s2, norm_tri},
    {"spec_blocks", &g_spec_blocks, [](int v) { return v > 0 ? v : 0; }},
    {"conv_split_want", &g_conv_split_want, norm_tri},
};
static const DebugSwitch *debug_switch(const char *key) {
  for (const DebugSwitch &s : kDebugSwitches)
    if (key && strcmp(key, s.name) == 0) return &s;
  return nullptr;
}

extern "C" {

// ONE entry for the test / tools switches (round-5 review: the library exported eleven xm_debug_* functions that set
// process-global state).  Returns the previous value, INT_MIN for an unknown key.  Keys and values: include/xmodal_prof.h.
int xm_debug_set(const char *key, int value) {
  if (const DebugSwitch *s = debug_switch(key)) {
    const int old = *s->value;
    *s->value = s->normalise(value);
    return old;
  }
  if (key && strcmp(key, "comm_single") == 0) return comm_force_single(value);
  return INT_MIN;
}
int xm_debug_get(const char *key) {
  if (key && strcmp(key, "num_conv_cfgs") == 0) return kNumCfg;
  if (key && strcmp(key, "conv_last_combine") == 0) return g_last_combine;
  if (key && strcmp(key, "conv_last_lattice") == 0) return g_last_lattice;
  if (key && strcmp(key, "wgrad_last_splits") == 0) return g_last_wgrad_splits;
  if (key && strcmp(key, "bias_grad_last_splits") == 0) return g_last_bias_splits;
  if (key && strcmp(key, "stats_last_splits") == 0) return g_last_stats_splits;
  if (key && strcmp(key, "dgrad_last_transpose") == 0) return g_last_dgrad_transpose;
  if (key && strcmp(key, "dgrad_last_prepared") == 0) return g_last_dgrad_prepared;
  const DebugSwitch *s = debug_switch(key);
  return s ? *s->value : INT_MIN;
}

int xm_set_exec_hint(unsigned flags) {
  if (flags & ~(unsigned)XM_EXEC_SINGLE_STREAM) return fail(XM_EINVAL, "xm_set_exec_hint: unknown flag bits 0x%x", flags);
  g_exec_hint = flags;
  return XM_OK;
}
unsigned xm_get_exec_hint(void) { return g_exec_hint; }


// ---- persistent tuning table (include/xmodal.h) ----------------------------------------------
int xm_tune_load(const char *path) {
  return g_tune.load(path && path[0] ? path : tune_default_path().c_str());
}
int xm_tune_save(const char *path) {
  tune_load_once();   // merge with the default file
  const std::string p = path && path[0] ? std::string(path) : tune_default_path();
  const int rc = g_tune.save(p.c_str());
  if (rc == 1) return fail(XM_EINVAL, "xm_tune_save: cannot write %s.tmp", p.c_str());
  if (rc) return fail(XM_EINVAL, "xm_tune_save: rename to %s failed", p.c_str());
  return XM_OK;
}
int xm_tune_entries(int *total, int *unsaved) {
  tune_load_once();
  if (total) *total = g_tune.size();
  if (unsaved) *unsaved = g_tune.unsaved;
  return XM_OK;
}
// on = 1: every block (< 4096) of every later conv_gemm launch records {first clock, last clock, HW_ID, XCC_ID};
// out (4 * nblocks words) receives the records of the most recent launch (caller synchronises first).
// Debugging / tools only.
#ifdef XM_DEBUG_CYCLES   // (tools build only: XM_DEBUG_CYCLES=1 python -m mcncrossmodalemotions_amd.build)
int xm_debug_conv_cycles(int on, unsigned long long *out, int nblocks) {
  const size_t bytes = 4096 * 4 * sizeof(unsigned long long);
  if (on && !g_dbg_cycles) {
    if (hipMalloc((void **)&g_dbg_cycles, bytes) != hipSuccess) return XM_ENOMEM;
    (void)hipMemset(g_dbg_cycles, 0, bytes);
  }
  if (out && g_dbg_cycles)
    (void)hipMemcpy(out, g_dbg_cycles, (size_t)std::min(nblocks, 4096) * 32, hipMemcpyDeviceToHost);
  if (!on && g_dbg_cycles) {
    (void)hipFree(g_dbg_cycles);
    g_dbg_cycles = nullptr;
  }
  return XM_OK;
}
#endif

// The fused forward behind xm_nnconv_forward_fused (gate == NULL) / _gated / _strided_residual: the residual has the
// extent res_H x res_W x K x N and is read at (oy * res_sy, ox * res_sx); res_H == 0: at output extent, unit stride.
static int fused_forward(const float *x, int H, int W, int C, int N, const float *f, int FH, int FW,
                         int FC, int K, const float *b, float *y, int sy, int sx, int pt, int pb,
                         int pl, int pr, int dy, int dx, const float *scale, const float *shift,
                         const float *gate, const float *residual, int res_H, int res_W, int res_sy,
                         int res_sx, int flags, void *stream) {
  Geo g;
  int rc = make_geo(g, H, W, C, N, FH, FW, FC, K, sy, sx, pt, pb, pl, pr, dy, dx);
  if (rc) return rc;
  if (res_H == 0) res_H = g.Ho, res_W = g.Wo, res_sy = res_sx = 1;
  if (!x || !f || !y) return fail(XM_EINVAL, "vl_nnconv: NULL tensor");
  if ((scale == nullptr) != (shift == nullptr))
    return fail(XM_EINVAL, "vl_nnconv(fused): scale and shift must be given together");
  if ((flags & XM_FUSE_RELU) && (flags & XM_FUSE_SIGMOID))
    return fail(XM_EINVAL, "vl_nnconv(fused): relu and sigmoid are exclusive");
  if (gate && (flags & XM_FUSE_SIGMOID)) return fail(XM_ENOTSUP, "vl_nnconv(gated): sigmoid epilogue is not built");
  if (residual) {
    if (res_sy < 1 || res_sx < 1 || res_H < 1 || res_W < 1 || g.Ho != (res_H - 1) / res_sy + 1 ||
        g.Wo != (res_W - 1) / res_sx + 1)
      return fail(XM_EINVAL, "vl_nnconv(fused): a %d x %d residual sampled with stride [%d %d] does not give the %d x %d output",
                  res_H, res_W, res_sy, res_sx, g.Ho, g.Wo);
    if ((long long)res_H * res_W * g.K * g.N >= (1LL << 30))
      return fail(XM_ETOOBIG, "vl_nnconv(fused): residual with >= 2^30 elements (4 GiB)");
  }
  hipStream_t st = (hipStream_t)stream;
  if (!gate && !residual && fc_skinny_ok(g))
    return fc_skinny_forward(x, f, b, y, g, (flags & XM_FUSE_SIGMOID) ? 2 : ((flags & XM_FUSE_RELU) ? 1 : 0), st, scale,
                             shift);
  rc = conv_forward(x, f, b, y, g, scale, shift, residual, (flags & XM_FUSE_RELU) ? 1 : 0, st, nullptr, 0.f, gate, res_H,
                    res_W, res_sy, res_sx);
  if (rc || !(flags & XM_FUSE_SIGMOID)) return rc;
  return xm_nnsigmoid(y, (size_t)g.Ho * g.Wo * g.K * g.N, nullptr, y, stream);  // in place (elementwise)
}

int xm_nnconv_forward_fused(const float *x, int H, int W, int C, int N, const float *f, int FH,
                            int FW, int FC, int K, const float *b, float *y, int sy, int sx,
                            int pt, int pb, int pl, int pr, int dy, int dx, const float *scale,
                            const float *shift, const float *residual, int flags, void *stream) {
  return fused_forward(x, H, W, C, N, f, FH, FW, FC, K, b, y, sy, sx, pt, pb, pl, pr, dy, dx, scale, shift, nullptr, residual,
                       0, 0, 1, 1, flags, stream);
}

int xm_nnconv_forward_strided_residual(const float *x, int H, int W, int C, int N, const float *f, int FH, int FW,
                                       int FC, int K, const float *b, float *y, int sy, int sx, int pt, int pb,
                                       int pl, int pr, int dy, int dx, const float *scale, const float *shift,
                                       const float *gate, const float *residual, int res_H, int res_W, int res_sy,
                                       int res_sx, int flags, void *stream) {
  if (residual && res_H < 1) return fail(XM_EINVAL, "vl_nnconv(fused): residual extent must be positive");
  return fused_forward(x, H, W, C, N, f, FH, FW, FC, K, b, y, sy, sx, pt, pb, pl, pr, dy, dx, scale, shift, gate, residual,
                       residual ? res_H : 0, res_W, res_sy, res_sx, flags, stream);
}

int xm_nnconv_forward_lattice(const float *x, int H, int W, int C, int N, const float *f, int FH, int FW, int FC, int K,
                              const float *b, float *y, int sy, int sx, int pt, int pb, int pl, int pr, int dy, int dx,
                              const float *scale, const float *shift, const float *residual, int flags, int lat_y,
                              int lat_x, void *stream) {
  Geo g;
  int rc = make_geo(g, H, W, C, N, FH, FW, FC, K, sy, sx, pt, pb, pl, pr, dy, dx);
  if (rc) return rc;
  if (!x || !f || !y) return fail(XM_EINVAL, "vl_nnconv: NULL tensor");
  if (lat_y < 1 || lat_x < 1) return fail(XM_EINVAL, "vl_nnconv(lattice): the lattice steps must be >= 1, got [%d %d]", lat_y, lat_x);
  if ((scale == nullptr) != (shift == nullptr))
    return fail(XM_EINVAL, "vl_nnconv(fused): scale and shift must be given together");
  if (residual) return fail(XM_ENOTSUP, "vl_nnconv(lattice): a residual operand is not built");
  if (flags & ~XM_FUSE_RELU) return fail(XM_ENOTSUP, "vl_nnconv(lattice): only the ReLU epilogue is built");
  g_last_lattice = 0;
  int ran = 0;
  if ((lat_y > 1 || lat_x > 1) && !fc_skinny_ok(g)) {
    rc = conv_forward_lattice(x, f, b, y, g, scale, shift, (flags & XM_FUSE_RELU) ? 1 : 0, lat_y, lat_x, (hipStream_t)stream, &ran);
    if (rc) return rc;
  }
  g_last_lattice = ran;
  if (ran) return XM_OK;
  // bits before FLOPs: the layer at full extent (every lattice pixel is among its pixels)
  return fused_forward(x, H, W, C, N, f, FH, FW, FC, K, b, y, sy, sx, pt, pb, pl, pr, dy, dx, scale, shift, nullptr, nullptr, 0, 0,
                       1, 1, flags, stream);
}

int xm_nnconv_forward_moments(const float *x, int H, int W, int C, int N, const float *f, int FH, int FW,
                              int FC, int K, const float *b, float *y, int sy, int sx, int pt, int pb,
                              int pl, int pr, int dy, int dx, float epsilon, float *moments_out, void *stream) {
  Geo g;
  int rc = make_geo(g, H, W, C, N, FH, FW, FC, K, sy, sx, pt, pb, pl, pr, dy, dx);
  if (rc) return rc;
  if (!x || !f || !y || !moments_out) return fail(XM_EINVAL, "vl_nnconv(+moments): NULL tensor");
  hipStream_t st = (hipStream_t)stream;
  if (fc_skinny_ok(g)) {
    g_last_stats_splits = 0;
    rc = fc_skinny_forward(x, f, b, y, g, 0, st);
    return rc ? rc : bn_batch_moments(y, g.Ho, g.Wo, g.K, g.N, epsilon, moments_out, st);
  }
  return conv_forward(x, f, b, y, g, nullptr, nullptr, nullptr, 0, st, moments_out, epsilon);
}

int xm_nnconv_forward_gated(const float *x, int H, int W, int C, int N, const float *f, int FH, int FW,
                            int FC, int K, const float *b, float *y, int sy, int sx, int pt, int pb,
                            int pl, int pr, int dy, int dx, const float *scale, const float *shift,
                            const float *gate, const float *residual, int flags, void *stream) {
  if (!gate) return fail(XM_EINVAL, "vl_nnconv(gated): NULL tensor");     // (every other check: fused_forward)
  return fused_forward(x, H, W, C, N, f, FH, FW, FC, K, b, y, sy, sx, pt, pb, pl, pr, dy, dx, scale, shift, gate, residual,
                       0, 0, 1, 1, flags, stream);
}

int xm_nnconv_forward(const float *x, int H, int W, int C, int N, const float *f, int FH, int FW,
                      int FC, int K, const float *b, float *y, int sy, int sx, int pt, int pb,
                      int pl, int pr, int dy, int dx, void *stream) {
  return xm_nnconv_forward_fused(x, H, W, C, N, f, FH, FW, FC, K, b, y, sy, sx, pt, pb, pl, pr, dy,
                                 dx, nullptr, nullptr, nullptr, 0, stream);
}

int xm_nnconv_prepare_backward(int H, int W, int C, int N, const float *f, int FH, int FW, int FC, int K,
                               int sy, int sx, int pt, int pb, int pl, int pr, int dy, int dx, void *stream) {
  Geo g;
  int rc = make_geo(g, H, W, C, N, FH, FW, FC, K, sy, sx, pt, pb, pl, pr, dy, dx);
  if (rc) return rc;
  if (!f) return fail(XM_EINVAL, "vl_nnconv: F is NULL");
  return conv_dgrad(f, nullptr, nullptr, g, (hipStream_t)stream, nullptr, true);
}

int xm_params_changed(void) {
  ++g_param_version;
  return XM_OK;
}

// dzdf (+ dzdb) of a first-layer convolution whose output feeds vl_nnbnorm -> vl_nnrelu -> vl_nnpool('max') and nothing
// else (the student's conv1 -> bn1 -> relu1 -> pool1, emoVoxZoo.m:50-62 / Appendix B.1), together with the bnorm's dg / db:
// the bnorm's DZDX -- the widest tensor of the backward pass, 462 MB at 32 spectrograms -- is rebuilt inside the
// filter-derivative kernel from the pooled derivative and the routing table instead of being written by
// xm_nnbnorm_relu_pool_backward and read back by xm_nnconv_backward.  XM_ENOTSUP when the geometry is not the one the
// kernel is written for (single-channel stem, 3 x 3 / stride-2 unpadded pooling): the caller then makes the two calls.
int xm_nnconv_backward_filter_bnrelupool(const float *x, int H, int W, int C, int N, int FH, int FW, int FC, int K, int sy,
                                         int sx, int pt, int pb, int pl, int pr, int dy, int dx, const float *y,
                                         const float *bn_g, const float *bn_b, const float *moments, int train, int ph,
                                         int pw, int psy, int psx, int ppt, int ppb, int ppl, int ppr,
                                         const unsigned char *argmax, const float *y_pool, const float *dzdy_pool,
                                         float *df_out, float *dbias_out, float *dg_out, float *db_out, void *stream) {
  Geo g;
  int rc = make_geo(g, H, W, C, N, FH, FW, FC, K, sy, sx, pt, pb, pl, pr, dy, dx);
  if (rc) return rc;
  if (!x || !y || !bn_g || !bn_b || !moments || !argmax || !dzdy_pool || !df_out)
    return fail(XM_EINVAL, "vl_nnconv(filter derivative through bnorm+relu+pool): NULL tensor");
  hipStream_t st = (hipStream_t)stream;
  const int pHo = out_size(g.Ho, ppt, ppb, ph, 1, psy), pWo = out_size(g.Wo, ppl, ppr, pw, 1, psx);
  const bool ok = g_force_stem != 0 && stem_wgrad_can(g, (uintptr_t)x, (uintptr_t)y) && g.K == g.Kg && y_pool != nullptr &&
                  pool3x3s2_unpadded(ph, pw, psy, psx, ppt, ppb, ppl, ppr) && (g.Ho & 1) == 0 && pHo >= 1 && pWo >= 1 &&
                  (!dbias_out || g.R < 64) && fits_i32_bytes((size_t)pHo * pWo * g.K * g.N);
  if (!ok)
    return fail(XM_ENOTSUP, "vl_nnconv(filter derivative through bnorm+relu+pool): geometry not covered by the fused kernel");
  const int grid = stem_grid(g.Ho * g.Wo * g.N);
  WsCarver ws;
  rc = ws.init(WsCarver::need((size_t)6 * g.K, 4) + WsCarver::need((size_t)grid * 96 * 64, 4) + bnpool_sums_need(g.K, g.N), st);
  if (rc) return rc;
  float *rowc = ws.take<float>((size_t)6 * g.K);
  float *spart = ws.take<float>((size_t)grid * 96 * 64);
  rc = bnpool_backward_sums(ws, y, g.Ho, g.Wo, g.K, g.N, bn_g, bn_b, moments, train, ph, pw, psy, psx, ppt, ppb, ppl, ppr,
                            argmax, y_pool, dzdy_pool, dg_out, db_out, rowc, st);
  if (rc) return rc;
  StemBnp bnp{dzdy_pool, argmax, rowc, pHo, pWo, dbias_out};
  return launch_stem_wgrad(x, y, df_out, g, spart, grid, st, &bnp);
}

int xm_nnconv_backward(const float *x, int H, int W, int C, int N, const float *f, int FH, int FW,
                       int FC, int K, const float *dzdy, float *dx_out, float *df_out,
                       float *db_out, int sy, int sx, int pt, int pb, int pl, int pr, int dy,
                       int dx, void *stream) {
  return xm_nnconv_backward_accum(x, H, W, C, N, f, FH, FW, FC, K, dzdy, dx_out, df_out, db_out, sy, sx, pt,
                                  pb, pl, pr, dy, dx, nullptr, stream);
}

int xm_nnconv_backward_accum(const float *x, int H, int W, int C, int N, const float *f, int FH, int FW,
                             int FC, int K, const float *dzdy, float *dx_out, float *df_out,
                             float *db_out, int sy, int sx, int pt, int pb, int pl, int pr, int dy,
                             int dx, const float *dx_accum, void *stream) {
  Geo g;
  int rc = make_geo(g, H, W, C, N, FH, FW, FC, K, sy, sx, pt, pb, pl, pr, dy, dx);
  if (rc) return rc;
  if (!dzdy) return fail(XM_EINVAL, "vl_nnconv: DZDY is NULL in backward mode");
  hipStream_t st = (hipStream_t)stream;
  if (db_out) {
    int S = std::max(1, std::min(N, 2048 / K));
    if ((long long)g.Ho * g.Wo < 1024) S = 1;
    WsCarver ws;
    rc = ws.init(WsCarver::need((size_t)K * S, 8), st);
    if (rc) return rc;
    double *part = ws.take<double>((size_t)K * S);
    const int HWo = g.Ho * g.Wo;
    const bool vec = (HWo & 3) == 0 && ((uintptr_t)dzdy & 15) == 0;   // 16-byte loads of whole pixel quads
    g_last_bias_splits = S;
    hipLaunchKernelGGL(bias_grad_partial_kernel, dim3(K, S), dim3(256), 0, st, dzdy, part, HWo, K, N, S, vec ? 1 : 0,
                       make_fastdiv((uint32_t)(vec ? HWo >> 2 : HWo)));
    XM_LAUNCH_CHECK();
    hipLaunchKernelGGL(bias_grad_finalize_kernel, dim3((K + 3) / 4), dim3(256), 0, st, part, db_out,
                       K, S);
    XM_LAUNCH_CHECK();
  }
  if (df_out) {
    if (!x) return fail(XM_EINVAL, "vl_nnconv: X is NULL but DZDF requested");
    rc = conv_wgrad(x, dzdy, df_out, g, st);
    if (rc) return rc;
  }
  if (dx_out) {
    if (!f) return fail(XM_EINVAL, "vl_nnconv: F is NULL but DZDX requested");
    if (dx_accum == dx_out) return fail(XM_EINVAL, "vl_nnconv: dx_accum must not alias dx_out");
    rc = conv_dgrad(f, dzdy, dx_out, g, st, dx_accum);
    if (rc) return rc;
  }
  return XM_OK;
}
}

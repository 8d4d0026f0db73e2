// The bf16x3 arm of vl_nnconv for 1 x 1 layers (xm_nnconv_forward_split, ABI 124): the GEMM of a 1 x 1 convolution on the
// bf16 matrix cores with every fp32 operand split in two bf16 halves.  An independent unit: conv.hip's dispatch, the tuning
// table and the fp32 kernels do not know it; nothing reaches it unless the caller asks for XM_CONV_BF16X3.
//
//   v = hi + lo + r,  hi = bf16(v) (round to nearest even),  lo = bf16(v - hi)  (v - hi is exact in fp32),
//   |v - hi| <= 2^-8 |v|,  |r| <= 2^-16 |v|.
// Per 16 reduction steps THREE v_mfma_f32_32x32x16_bf16 add into ONE fp32 accumulator, small terms first:
//   acc += x_lo * f_hi;   acc += x_hi * f_lo;   acc += x_hi * f_hi
// (every bf16 x bf16 product is exact in fp32).  Dropped per product: x_lo f_lo + r_x f + x r_f, at most 3 * 2^-16 |x| |f|
// plus second-order terms -- derived, not measured.  c ascends, the C tail is zero-filled, one accumulation chain per
// output, never split-K, no atomics: the bits of an output element depend on its own operands only -- not on N, not on
// which other pixels the call computes, not on what the process ran before.
//
// Layout of the work: A = filters (rows = output channels), B = activations (columns = output pixels), so a register of
// the 32 x 32 accumulator holds 32 consecutive pixels of one channel and stores 128 contiguous bytes.  Pixels are numbered
// across samples (a 128-pixel tile may cross a sample boundary: 7 x 7 maps fill their tiles).  The fp32 tiles are split on
// their way into LDS by the thread that loaded them: the thread holds eight consecutive channels of ONE pixel (eight
// coalesced loads across the wave), so it writes the eight hi and the eight lo halves as two 16-byte row pieces with c
// contiguous -- the transposition the B operand needs happens in registers, and both operands are read back with plain
// 16-byte LDS reads.  The two bf16 planes of a tile take exactly the bytes its fp32 form would.
#include "conv_plan.h"
#include "conv_split_plan.h"
#include "prof.h"
#include "xm_common.h"

namespace xm {

// test switch behind xm_debug_set("conv_split_want", v): what xm_nnconv_split_geometry reports as WANT
//   -1 the measured rule (default), 0 never, 1 wherever the kernel can run
int g_conv_split_want = -1;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// LDS row of a pixel (x tile) or an output channel (f tile): 32 hi halves, 32 lo halves, 16 bytes of padding.  144 bytes =
// 36 banks: the rows of 16 consecutive lanes start 9 sixteen-byte slots apart (odd), so a 16-byte read of one column piece by
// 16 rows touches every slot once.
constexpr int kSplitRow = 2 * kSplitBC * 2 + 16;
constexpr int kSplitLo = kSplitBC * 2;   // byte offset of the lo plane inside a row

struct SplitArgs {
  const float *x, *f, *bias, *scale, *shift, *gate, *resid;
  float *y;
  int C, K;
  int H, HW;               // rows and pixels of an input map (HW: channel stride of x)
  int Ho, P, NP;           // rows and pixels of an output map; P * N
  int sy, sx;
  int rH, rHW, rsy, rsx;   // residual: rows, pixels of a map, sampling strides
  int relu, kTiles;
};

__device__ __forceinline__ void split_pair(const float (&v)[8], bf16x8 &hi, bf16x8 &lo) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const __bf16 h = (__bf16)v[j];
    hi[j] = h;
    lo[j] = (__bf16)(v[j] - (float)h);
  }
}

// grid: kTiles * ceil(NP / 128) blocks of 256 threads, output-channel tile fastest (the blocks that read one pixel tile run
// next to each other).  Four waves as 2 (pixels) x 2 (output channels): a wave owns 64 pixels x 32 channels = two accumulators.
__global__ __launch_bounds__(kSplitThreads) void conv_split_kernel(const SplitArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[(kSplitBP + kSplitBK) * kSplitRow];
  unsigned char *Xs = lds, *Fs = lds + kSplitBP * kSplitRow;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kt = (int)(blockIdx.x % (unsigned)a.kTiles), ptile = (int)(blockIdx.x / (unsigned)a.kTiles);
  const int p0 = ptile * kSplitBP, k0 = kt * kSplitBK;

  // staging roles.  x: pixel tid & 127, channels 16 * (tid >> 7) .. + 15 of a stage; f: output channel tid >> 2, channels
  // 8 * (tid & 3) .. + 7.  Every load is in bounds (clamped) and masked afterwards: no branch around a load.
  const int sp = p0 + (tid & 127);
  const bool spv = sp < a.NP;
  uint32_t xoff = 0;
  if (spv) {
    const uint32_t n = (uint32_t)sp / (uint32_t)a.P, q = (uint32_t)sp - n * (uint32_t)a.P;
    const uint32_t ox = q / (uint32_t)a.Ho, oy = q - ox * (uint32_t)a.Ho;
    xoff = oy * a.sy + (uint32_t)a.H * (ox * a.sx) + (uint32_t)a.HW * (uint32_t)a.C * n;
  }
  const int xc = 16 * (tid >> 7);
  const int fk = k0 + (tid >> 2), fc = 8 * (tid & 3);
  const bool fkv = fk < a.K;
  const float *xp = a.x + xoff;
  const float *fp = a.f + (size_t)a.C * (fkv ? fk : 0);
  unsigned char *xrow = Xs + (tid & 127) * kSplitRow + 2 * xc;
  unsigned char *frow = Fs + (tid >> 2) * kSplitRow + 2 * fc;

  float xr[2][8], fr[8];
  auto load = [&](int c0) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int c = c0 + xc + j;
      const float v = xp[(size_t)min(c, a.C - 1) * a.HW];
      xr[j >> 3][j & 7] = (spv && c < a.C) ? v : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + fc + j;
      const float v = fp[min(c, a.C - 1)];
      fr[j] = (fkv && c < a.C) ? v : 0.f;
    }
  };
  auto stage = [&]() {
    bf16x8 hi, lo;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      split_pair(xr[g], hi, lo);
      *reinterpret_cast<bf16x8 *>(xrow + 16 * g) = hi;
      *reinterpret_cast<bf16x8 *>(xrow + 16 * g + kSplitLo) = lo;
    }
    split_pair(fr, hi, lo);
    *reinterpret_cast<bf16x8 *>(frow) = hi;
    *reinterpret_cast<bf16x8 *>(frow + kSplitLo) = lo;
  };

  // MFMA operand maps (32x32x16 bf16): lane l, r = l & 31, h = l >> 5 holds A[row r][k = 8 h + j], B[k = 8 h + j][col r]
  const int r = lane & 31, h = lane >> 5;
  const int wp = (wave & 1) * 64, wk = (wave >> 1) * 32;
  const unsigned char *fa = Fs + (wk + r) * kSplitRow + 16 * h;
  const unsigned char *xb = Xs + (wp + r) * kSplitRow + 16 * h;
  f32x16 acc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

  const int stages = (a.C + kSplitBC - 1) / kSplitBC;
  load(0);
  for (int st = 0; st < stages; ++st) {
    stage();
    __syncthreads();
    if (st + 1 < stages) load((st + 1) * kSplitBC);
#pragma unroll
    for (int s = 0; s < kSplitBC / kSplitStep; ++s) {
      if (st * kSplitBC + s * kSplitStep < a.C) {   // (uniform) a step that is all zero fill adds nothing
        const bf16x8 fhi = *reinterpret_cast<const bf16x8 *>(fa + 32 * s);
        const bf16x8 flo = *reinterpret_cast<const bf16x8 *>(fa + 32 * s + kSplitLo);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const bf16x8 xhi = *reinterpret_cast<const bf16x8 *>(xb + 32 * t * kSplitRow + 32 * s);
          const bf16x8 xlo = *reinterpret_cast<const bf16x8 *>(xb + 32 * t * kSplitRow + 32 * s + kSplitLo);
          // the fixed term order, small terms first: x_lo f_hi, x_hi f_lo, x_hi f_hi
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fhi, xlo, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(flo, xhi, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fhi, xhi, acc[t], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  // epilogue, fp32, the order of operations of the fp32 kernels: ((v + b) * scale + shift) * gate + residual, relu.
  // C/D map: register i of lane l is row (i & 3) + 8 (i >> 2) + 4 h, column r.
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int p = p0 + wp + 32 * t + r;
    if (p >= a.NP) continue;
    const uint32_t n = (uint32_t)p / (uint32_t)a.P, q = (uint32_t)p - n * (uint32_t)a.P;
    float *yp = a.y + q + (uint32_t)a.P * (uint32_t)a.K * n;
    const float *rp = nullptr;
    if (a.resid) {
      const uint32_t ox = q / (uint32_t)a.Ho, oy = q - ox * (uint32_t)a.Ho;
      rp = a.resid + (oy * a.rsy + (uint32_t)a.rH * (ox * a.rsx) + (uint32_t)a.rHW * (uint32_t)a.K * n);
    }
    const float *gp = a.gate ? a.gate + (size_t)a.K * n : nullptr;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int k = k0 + wk + (i & 3) + 8 * (i >> 2) + 4 * h;
      if (k >= a.K) continue;
      float v = acc[t][i];
      if (a.bias) v += a.bias[k];
      if (a.scale) v = v * a.scale[k] + a.shift[k];
      if (gp) v *= gp[k];
      if (rp) v += rp[(size_t)k * a.rHW];
      if (a.relu) v = fmaxf(v, 0.f);
      yp[(size_t)k * a.P] = v;
    }
  }
}

static SplitShape split_shape(int H, int W, int C, int N, int FH, int FW, int FC, int K, int sy, int sx, int pt, int pb,
                              int pl, int pr, int dy, int dx, int flags) {
  return SplitShape{H, W, C, N, FH, FW, FC, K, sy, sx, pt, pb, pl, pr, dy, dx, flags};
}

}  // namespace xm

using namespace xm;

extern "C" {

int xm_nnconv_split_geometry(int H, int W, int C, int N, int FH, int FW, int FC, int K, int sy, int sx, int pt, int pb,
                             int pl, int pr, int dy, int dx, int flags, int *can, int *want, int *blocks, int *launches) {
  const SplitShape s = split_shape(H, W, C, N, FH, FW, FC, K, sy, sx, pt, pb, pl, pr, dy, dx, flags);
  const bool ok = split_can(s, XM_FUSE_SIGMOID);
  const SplitLaunch l = ok ? split_launch(s) : SplitLaunch{0, 0, 0, 0};
  if (can) *can = ok ? 1 : 0;
  if (want) *want = ok && (g_conv_split_want < 0 ? split_want(s) : g_conv_split_want != 0) ? 1 : 0;
  if (blocks) *blocks = l.blocks;
  if (launches) *launches = l.launches;
  return XM_OK;
}

int xm_nnconv_forward_split(const float *x, int H, int W, int C, int N, const float *f, int FH, int FW, int FC, int K,
                            const float *b, float *y, int sy, int sx, int pt, int pb, int pl, int pr, int dy, int dx,
                            const float *scale, const float *shift, const float *gate, const float *residual, int res_H,
                            int res_W, int res_sy, int res_sx, int flags, int precision, void *stream) {
  if (precision == XM_CONV_F32)
    return fail(XM_EINVAL, "vl_nnconv(split): XM_CONV_F32 is the other entry points' (xm_nnconv_forward_strided_residual)");
  if (precision != XM_CONV_BF16X3) return fail(XM_EINVAL, "vl_nnconv(split): unknown precision %d", precision);
  Geo g;
  int rc = make_geo(g, H, W, C, N, FH, FW, FC, K, sy, sx, pt, pb, pl, pr, dy, dx);
  if (rc) return rc;
  if (flags & ~(XM_FUSE_RELU | XM_FUSE_SIGMOID)) return fail(XM_EINVAL, "vl_nnconv(split): unknown flag bits 0x%x", flags);
  const SplitShape s = split_shape(H, W, C, N, FH, FW, FC, K, sy, sx, pt, pb, pl, pr, dy, dx, flags);
  if (!split_can(s, XM_FUSE_SIGMOID)) {
    const char *why = (FH != 1 || FW != 1) ? "a filter larger than 1 x 1"
                      : FC != C            ? "filter groups"
                      : (pt | pb | pl | pr) ? "padding"
                      : (flags & XM_FUSE_SIGMOID) ? "the sigmoid epilogue"
                                                  : "a tensor of 2^31 elements or more";
    return fail(XM_ENOTSUP, "vl_nnconv(split): the bf16x3 kernel is built for unpadded, ungrouped 1 x 1 layers; this call has %s", why);
  }
  if (residual) {
    if (res_sy < 1 || res_sx < 1 || res_H < 1 || res_W < 1 || g.Ho != (res_H - 1) / res_sy + 1 ||
        g.Wo != (res_W - 1) / res_sx + 1)
      return fail(XM_EINVAL, "vl_nnconv(split): a %d x %d residual sampled with stride [%d %d] does not give the %d x %d output",
                  res_H, res_W, res_sy, res_sx, g.Ho, g.Wo);
    if (!split_fits((long long)res_H * res_W * K * N))
      return fail(XM_ETOOBIG, "vl_nnconv(split): residual with >= 2^31 elements");
  }
  if (!x || !f || !y) return fail(XM_EINVAL, "vl_nnconv(split): NULL tensor");
  if ((scale == nullptr) != (shift == nullptr))
    return fail(XM_EINVAL, "vl_nnconv(split): scale and shift must be given together");
  const SplitLaunch l = split_launch(s);
  SplitArgs a;
  a.x = x, a.f = f, a.bias = b, a.scale = scale, a.shift = shift, a.gate = gate, a.resid = residual, a.y = y;
  a.C = C, a.K = K, a.H = H, a.HW = H * W, a.Ho = g.Ho, a.P = g.Ho * g.Wo, a.NP = g.Ho * g.Wo * N;
  a.sy = sy, a.sx = sx;
  a.rH = residual ? res_H : 0, a.rHW = residual ? res_H * res_W : 0, a.rsy = res_sy, a.rsx = res_sx;
  a.relu = (flags & XM_FUSE_RELU) ? 1 : 0, a.kTiles = l.k_tiles;
  hipStream_t st = (hipStream_t)stream;
  const double np = (double)a.NP;
  ProfScope ps(prof_key(kProfConvSplit), 2.0 * K * np * C, st,
               4.0 * ((double)H * W * C * N + (double)C * K + np * K * (residual ? 2 : 1)));
  hipLaunchKernelGGL(conv_split_kernel, dim3(l.blocks), dim3(kSplitThreads), 0, st, a);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

}  // extern "C"

// Elementwise operators, losses, optimiser update and the batch-provider arithmetic on gfx950.
// vl_nnrelu / vl_nnsigmoid / dagnn.Sum / mcnExtraLayers Scale+Axpy, vl_nnsoftmaxt,
// vl_nnsoftmaxceloss (emoVoxZoo.m:152), vl_nnloss (emoVoxZoo.m:149,160), the SGD-momentum step of
// cnn_train_dag (run_distillation.m:170-182), its 'solver' option and the device side of getBatchEmoVoxCeleb /
// getImageBatch.  All HBM- or latency-bound; float4 grid-stride loops, no atomics.
#include "norm_pool_plan.h"
#include "wav_resample.h"
#include "xm_common.h"

namespace xm {
extern unsigned long long g_param_version;   // conv.hip: prepared dgrad operands are valid for one version
}

namespace xm {

enum { OP_RELU_F, OP_RELU_B, OP_SIG_F, OP_SIG_B, OP_SUM, OP_SUM_RELU };

template <int OP>
__device__ __forceinline__ float ew_op(float a, float b, float leak) {
  if (OP == OP_RELU_F) return a > 0.f ? a : leak * a;
  if (OP == OP_RELU_B) return a > 0.f ? b : leak * b;  // a = x, b = dzdy
  if (OP == OP_SIG_F) return 1.f / (1.f + expf(-a));
  if (OP == OP_SIG_B) {
    float s = 1.f / (1.f + expf(-a));
    return b * s * (1.f - s);
  }
  if (OP == OP_SUM) return a + b;
  return fmaxf(a + b, 0.f);
}

template <int OP, bool BINARY>
__global__ void __launch_bounds__(256)
ew_kernel(const float *__restrict__ a, const float *__restrict__ b, float *__restrict__ y, size_t n,
          float leak, int vec) {
  size_t stride = (size_t)gridDim.x * 256;
  size_t i0 = blockIdx.x * (size_t)256 + threadIdx.x;
  if (vec) {
    size_t n4 = n >> 2;
    for (size_t i = i0; i < n4; i += stride) {
      float4 av = reinterpret_cast<const float4 *>(a)[i];
      float4 bv = BINARY ? reinterpret_cast<const float4 *>(b)[i] : make_float4(0, 0, 0, 0);
      float4 o;
      o.x = ew_op<OP>(av.x, bv.x, leak);
      o.y = ew_op<OP>(av.y, bv.y, leak);
      o.z = ew_op<OP>(av.z, bv.z, leak);
      o.w = ew_op<OP>(av.w, bv.w, leak);
      reinterpret_cast<float4 *>(y)[i] = o;
    }
    for (size_t i = (n4 << 2) + i0; i < n; i += stride)
      y[i] = ew_op<OP>(a[i], BINARY ? b[i] : 0.f, leak);
  } else {
    for (size_t i = i0; i < n; i += stride) y[i] = ew_op<OP>(a[i], BINARY ? b[i] : 0.f, leak);
  }
}

template <int OP, bool BINARY>
static int ew_launch(const float *a, const float *b, float *y, size_t n, float leak, hipStream_t st) {
  if (n == 0) return XM_OK;
  if (!a || !y || (BINARY && !b)) return fail(XM_EINVAL, "elementwise op: NULL tensor");
  int vec = aligned16(a, b, y) ? 1 : 0;
  hipLaunchKernelGGL((ew_kernel<OP, BINARY>), dim3(ew_grid(vec ? n / 4 + 1 : n)), dim3(256), 0, st, a,
                     b, y, n, leak, vec);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

// y(:,:,c,n) = a(c,n) * x(:,:,c,n) [+ r] [relu] : one block-row per plane chunk
__global__ void __launch_bounds__(256)
scale_axpy_kernel(const float *__restrict__ x, const float *__restrict__ a,
                  const float *__restrict__ r, float *__restrict__ y, FastDiv divHW, size_t total,
                  int relu) {
  size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < total; i += stride) {
    uint32_t plane = xm_div((uint32_t)i, divHW);
    float v = a[plane] * x[i] + (r ? r[i] : 0.f);
    if (relu) v = fmaxf(v, 0.f);
    y[i] = v;
  }
}

// ---- forward of the same tail without materialising the bnorm's output ------------------------------------------------
// x = g/sigma (u - mu) + b is consumed by exactly two readers, the squeeze and the excite, and the fused backward above
// never reads it: both readers recompute it from u with bn_apply_kernel's own expression (same bits), so the bnorm's
// apply pass (read u, write x) disappears.  One wave per plane for the squeeze (pool_global_kernel's summation order).
__global__ void __launch_bounds__(256)
se_squeeze_bn_kernel(const float *__restrict__ u, const float *__restrict__ g, const float *__restrict__ b,
                     const float *__restrict__ mom, int HW, int C, int planes, float *__restrict__ gp) {
  const int plane = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (plane >= planes) return;
  const int lane = threadIdx.x & 63, c = plane % C;
  const float *p = u + (size_t)plane * HW;
  const float sc = g[c] / mom[C + c], mu = mom[c], bb = b[c];
  float r = 0.f;
  if ((HW & 3) == 0 && (((uintptr_t)p) & 15) == 0) {
    const float4 *p4 = reinterpret_cast<const float4 *>(p);
#pragma unroll 4
    for (int i = lane; i < (HW >> 2); i += 64) {
      const float4 v = p4[i];
      r += ((sc * (v.x - mu) + bb) + (sc * (v.y - mu) + bb)) + ((sc * (v.z - mu) + bb) + (sc * (v.w - mu) + bb));
    }
  } else {
    for (int i = lane; i < HW; i += 64) r += sc * (p[i] - mu) + bb;
  }
  r = xm_wave_sum(r);
  if (lane == 0) gp[plane] = r / (float)HW;
}

// y = [relu](a .* bn(u) + r)
__global__ void __launch_bounds__(256)
scale_axpy_bn_kernel(const float *__restrict__ u, const float *__restrict__ a, const float *__restrict__ r,
                     const float *__restrict__ g, const float *__restrict__ b, const float *__restrict__ mom,
                     float *__restrict__ y, FastDiv divHW, int C, size_t total, int relu) {
  const size_t stride = (size_t)gridDim.x * 256;
  const bool vec = (divHW.d & 3) == 0 && ((((uintptr_t)u | (uintptr_t)r | (uintptr_t)y) & 15) == 0);
  if (vec) {
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < (total >> 2); i += stride) {
      const uint32_t plane = xm_div((uint32_t)(i << 2), divHW);
      const int c = plane % C;
      const float sc = g[c] / mom[C + c], mu = mom[c], bb = b[c], av = a[plane];
      const float4 v = reinterpret_cast<const float4 *>(u)[i];
      const float4 s = r ? reinterpret_cast<const float4 *>(r)[i] : float4{0.f, 0.f, 0.f, 0.f};
      float4 o;
      o.x = av * (sc * (v.x - mu) + bb) + s.x;
      o.y = av * (sc * (v.y - mu) + bb) + s.y;
      o.z = av * (sc * (v.z - mu) + bb) + s.z;
      o.w = av * (sc * (v.w - mu) + bb) + s.w;
      if (relu) o.x = fmaxf(o.x, 0.f), o.y = fmaxf(o.y, 0.f), o.z = fmaxf(o.z, 0.f), o.w = fmaxf(o.w, 0.f);
      reinterpret_cast<float4 *>(y)[i] = o;
    }
  } else {
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < total; i += stride) {
      const uint32_t plane = xm_div((uint32_t)i, divHW);
      const int c = plane % C;
      float v = a[plane] * (g[c] / mom[C + c] * (u[i] - mom[c]) + b[c]) + (r ? r[i] : 0.f);
      if (relu) v = fmaxf(v, 0.f);
      y[i] = v;
    }
  }
}

// ---- backward of the tail of an SE bottleneck block in TRAINING mode (teacher/ferplus_baselines.m:140-141, config 5) ----
//   u -> vl_nnbnorm -> x ;  gp = mean_hw(x) -> fc1 -> relu -> fc2 -> sigmoid = a ;  y = relu(a .* x + shortcut)
// The separate operators make 13 passes over block-sized tensors on the way back (relu mask 3, scale backward 3,
// squeeze backward at its fork 2, bnorm sums 2, bnorm apply 3).  Everything the gate's backward and the bnorm's sums
// need from those tensors are three numbers per (channel, sample) plane:
//   S0 = sum (u - mu),  S1 = sum dz,  S2 = sum dz (u - mu),      dz = [y > 0] dzdy
//   da = g/sigma S2 + b S1                                        (x is recomputed from u: the forward direction)
//   D  = a dz + dgp / (H W)   is the derivative that reaches x    (excite + squeeze), so per channel
//   sum D = sum_n (a S1 + dgp),   sum D (u - mu) = sum_n (a S2 + dgp / (H W) S0)
// se_tail_reduce_kernel (3 reads) leaves S0..S2 and da; after the gate's backward has produced dgp,
// se_tail_apply_kernel (3 reads, 2 writes) writes dz (the shortcut's derivative) and du = g/sigma (D - c1 - (u - mu) c2)
// with the bnorm's usual fp64 expression.  x itself is not read on the way back.
// one wave per plane (4 planes per block): planes have 49 ... 3136 elements
__global__ void __launch_bounds__(256)
se_tail_reduce_kernel(const float *__restrict__ y, const float *__restrict__ dzdy, const float *__restrict__ u,
                      const float *__restrict__ g, const float *__restrict__ b, const float *__restrict__ mom, int HW, int C,
                      int planes, float *__restrict__ da, double *__restrict__ S) {
  const int plane = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (plane >= planes) return;
  const int lane = threadIdx.x & 63, c = plane % C;
  const size_t off = (size_t)plane * HW;
  const double mu = (double)mom[c];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  // HW % 4 == 0 keeps every plane as aligned as its tensor's base
  if ((HW & 3) == 0 && ((((uintptr_t)y | (uintptr_t)dzdy | (uintptr_t)u) & 15) == 0)) {
    for (int i = lane * 4; i < HW; i += 256) {
      const float4 yv = *reinterpret_cast<const float4 *>(y + off + i), dv = *reinterpret_cast<const float4 *>(dzdy + off + i),
                   uv = *reinterpret_cast<const float4 *>(u + off + i);
      const double t0 = (double)uv.x - mu, t1 = (double)uv.y - mu, t2 = (double)uv.z - mu, t3 = (double)uv.w - mu;
      const double d0 = yv.x > 0.f ? (double)dv.x : 0.0, d1 = yv.y > 0.f ? (double)dv.y : 0.0,
                   d2 = yv.z > 0.f ? (double)dv.z : 0.0, d3 = yv.w > 0.f ? (double)dv.w : 0.0;
      s0 += (t0 + t1) + (t2 + t3);
      s1 += (d0 + d1) + (d2 + d3);
      s2 += (d0 * t0 + d1 * t1) + (d2 * t2 + d3 * t3);
    }
  } else {
    for (int i = lane; i < HW; i += 64) {
      const double t = (double)u[off + i] - mu, d = y[off + i] > 0.f ? (double)dzdy[off + i] : 0.0;
      s0 += t;
      s1 += d;
      s2 += d * t;
    }
  }
  s0 = xm_wave_sum_d(s0);
  s1 = xm_wave_sum_d(s1);
  s2 = xm_wave_sum_d(s2);
  if (lane == 0) {
    S[3 * (size_t)plane] = s0;
    S[3 * (size_t)plane + 1] = s1;
    S[3 * (size_t)plane + 2] = s2;
    da[plane] = (float)((double)g[c] / (double)mom[C + c] * s2 + (double)b[c] * s1);
  }
}

// one wave per channel: the bnorm's two sums over its N planes in fp64, dg / db
__global__ void __launch_bounds__(256)
se_tail_finalize_kernel(const double *__restrict__ S, const float *__restrict__ gate, const float *__restrict__ dgp,
                        const float *__restrict__ mom, int HW, int C, int N, double *__restrict__ sums,
                        float *__restrict__ dg, float *__restrict__ db) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= C) return;
  double sd = 0.0, sx = 0.0;
  for (int n = lane; n < N; n += 64) {
    const size_t p = (size_t)c + (size_t)C * n;
    const double a = (double)gate[p], k = (double)dgp[p] / (double)HW;
    sd += a * S[3 * p + 1] + (double)dgp[p];
    sx += a * S[3 * p + 2] + k * S[3 * p];
  }
  sd = xm_wave_sum_d(sd);
  sx = xm_wave_sum_d(sx);
  if (lane) return;
  sums[c] = sd;
  sums[C + c] = sx;
  if (dg) dg[c] = (float)(sx / (double)mom[C + c]);
  if (db) db[c] = (float)sd;
}

template <bool VEC>
__global__ void __launch_bounds__(256)
se_tail_apply_kernel(const float *__restrict__ y, const float *__restrict__ dzdy, const float *__restrict__ u,
                     const float *__restrict__ gate, const float *__restrict__ dgp, const float *__restrict__ g,
                     const float *__restrict__ mom, const double *__restrict__ sums, FastDiv divHW, int C, size_t total,
                     double m, int train, float *__restrict__ dz, float *__restrict__ du) {
  const size_t stride = (size_t)gridDim.x * 256;
  const size_t cnt = VEC ? (total >> 2) : total;
  const double ihw = 1.0 / (double)divHW.d;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < cnt; i += stride) {
    const uint32_t plane = xm_div((uint32_t)(VEC ? (i << 2) : i), divHW);
    const int c = plane % C;
    const double sg = mom[C + c], mu = mom[c];
    const double gs = (double)g[c] / sg;
    const double c1 = train ? sums[c] / m : 0.0;
    const double c2 = train ? sums[C + c] / (m * sg * sg) : 0.0;
    const float a = gate[plane];
    const double k = (double)dgp[plane] * ihw;
    if (VEC) {
      const float4 yv = reinterpret_cast<const float4 *>(y)[i], uv = reinterpret_cast<const float4 *>(u)[i];
      float4 dv = reinterpret_cast<const float4 *>(dzdy)[i];
      dv.x = yv.x > 0.f ? dv.x : 0.f;
      dv.y = yv.y > 0.f ? dv.y : 0.f;
      dv.z = yv.z > 0.f ? dv.z : 0.f;
      dv.w = yv.w > 0.f ? dv.w : 0.f;
      reinterpret_cast<float4 *>(dz)[i] = dv;
      float4 o;   // D = fl(a dz) + k: the excite's derivative is a float product (xm_scale_backward), the squeeze's share is added to it
      o.x = (float)(gs * (((double)(a * dv.x) + k) - c1 - ((double)uv.x - mu) * c2));
      o.y = (float)(gs * (((double)(a * dv.y) + k) - c1 - ((double)uv.y - mu) * c2));
      o.z = (float)(gs * (((double)(a * dv.z) + k) - c1 - ((double)uv.z - mu) * c2));
      o.w = (float)(gs * (((double)(a * dv.w) + k) - c1 - ((double)uv.w - mu) * c2));
      reinterpret_cast<float4 *>(du)[i] = o;
    } else {
      const float d = y[i] > 0.f ? dzdy[i] : 0.f;
      dz[i] = d;
      du[i] = (float)(gs * (((double)(a * d) + k) - c1 - ((double)u[i] - mu) * c2));
    }
  }
}

// one wave per plane: da = sum dy .* x ; dx = a .* dy
__global__ void __launch_bounds__(256)
scale_bwd_kernel(const float *__restrict__ x, const float *__restrict__ a,
                 const float *__restrict__ dy, float *__restrict__ dx, float *__restrict__ da, int HW,
                 int planes) {
  int plane = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (plane >= planes) return;
  int lane = threadIdx.x & 63;
  size_t off = (size_t)plane * HW;
  float av = a[plane], s = 0.f;
  for (int i = lane; i < HW; i += 64) {
    float d = dy[off + i];
    s += d * x[off + i];
    if (dx) dx[off + i] = av * d;
  }
  s = xm_wave_sum(s);
  if (lane == 0 && da) da[plane] = s;
}

// softmax(X/T) along channels; one thread per (i, n) column
__global__ void softmaxt_kernel(const float *__restrict__ x, float *__restrict__ y, int HW, int C,
                                int N, float T) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= HW * N) return;
  int i = idx % HW, n = idx / HW;
  const float *p = x + i + (size_t)HW * C * n;
  float *q = y + i + (size_t)HW * C * n;
  double mx = -INFINITY, s = 0;
  for (int c = 0; c < C; ++c) mx = fmax(mx, (double)p[(size_t)HW * c] / T);
  for (int c = 0; c < C; ++c) s += exp((double)p[(size_t)HW * c] / T - mx);
  for (int c = 0; c < C; ++c) q[(size_t)HW * c] = (float)(exp((double)p[(size_t)HW * c] / T - mx) / s);
}

__global__ void softmaxt_bwd_kernel(const float *__restrict__ x, const float *__restrict__ dzdy,
                                    float *__restrict__ dx, int HW, int C, int N, float T) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= HW * N) return;
  int i = idx % HW, n = idx / HW;
  const size_t base = i + (size_t)HW * C * n;
  const float *p = x + base, *d = dzdy + base;
  float *q = dx + base;
  double mx = -INFINITY, s = 0, dot = 0;
  for (int c = 0; c < C; ++c) mx = fmax(mx, (double)p[(size_t)HW * c] / T);
  for (int c = 0; c < C; ++c) s += exp((double)p[(size_t)HW * c] / T - mx);
  for (int c = 0; c < C; ++c) dot += (double)d[(size_t)HW * c] * (exp((double)p[(size_t)HW * c] / T - mx) / s);
  for (int c = 0; c < C; ++c) {
    double y = exp((double)p[(size_t)HW * c] / T - mx) / s;
    q[(size_t)HW * c] = (float)(y * ((double)d[(size_t)HW * c] - dot) / T);
  }
}

// block-wide deterministic sum of one double per thread (256 threads) -> thread 0
__device__ double block_sum_d(double v, double *red /*256*/) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

// single block; thread-per-sample loop.  Matches oracle/xm_oracle.c orc_nnsoftmaxceloss.
__global__ void __launch_bounds__(256)
softmaxceloss_kernel(const float *__restrict__ x, const float *__restrict__ p, int C, int N, float T,
                     int logit_targets, const float *__restrict__ w, const float *__restrict__ dzdy,
                     float *__restrict__ y) {
  __shared__ double red[256];
  double total = 0;
  for (int n = threadIdx.x; n < N; n += 256) {
    const float *xn = x + (size_t)C * n, *pn = p + (size_t)C * n;
    double pt[64], mx = -INFINITY, s = 0, psum = 0;
    if (logit_targets) {
      double mp = -INFINITY, sp = 0;
      for (int c = 0; c < C; ++c) mp = fmax(mp, (double)pn[c] / T);
      for (int c = 0; c < C; ++c) sp += exp((double)pn[c] / T - mp);
      for (int c = 0; c < C; ++c) pt[c] = exp((double)pn[c] / T - mp) / sp;
    } else {
      for (int c = 0; c < C; ++c) pt[c] = pn[c];
    }
    for (int c = 0; c < C; ++c) {
      mx = fmax(mx, (double)xn[c] / T);
      psum += pt[c];
    }
    for (int c = 0; c < C; ++c) s += exp((double)xn[c] / T - mx);
    double lse = mx + log(s);
    double wn = w ? (double)w[n] : 1.0;
    if (!dzdy) {
      double l = 0;
      for (int c = 0; c < C; ++c) l += pt[c] * (lse - (double)xn[c] / T);
      total += wn * l;
    } else {
      double dz = dzdy[0];
      for (int c = 0; c < C; ++c) {
        double q = exp((double)xn[c] / T - lse);
        y[(size_t)C * n + c] = (float)(dz * wn * (q * psum - pt[c]) / T);
      }
    }
  }
  if (!dzdy) {
    double t = block_sum_d(total, red);
    if (threadIdx.x == 0) y[0] = (float)t;
  }
}

// regression losses: forward = single block, fixed-order double sum; backward = elementwise
__global__ void __launch_bounds__(256)
regloss_kernel(const float *__restrict__ x, const float *__restrict__ t, int E, int N, int kind,
               float sigma, const float *__restrict__ w, const float *__restrict__ dzdy,
               float *__restrict__ y) {
  __shared__ double red[256];
  const double s2 = (double)sigma * sigma;
  const size_t total_e = (size_t)E * N;
  double total = 0;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < total_e; i += (size_t)gridDim.x * 256) {
    const int n = (int)(i / E);
    const double wn = w ? (double)w[n] : 1.0;
    const double d = (double)x[i] - (double)t[i];
    const double a = fabs(d);
    const bool lin = kind == 1 && a > 1.0 / s2;
    if (!dzdy) {
      total += wn * (kind == 0 ? 0.5 * d * d : (lin ? a - 0.5 / s2 : 0.5 * s2 * d * d));
    } else {
      const double g = kind == 0 ? d : (lin ? (d > 0 ? 1.0 : -1.0) : s2 * d);
      y[i] = (float)((double)dzdy[0] * wn * g);
    }
  }
  if (!dzdy) {
    double r = block_sum_d(total, red);
    if (threadIdx.x == 0) y[0] = (float)r;
  }
}

__global__ void __launch_bounds__(256)
nnloss_kernel(const float *__restrict__ x, const float *__restrict__ labels, int C, int N, int loss,
              const float *__restrict__ dzdy, float *__restrict__ y) {
  __shared__ double red[256];
  double total = 0;
  for (int n = threadIdx.x; n < N; n += 256) {
    const float *xn = x + (size_t)C * n;
    const int lab = (int)labels[n];
    if (lab < 1 || lab > C) {   // vl_nnloss skips label 0; every label outside 1..C is skipped alike (class_stats_kernel)
      if (dzdy)
        for (int c = 0; c < C; ++c) y[(size_t)C * n + c] = 0.f;
      continue;
    }
    const int c0 = lab - 1;
    double mx = -INFINITY, s = 0;
    int arg = 0;
    for (int c = 0; c < C; ++c)
      if ((double)xn[c] > mx) {
        mx = xn[c];
        arg = c;
      }
    for (int c = 0; c < C; ++c) s += exp((double)xn[c] - mx);
    if (loss == XM_LOSS_SOFTMAXLOG) {
      if (!dzdy)
        total += mx + log(s) - (double)xn[c0];
      else
        for (int c = 0; c < C; ++c)
          y[(size_t)C * n + c] =
              (float)((double)dzdy[0] * (exp((double)xn[c] - mx) / s - (c == c0 ? 1.0 : 0.0)));
    } else {
      if (!dzdy)
        total += (arg != c0) ? 1.0 : 0.0;
      else
        for (int c = 0; c < C; ++c) y[(size_t)C * n + c] = 0.f;
    }
  }
  if (!dzdy) {
    double t = block_sum_d(total, red);
    if (threadIdx.x == 0) y[0] = (float)t;
  }
}

__global__ void __launch_bounds__(256)
sgd_kernel(float *__restrict__ w, float *__restrict__ m, const float *__restrict__ der, size_t n,
           float lr, float mom, float wd, float inv_batch, int vec) {
  size_t stride = (size_t)gridDim.x * 256;
  size_t i0 = blockIdx.x * (size_t)256 + threadIdx.x;
  if (vec) {
    size_t n4 = n >> 2;
    for (size_t i = i0; i < n4; i += stride) {
      float4 wv = reinterpret_cast<float4 *>(w)[i], mv = reinterpret_cast<float4 *>(m)[i];
      float4 dv = reinterpret_cast<const float4 *>(der)[i];
      // written exactly as cnn_train_dag: m = mom*m - (wd*w + der/B); w = w + lr*m
      mv.x = mom * mv.x - (wd * wv.x + dv.x * inv_batch);
      mv.y = mom * mv.y - (wd * wv.y + dv.y * inv_batch);
      mv.z = mom * mv.z - (wd * wv.z + dv.z * inv_batch);
      mv.w = mom * mv.w - (wd * wv.w + dv.w * inv_batch);
      wv.x += lr * mv.x;
      wv.y += lr * mv.y;
      wv.z += lr * mv.z;
      wv.w += lr * mv.w;
      reinterpret_cast<float4 *>(m)[i] = mv;
      reinterpret_cast<float4 *>(w)[i] = wv;
    }
    for (size_t i = (n4 << 2) + i0; i < n; i += stride) {
      float mm = mom * m[i] - (wd * w[i] + der[i] * inv_batch);
      m[i] = mm;
      w[i] += lr * mm;
    }
  } else {
    for (size_t i = i0; i < n; i += stride) {
      float mm = mom * m[i] - (wd * w[i] + der[i] * inv_batch);
      m[i] = mm;
      w[i] += lr * mm;
    }
  }
}

// ---- cnn_train_dag's 'solver' option (MatConvNet +solver package [EXT]) and the nesterovUpdate arm of its default solver --
// One element of one update, in fp32, operation by operation in the order of the MATLAB source (xmodal.h has the formulas
// and the coef slots).  g = vl_taccum(1 / batchSize, parDer, thisDecay, value).  The scalar coefficients arrive rounded as
// MATLAB rounds them (a double expression such as 1 - beta2 is evaluated in double, then meets the single array).
struct SolverArgs {
  float lr, wd, inv_batch, c0, c1, c2, c3;
};

template <int KIND>
__device__ __forceinline__ void solver_step(float &w, float &s1, float &s2, float d, const SolverArgs &a) {
  const float g = d * a.inv_batch + a.wd * w;
  if (KIND == XM_SOLVER_ADAGRAD) {            // c0 = epsilon, c1 = rho
    s1 = s1 * a.c1 + g * g;
    w = w - a.lr * g / (sqrtf(s1) + a.c0);
  } else if (KIND == XM_SOLVER_RMSPROP) {     // c0 = epsilon, c1 = rho, c2 = 1 - rho
    s1 = s1 * a.c1 + g * g * a.c2;
    w = w - a.lr * g / (sqrtf(s1) + a.c0);
  } else if (KIND == XM_SOLVER_ADADELTA) {    // c0 = epsilon, c1 = rho, c2 = 1 - rho; s1 = g_sqr, s2 = delta_sqr
    s1 = s1 * a.c1 + g * g * a.c2;
    const float delta = -sqrtf((s2 + a.c0) / (s1 + a.c0)) * g;
    s2 = s2 * a.c1 + delta * delta * a.c2;
    w = w + a.lr * delta;
  } else if (KIND == XM_SOLVER_ADAM) {        // c0 = epsilon, c1 = 1 - beta1, c2 = 1 - beta2, c3 = lr_t; s1 = m, s2 = v
    s1 = s1 + a.c1 * (g - s1);
    s2 = s2 + a.c2 * (g * g - s2);
    w = w - a.c3 * s1 / (sqrtf(s2) + a.c0);
  } else {                                    // XM_SOLVER_NESTEROV: c0 = momentum; s1 = momentum state
    s1 = a.c0 * s1 - g;
    w = w + a.lr * (a.c0 * s1 - g);
  }
}

template <int KIND>
__global__ void __launch_bounds__(256)
solver_kernel(float *__restrict__ w, float *__restrict__ s1, float *__restrict__ s2, const float *__restrict__ der,
              size_t n, SolverArgs a, int vec) {
  constexpr bool TWO = KIND == XM_SOLVER_ADADELTA || KIND == XM_SOLVER_ADAM;   // one-state kinds never touch s2
  size_t stride = (size_t)gridDim.x * 256;
  size_t i0 = blockIdx.x * (size_t)256 + threadIdx.x;
  size_t tail = 0;
  if (vec) {
    size_t n4 = n >> 2;
    for (size_t i = i0; i < n4; i += stride) {
      float4 wv = reinterpret_cast<float4 *>(w)[i], av = reinterpret_cast<float4 *>(s1)[i];
      float4 bv = TWO ? reinterpret_cast<float4 *>(s2)[i] : make_float4(0, 0, 0, 0);
      float4 dv = reinterpret_cast<const float4 *>(der)[i];
      solver_step<KIND>(wv.x, av.x, bv.x, dv.x, a);
      solver_step<KIND>(wv.y, av.y, bv.y, dv.y, a);
      solver_step<KIND>(wv.z, av.z, bv.z, dv.z, a);
      solver_step<KIND>(wv.w, av.w, bv.w, dv.w, a);
      reinterpret_cast<float4 *>(s1)[i] = av;
      if (TWO) reinterpret_cast<float4 *>(s2)[i] = bv;
      reinterpret_cast<float4 *>(w)[i] = wv;
    }
    tail = n4 << 2;
  }
  for (size_t i = tail + i0; i < n; i += stride) {
    float ww = w[i], aa = s1[i], bb = TWO ? s2[i] : 0.f;
    solver_step<KIND>(ww, aa, bb, der[i], a);
    s1[i] = aa;
    if (TWO) s2[i] = bb;
    w[i] = ww;
  }
}

template <int KIND>
static void solver_launch(float *w, float *s1, float *s2, const float *der, size_t n, const SolverArgs &a,
                          hipStream_t st) {
  int vec = aligned16(w, s1, s2, der) ? 1 : 0;
  hipLaunchKernelGGL(solver_kernel<KIND>, dim3(ew_grid(vec ? n / 4 + 1 : n)), dim3(256), 0, st, w, s1, s2,
                     der, n, a, vec);
}

__global__ void scale_kernel(float *__restrict__ x, size_t n, float a) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < n) x[i] *= a;
}

// ---- vl_nndropout (emoVoxZoo.m:116-135,272-277: dagnn.DropOut behind fc6 / fc7 when opts.dropout > 0) -------------
// mask = (u >= rate) / (1 - rate), u ~ U[0, 1); Y = mask .* X.  MATLAB's generator stream cannot be reproduced, so the
// stream is our own and stateless: Philox4x32-10 keyed by `seed`, counter = (element index / 4 + offset): the same
// (seed, offset) gives the same mask on any launch geometry; a host advances `offset` by ceil(n / 4) per call.
__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0], p1 = (unsigned long long)0xCD9E8D57u * c[2];
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1,
                   n3 = (unsigned)p0;
    c[0] = n0, c[1] = n1, c[2] = n2, c[3] = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}
__global__ void __launch_bounds__(256)
dropout_fwd_kernel(const float *__restrict__ x, size_t n, float rate, float scale, unsigned long long seed,
                   unsigned long long offset, float *__restrict__ y, float *__restrict__ mask) {
  const size_t g = blockIdx.x * (size_t)256 + threadIdx.x;   // one counter = four elements
  if (4 * g >= n) return;
  const unsigned long long ctr = g + offset;
  unsigned c[4] = {(unsigned)ctr, (unsigned)(ctr >> 32), 0u, 0u};
  philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const size_t i = 4 * g + e;
    if (i >= n) break;
    const float u = (float)(c[e] >> 8) * (1.0f / 16777216.0f);   // 24 random bits: exact in fp32, in [0, 1)
    const float m = u >= rate ? scale : 0.f;
    if (mask) mask[i] = m;
    y[i] = m * x[i];
  }
}
__global__ void mul_kernel(const float *__restrict__ x, const float *__restrict__ m, size_t n, float *__restrict__ y) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < n) y[i] = m[i] * x[i];
}

__global__ void average_kernel(float *__restrict__ w, const float *__restrict__ der, size_t n,
                               float lr, float inv_workers) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < n) w[i] = (1.f - lr) * w[i] + lr * (der[i] * inv_workers);
}

// per-frequency-row normalisation: a block owns 64 consecutive rows h of one clip; its 4 waves split
// the time axis (w = wave, wave + 4, ...), lanes along h are contiguous in memory.  Partial sums meet
// in LDS in wave order (fixed -> deterministic); two passes (mean, then centred squares) as the
// reference's mean() / std() do.
__global__ void __launch_bounds__(256)
spec_rownorm_kernel(const float *__restrict__ s, float *__restrict__ o, int H, int W, int N) {
  __shared__ float red[4][64];
  const int hl = threadIdx.x & 63, wl = threadIdx.x >> 6;
  const int h = blockIdx.x * 64 + hl, n = blockIdx.y;
  const bool ok = h < H;
  const float *p = s + (ok ? h : 0) + (size_t)H * W * n;
  float *q = o + (ok ? h : 0) + (size_t)H * W * n;
  float sum = 0.f;
  for (int w = wl; w < W; w += 4) sum += p[(size_t)H * w];
  red[wl][hl] = sum;
  __syncthreads();
  const float mu = ((red[0][hl] + red[1][hl]) + (red[2][hl] + red[3][hl])) / (float)W;
  __syncthreads();
  float ss = 0.f;
  for (int w = wl; w < W; w += 4) {
    float d = p[(size_t)H * w] - mu;
    ss += d * d;
  }
  red[wl][hl] = ss;
  __syncthreads();
  const float inv = 1.f / sqrtf(((red[0][hl] + red[1][hl]) + (red[2][hl] + red[3][hl])) / (float)(W - 1));
  if (!ok) return;
  for (int w = wl; w < W; w += 4) q[(size_t)H * w] = (p[(size_t)H * w] - mu) * inv;
}

__global__ void aggregate_logits_kernel(const float *__restrict__ lg, int F, int E,
                                        const int *__restrict__ first, const int *__restrict__ last,
                                        int N, int agg, float *__restrict__ out,
                                        float *__restrict__ max_label) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  int f0 = first[n] - 1, f1 = min(last[n], F);
  // XM_AGG_PEAK (selectPeakLogit, run_cross_val.m:149-155): the row holding the block's largest entry, the first one in
  // column-major order as max(logits(:)) finds it -- lowest e, then lowest row
  int peak = f0;
  if (agg == XM_AGG_PEAK) {
    float top = -INFINITY;
    for (int e = 0; e < E; ++e)
      for (int fr = f0; fr < f1; ++fr) {
        float v = lg[fr + (size_t)F * e];
        if (v > top) {
          top = v;
          peak = fr;
        }
      }
  }
  float best = -INFINITY;
  int arg = 0;
  for (int e = 0; e < E; ++e) {
    float a;
    if (agg == XM_AGG_PEAK) {
      a = f1 > f0 ? lg[peak + (size_t)F * e] : -INFINITY;
    } else {
      a = agg == XM_AGG_MAX ? -INFINITY : 0.f;
      for (int fr = f0; fr < f1; ++fr) {
        float v = lg[fr + (size_t)F * e];
        a = agg == XM_AGG_MAX ? fmaxf(a, v) : a + v;
      }
      if (agg == XM_AGG_MEAN) a /= (float)(f1 - f0);
    }
    out[(size_t)E * n + e] = a;
    if (a > best) {
      best = a;
      arg = e;
    }
  }
  if (max_label) max_label[n] = (float)(arg + 1);
}

// [~, maxLabel] = max(lgo, [], 3)   (getBatchEmoVoxCeleb.m:32); x is 1 x 1 x C x N
__global__ void max_label_kernel(const float *__restrict__ x, int C, int N, float *__restrict__ lab) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float best = -INFINITY;
  int arg = 0;
  for (int c = 0; c < C; ++c) {
    float v = x[(size_t)C * n + c];
    if (v > best) {
      best = v;
      arg = c;
    }
  }
  lab[n] = (float)(arg + 1);
}

// lgo = aggregate(logits(rows of pair n)) ; lgo = lgo(:,:,1:P,:) ; [~, maxLabel] = max(lgo, [], 3)
// (getBatchEmoVoxCeleb.m:145-158,179-188,30-32) straight from the teacher's 1 x 1 x E x F output: no transposed copy.
// One lane per (pair, emotion): G = the power of two >= P lanes of a wave form a pair's group (G <= 64 = blockDim, so a
// group never straddles a wave), lane e walks the rows of emotion e in ascending order -- the summation order of
// aggregate_logits_kernel, whose arithmetic this repeats expression for expression -- and the label is a scan of the
// group's P values through __shfl in max_label_kernel's order.  Every lane reaches every __shfl; rows are clamped to
// [0, F), the mean still divides by the caller's row count as aggregate_logits_kernel does.
__global__ void __launch_bounds__(64)
window_targets_kernel(const float *__restrict__ lg, int E, int F, const int *__restrict__ first,
                      const int *__restrict__ last, int N, int agg, int P, int G, float *__restrict__ out,
                      float *__restrict__ max_label) {
  const int lane = threadIdx.x, e = lane % G, base = lane - e;
  const int n = blockIdx.x * (64 / G) + lane / G;
  const bool live = n < N && e < P;
  float a = -INFINITY;
  if (live) {
    const int f0 = first[n] - 1, f1 = min(last[n], F);
    a = agg == XM_AGG_MAX ? -INFINITY : 0.f;
    for (int fr = max(f0, 0); fr < f1; ++fr) {
      float v = lg[e + (size_t)E * fr];
      a = agg == XM_AGG_MAX ? fmaxf(a, v) : a + v;
    }
    if (agg == XM_AGG_MEAN) a /= (float)(f1 - f0);
    out[(size_t)P * n + e] = a;
  }
  float best = -INFINITY;
  int arg = 0;
  for (int c = 0; c < P; ++c) {
    float v = __shfl(a, base + c, 64);
    if (v > best) {
      best = v;
      arg = c;
    }
  }
  if (live && e == 0) max_label[n] = (float)(arg + 1);
}

// one block; per-class counts through LDS atomics -- the addends are 0/1, so the float sums are
// exact integers (< 2^24) whatever the order: deterministic
__global__ void __launch_bounds__(256)
class_stats_kernel(const float *__restrict__ x, const float *__restrict__ labels, int C, int N,
                   float *__restrict__ correct, float *__restrict__ population) {
  extern __shared__ float cnt[];  // [2][C]
  for (int i = threadIdx.x; i < 2 * C; i += 256) cnt[i] = 0.f;
  __syncthreads();
  for (int n = threadIdx.x; n < N; n += 256) {
    float best = -INFINITY;
    int arg = 0;
    for (int c = 0; c < C; ++c) {
      float v = x[(size_t)C * n + c];
      if (v > best) {
        best = v;
        arg = c;
      }
    }
    const int lab = (int)labels[n];
    if (lab >= 1 && lab <= C) {
      atomicAdd(&cnt[C + lab - 1], 1.f);
      if (arg + 1 == lab) atomicAdd(&cnt[lab - 1], 1.f);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < C; i += 256) {
    correct[i] += cnt[i];
    population[i] += cnt[C + i];
  }
}

__global__ void normalize_face_kernel(const float *__restrict__ rgb, float *__restrict__ out, int HW,
                                      int N, float a0, float a1, float a2) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= (size_t)HW * N) return;
  size_t n = i / HW, q = i % HW;
  const float *p = rgb + q + (size_t)HW * 3 * n;
  float gr = 0.2989f * p[0] + 0.5870f * p[HW] + 0.1140f * p[2 * (size_t)HW];
  gr = fminf(floorf(gr + 0.5f), 255.f);
  float *o = out + q + (size_t)HW * 3 * n;
  o[0] = gr - a0;
  o[HW] = gr - a1;
  o[2 * (size_t)HW] = gr - a2;
}

}  // namespace xm

using namespace xm;

extern "C" {

int xm_nnrelu(const float *x, size_t n, float leak, const float *dzdy, float *y, void *stream) {
  if (dzdy) return ew_launch<OP_RELU_B, true>(x, dzdy, y, n, leak, (hipStream_t)stream);
  return ew_launch<OP_RELU_F, false>(x, nullptr, y, n, leak, (hipStream_t)stream);
}

int xm_nnsigmoid(const float *x, size_t n, const float *dzdy, float *y, void *stream) {
  if (dzdy) return ew_launch<OP_SIG_B, true>(x, dzdy, y, n, 0.f, (hipStream_t)stream);
  return ew_launch<OP_SIG_F, false>(x, nullptr, y, n, 0.f, (hipStream_t)stream);
}

int xm_sum2(const float *a, const float *b, size_t n, int flags, float *y, void *stream) {
  if (flags & XM_FUSE_RELU) return ew_launch<OP_SUM_RELU, true>(a, b, y, n, 0.f, (hipStream_t)stream);
  return ew_launch<OP_SUM, true>(a, b, y, n, 0.f, (hipStream_t)stream);
}

int xm_scale_axpy(const float *x, int HW, int CN, const float *a, const float *r, int flags,
                  float *y, void *stream) {
  if (HW <= 0 || CN <= 0) return fail(XM_EINVAL, "scale: empty tensor");
  if (!x || !a || !y) return fail(XM_EINVAL, "scale: NULL tensor");
  if (too_big(HW, CN)) return fail(XM_ETOOBIG, "scale: tensor with >= 2^31 elements");
  size_t total = (size_t)HW * CN;
  hipLaunchKernelGGL(scale_axpy_kernel, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, x, a,
                     r, y, make_fastdiv((uint32_t)HW), total, (flags & XM_FUSE_RELU) ? 1 : 0);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_se_squeeze_bn(const float *u, int H, int W, int C, int N, const float *g, const float *b, const float *moments,
                     float *gp_out, void *stream) {
  if (H <= 0 || W <= 0 || C <= 0 || N <= 0) return fail(XM_EINVAL, "SE squeeze: empty tensor");
  if (too_big(H, W, C, N)) return fail(XM_ETOOBIG, "SE squeeze: tensor with >= 2^31 elements");
  if (!u || !g || !b || !moments || !gp_out) return fail(XM_EINVAL, "SE squeeze: NULL tensor");
  const int planes = C * N;
  hipLaunchKernelGGL(se_squeeze_bn_kernel, dim3((planes + 3) / 4), dim3(256), 0, (hipStream_t)stream, u, g, b, moments,
                     H * W, C, planes, gp_out);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_scale_axpy_bn(const float *u, int H, int W, int C, int N, const float *a, const float *r, const float *g,
                     const float *b, const float *moments, int flags, float *y, void *stream) {
  if (H <= 0 || W <= 0 || C <= 0 || N <= 0) return fail(XM_EINVAL, "scale: empty tensor");
  if (too_big(H, W, C, N)) return fail(XM_ETOOBIG, "scale: tensor with >= 2^31 elements");
  if (!u || !a || !g || !b || !moments || !y) return fail(XM_EINVAL, "scale: NULL tensor");
  const size_t total = (size_t)H * W * C * N;
  const unsigned grid = (unsigned)std::min<size_t>((total / 4 + 255) / 256 + 1, (size_t)256 * 64);
  hipLaunchKernelGGL(scale_axpy_bn_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, u, a, r, g, b, moments, y,
                     make_fastdiv((uint32_t)(H * W)), C, total, (flags & XM_FUSE_RELU) ? 1 : 0);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_se_tail_backward_reduce(const float *y, const float *dzdy, const float *u, int H, int W, int C, int N,
                               const float *g, const float *b, const float *moments, float *da_out, double *plane_sums,
                               void *stream) {
  if (H <= 0 || W <= 0 || C <= 0 || N <= 0) return fail(XM_EINVAL, "SE tail backward: empty tensor");
  if (too_big(H, W, C, N)) return fail(XM_ETOOBIG, "SE tail backward: tensor with >= 2^31 elements");
  if (!y || !dzdy || !u || !g || !b || !moments || !da_out || !plane_sums) return fail(XM_EINVAL, "SE tail backward: NULL tensor");
  const int planes = C * N;
  hipLaunchKernelGGL(se_tail_reduce_kernel, dim3((planes + 3) / 4), dim3(256), 0, (hipStream_t)stream, y, dzdy, u, g, b,
                     moments, H * W, C, planes, da_out, plane_sums);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_se_tail_backward_apply(const float *y, const float *dzdy, const float *u, int H, int W, int C, int N,
                              const float *gate, const float *dgp, const float *g, const float *moments, int train,
                              const double *plane_sums, float *dz_out, float *du_out, float *dg_out, float *db_out,
                              void *stream) {
  if (H <= 0 || W <= 0 || C <= 0 || N <= 0) return fail(XM_EINVAL, "SE tail backward: empty tensor");
  if (too_big(H, W, C, N)) return fail(XM_ETOOBIG, "SE tail backward: tensor with >= 2^31 elements");
  if (!y || !dzdy || !u || !gate || !dgp || !g || !moments || !plane_sums || !dz_out || !du_out)
    return fail(XM_EINVAL, "SE tail backward: NULL tensor");
  hipStream_t st = (hipStream_t)stream;
  WsCarver ws;
  int rc = ws.init(WsCarver::need((size_t)2 * C, 8), st);
  if (rc) return rc;
  double *sums = ws.take<double>((size_t)2 * C);
  const int HW = H * W;
  hipLaunchKernelGGL(se_tail_finalize_kernel, dim3((C + 3) / 4), dim3(256), 0, st, plane_sums, gate, dgp, moments, HW, C, N,
                     sums, dg_out, db_out);
  XM_LAUNCH_CHECK();
  const size_t total = (size_t)HW * C * N;
  const double m = (double)HW * N;
  const bool vec = (HW & 3) == 0 && aligned16(y, dzdy, u, dz_out, du_out);
  const size_t items = vec ? total / 4 : total;
  const unsigned grid = (unsigned)std::min<size_t>((items + 255) / 256, (size_t)256 * 64);
  if (vec)
    hipLaunchKernelGGL(se_tail_apply_kernel<true>, dim3(grid), dim3(256), 0, st, y, dzdy, u, gate, dgp, g, moments, sums,
                       make_fastdiv((uint32_t)HW), C, total, m, train, dz_out, du_out);
  else
    hipLaunchKernelGGL(se_tail_apply_kernel<false>, dim3(grid), dim3(256), 0, st, y, dzdy, u, gate, dgp, g, moments, sums,
                       make_fastdiv((uint32_t)HW), C, total, m, train, dz_out, du_out);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_scale_backward(const float *x, int HW, int CN, const float *a, const float *dzdy,
                      float *dx_out, float *da_out, void *stream) {
  if (HW <= 0 || CN <= 0) return fail(XM_EINVAL, "scale: empty tensor");
  if (!x || !a || !dzdy) return fail(XM_EINVAL, "scale: NULL tensor");
  hipLaunchKernelGGL(scale_bwd_kernel, dim3((CN + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, a,
                     dzdy, dx_out, da_out, HW, CN);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_nnsoftmaxt(const float *x, int HW, int C, int N, float temperature, float *y, void *stream) {
  if (HW <= 0 || C <= 0 || N <= 0) return fail(XM_EINVAL, "vl_nnsoftmaxt: empty tensor");
  if (!(temperature > 0.f)) return fail(XM_EINVAL, "vl_nnsoftmaxt: temperature must be > 0");
  int cols = HW * N;
  hipLaunchKernelGGL(softmaxt_kernel, dim3((cols + 127) / 128), dim3(128), 0, (hipStream_t)stream, x, y,
                     HW, C, N, temperature);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_nnsoftmaxt_backward(const float *x, const float *dzdy, int HW, int C, int N, float temperature,
                           float *dx, void *stream) {
  if (HW <= 0 || C <= 0 || N <= 0) return fail(XM_EINVAL, "vl_nnsoftmaxt: empty tensor");
  if (!x || !dzdy || !dx) return fail(XM_EINVAL, "vl_nnsoftmaxt: NULL tensor");
  if (!(temperature > 0.f)) return fail(XM_EINVAL, "vl_nnsoftmaxt: temperature must be > 0");
  int cols = HW * N;
  hipLaunchKernelGGL(softmaxt_bwd_kernel, dim3((cols + 127) / 128), dim3(128), 0, (hipStream_t)stream, x,
                     dzdy, dx, HW, C, N, temperature);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_nnsoftmaxceloss(const float *x, const float *p, int C, int N, float temperature,
                       int logit_targets, const float *instance_weights, const float *dzdy,
                       float *y, void *stream) {
  if (C <= 0 || N <= 0) return fail(XM_EINVAL, "vl_nnsoftmaxceloss: empty tensor");
  if (C > 64) return fail(XM_ENOTSUP, "vl_nnsoftmaxceloss: more than 64 classes (%d)", C);
  if (!(temperature > 0.f)) return fail(XM_EINVAL, "vl_nnsoftmaxceloss: temperature must be > 0");
  if (!x || !p || !y) return fail(XM_EINVAL, "vl_nnsoftmaxceloss: NULL tensor");
  hipLaunchKernelGGL(softmaxceloss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, x, p, C, N,
                     temperature, logit_targets, instance_weights, dzdy, y);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_nnregloss(const float *x, const float *t, int E, int N, int kind, float sigma,
                 const float *instance_weights, const float *dzdy, float *y, void *stream) {
  if (E <= 0 || N <= 0) return fail(XM_EINVAL, "regression loss: empty tensor");
  if (too_big(E, N)) return fail(XM_ETOOBIG, "regression loss: tensor too large");
  if (kind != XM_REGLOSS_EUCLIDEAN && kind != XM_REGLOSS_HUBER)
    return fail(XM_ENOTSUP, "regression loss: kind %d not built (euclidean, huber)", kind);
  if (kind == XM_REGLOSS_HUBER && !(sigma > 0.f)) return fail(XM_EINVAL, "vl_nnhuberloss: sigma must be > 0");
  if (!x || !t || !y) return fail(XM_EINVAL, "regression loss: NULL tensor");
  // forward: one block (deterministic sum); backward: elementwise over a grid
  size_t n = (size_t)E * N;
  size_t nb = (n + 255) / 256;
  unsigned grid = dzdy ? (unsigned)(nb < 4096 ? nb : 4096) : 1u;
  hipLaunchKernelGGL(regloss_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, t, E, N, kind,
                     sigma, instance_weights, dzdy, y);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_nnloss(const float *x, const float *labels, int C, int N, int loss, const float *dzdy,
              float *y, void *stream) {
  if (C <= 0 || N <= 0) return fail(XM_EINVAL, "vl_nnloss: empty tensor");
  if (loss != XM_LOSS_SOFTMAXLOG && loss != XM_LOSS_CLASSERROR)
    return fail(XM_ENOTSUP, "vl_nnloss: loss type %d not built (softmaxlog, classerror only)", loss);
  if (!x || !labels || !y) return fail(XM_EINVAL, "vl_nnloss: NULL tensor");
  hipLaunchKernelGGL(nnloss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, x, labels, C, N, loss,
                     dzdy, y);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_sgd_update(float *w, float *m, const float *der, size_t n, float lr, float momentum,
                  float weight_decay, float batch, void *stream) {
  ++xm::g_param_version;
  if (n == 0) return XM_OK;
  if (!w || !m || !der) return fail(XM_EINVAL, "sgd: NULL tensor");
  if (!(batch > 0.f)) return fail(XM_EINVAL, "sgd: batch must be > 0");
  int vec = aligned16(w, m, der) ? 1 : 0;
  hipLaunchKernelGGL(sgd_kernel, dim3(ew_grid(vec ? n / 4 + 1 : n)), dim3(256), 0, (hipStream_t)stream,
                     w, m, der, n, lr, momentum, weight_decay, 1.0f / batch, vec);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_solver_update(int kind, float *w, float *s1, float *s2, const float *der, size_t n, float lr,
                     float weight_decay, float batch, const float *coef, void *stream) {
  static const char *const names[] = {"adagrad", "rmsprop", "adadelta", "adam", "nesterov"};
  if (kind < XM_SOLVER_ADAGRAD || kind > XM_SOLVER_NESTEROV)
    return fail(XM_EINVAL, "solver: unknown kind %d (0 adagrad, 1 rmsprop, 2 adadelta, 3 adam, 4 nesterov)", kind);
  if (!(batch > 0.f)) return fail(XM_EINVAL, "solver %s: batch must be > 0", names[kind]);
  if (!coef) return fail(XM_EINVAL, "solver %s: NULL coefficient array", names[kind]);
  const bool two = kind == XM_SOLVER_ADADELTA || kind == XM_SOLVER_ADAM;
  if (n > 0 && (!w || !der || !s1)) return fail(XM_EINVAL, "solver %s: NULL tensor (w, der or state 1)", names[kind]);
  if (n > 0 && two && !s2) return fail(XM_EINVAL, "solver %s: needs a second state buffer, s2 is NULL", names[kind]);
  ++xm::g_param_version;
  if (n == 0) return XM_OK;
  const xm::SolverArgs a = {lr, weight_decay, 1.0f / batch, coef[0], coef[1], coef[2], coef[3]};
  hipStream_t st = (hipStream_t)stream;
  switch (kind) {
    case XM_SOLVER_ADAGRAD: solver_launch<XM_SOLVER_ADAGRAD>(w, s1, s2, der, n, a, st); break;
    case XM_SOLVER_RMSPROP: solver_launch<XM_SOLVER_RMSPROP>(w, s1, s2, der, n, a, st); break;
    case XM_SOLVER_ADADELTA: solver_launch<XM_SOLVER_ADADELTA>(w, s1, s2, der, n, a, st); break;
    case XM_SOLVER_ADAM: solver_launch<XM_SOLVER_ADAM>(w, s1, s2, der, n, a, st); break;
    default: solver_launch<XM_SOLVER_NESTEROV>(w, s1, s2, der, n, a, st); break;
  }
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_scale_f32(float *x, size_t n, float a, void *stream) {
  if (n == 0) return XM_OK;
  if (!x) return fail(XM_EINVAL, "scale: NULL tensor");
  hipLaunchKernelGGL(scale_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, n, a);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_nndropout_forward(const float *x, size_t n, float rate, unsigned long long seed, unsigned long long offset,
                         float *y, float *mask_out, void *stream) {
  if (n == 0) return XM_OK;
  if (!x || !y) return fail(XM_EINVAL, "vl_nndropout: NULL tensor");
  if (!(rate >= 0.f && rate < 1.f)) return fail(XM_EINVAL, "vl_nndropout: rate must be in [0, 1)");
  const size_t groups = (n + 3) / 4;
  hipLaunchKernelGGL(dropout_fwd_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, n,
                     rate, 1.f / (1.f - rate), seed, offset, y, mask_out);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_nndropout_apply(const float *x, const float *mask, size_t n, float *y, void *stream) {
  if (n == 0) return XM_OK;
  if (!x || !mask || !y) return fail(XM_EINVAL, "vl_nndropout: NULL tensor");
  hipLaunchKernelGGL(mul_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, mask, n, y);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_average_update(float *w, const float *der, size_t n, float lr, float nworkers, void *stream) {
  ++xm::g_param_version;
  if (n == 0) return XM_OK;
  if (!w || !der) return fail(XM_EINVAL, "average update: NULL tensor");
  hipLaunchKernelGGL(average_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, w, der, n, lr, 1.0f / nworkers);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

// out(b, j, n) = |reim(j, b, n) + i reim(j, B + b, n)|; a 32 x 32 LDS tile transposes (j, b) so
// that both the reads (j contiguous) and the writes (b contiguous) are coalesced
__global__ void __launch_bounds__(256)
spec_magnitude_kernel(const float *__restrict__ reim, float *__restrict__ out, int Wo, int B, int N) {
  __shared__ float tile[32][33];
  const int n = blockIdx.z, j0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const float *src = reim + (size_t)Wo * 2 * B * n;
  for (int r = ty; r < 32; r += 8) {
    int b = b0 + r, j = j0 + tx;
    float v = 0.f;
    if (b < B && j < Wo) {
      float re = src[j + (size_t)Wo * b], im = src[j + (size_t)Wo * (B + b)];
      v = sqrtf(re * re + im * im);
    }
    tile[r][tx] = v;
  }
  __syncthreads();
  float *dst = out + (size_t)B * Wo * n;
  for (int r = ty; r < 32; r += 8) {
    int j = j0 + r, b = b0 + tx;
    if (b < B && j < Wo) dst[b + (size_t)B * j] = tile[tx][r];
  }
}

int xm_spec_magnitude(const float *reim, int Wo, int B, int N, float *out, void *stream) {
  if (Wo <= 0 || B <= 0 || N <= 0) return fail(XM_EINVAL, "spec_magnitude: empty input");
  if (N > 65535) return fail(XM_ETOOBIG, "spec_magnitude: more than 65535 clips per call");
  if (too_big(Wo, 2 * B, N)) return fail(XM_ETOOBIG, "spec_magnitude: tensor too large");
  if (!reim || !out) return fail(XM_EINVAL, "spec_magnitude: NULL tensor");
  hipLaunchKernelGGL(spec_magnitude_kernel, dim3((Wo + 31) / 32, (B + 31) / 32, N), dim3(256), 0,
                     (hipStream_t)stream, reim, out, Wo, B, N);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

// ---- resample (chspeed branch of the batch provider, getBatchEmoVoxCeleb.m:102-108) --------------------------------
// y[j] = sum_k h[(j + delay) q - k p] x[k]: the polyphase form of upfirdn(x, h, p, q) with the filter delay removed
// (MATLAB resample [EXT Signal Processing Toolbox]); ~2 * 10 + 1 taps per output, one thread per output sample.
__global__ void __launch_bounds__(256)
resample_kernel(const float *__restrict__ x, int Lx, const float *__restrict__ h, int Lh, int p, int q, int delay,
                float *__restrict__ y, int Ly) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= Ly) return;
  const long long t0 = (long long)(j + delay) * q;
  // k with 0 <= t0 - k p < Lh and 0 <= k < Lx
  long long klo = (t0 - (Lh - 1) + p - 1) / p;
  if (t0 - (Lh - 1) < 0) klo = 0;
  long long khi = t0 / p;
  if (khi > Lx - 1) khi = Lx - 1;
  float acc = 0.f;
  for (long long k = klo; k <= khi; ++k) acc = fmaf(h[t0 - k * p], x[k], acc);
  y[j] = acc;
}

int xm_resample(const float *x, int Lx, const float *h, int Lh, int p, int q, int delay, float *y, int Ly, void *stream) {
  if (Lx <= 0 || Lh <= 0 || p <= 0 || q <= 0 || delay < 0 || Ly < 0) return fail(XM_EINVAL, "resample: bad sizes");
  if (Ly == 0) return XM_OK;
  if (!x || !h || !y) return fail(XM_EINVAL, "resample: NULL tensor");
  hipLaunchKernelGGL(resample_kernel, dim3((Ly + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, Lx, h, Lh, p, q, delay,
                     y, Ly);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

// ---- wav_batch: crop | resample, zero padding and noise mix of a whole batch (getBatchEmoVoxCeleb.m:102-135) --------
// The filter of resample(x, p, q) is never stored: with P = max(p, q), half = 10 P and the delay removed, output j is
//   y[j] = g sum_k u(j q - k p) x[k],  |j q - k p| <= half,  u(m) = sinc(m / P) I0(beta sqrt(1 - (m / half)^2)),
// g = p / sum_m u(m) (the constant 1 / (P I0(beta)) of the toolbox's taps cancels in p h / sum(h)).  sin(pi m / P)
// comes from r = m mod P and the parity of floor(m / P), both carried along the tap loop in integers (m moves by p per
// tap), so the argument of the sine is exact at every |m|; I0(beta sqrt(s)) is its power series in beta^2 s / 4, which
// needs no square root.  wav_gain_kernel (one workgroup per clip) reduces p, q by their gcd and sums u in fp64;
// wav_batch_kernel is one thread per output sample.  WavClip, the taps and the gain reduction are wav_resample.h, which
// wav.hip shares.
__global__ void __launch_bounds__(1024)
wav_gain_kernel(const long long *__restrict__ desc, WavClip *__restrict__ clip) {
  const int n = blockIdx.x;
  wav_gain_block(desc[6 * (size_t)n + 2], desc[6 * (size_t)n + 3], clip, n);
}

__global__ void __launch_bounds__(256)
wav_batch_kernel(const float *__restrict__ wav, long long wav_len, const float *__restrict__ noise, long long noise_len,
                 const long long *__restrict__ desc, const float *__restrict__ ratio, const WavClip *__restrict__ clip,
                 float *__restrict__ z, int L) {
  const int n = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= L) return;
  const long long *d = desc + 6 * (size_t)n;
  const long long src = d[0], nsrc = d[4], nlen = d[5];
  long long len = d[1];
  float v = 0.f;
  if (len > 0 && d[2] == d[3]) {                                   // crop, zero padded behind len (.m:109-119)
    const unsigned long long i = (unsigned long long)src + (unsigned long long)j;
    if (j < len && i < (unsigned long long)wav_len) v = wav[i];
  } else if (len > 0) {
    const WavClip c = clip[n];
    if (len > (1LL << 31)) len = 1LL << 31;
    // k such that src + k is a sample of the bank: every read below is inside [0, wav_len)
    long long lo = 0, hi = len - 1;
    if (src < -(1LL << 32)) {
      hi = -1;
    } else {
      if (src < 0) lo = -src;
      if (hi > wav_len - 1 - src) hi = wav_len - 1 - src;
    }
    if (c.p > 0 && (long long)j * c.q < len * c.p) {               // j < ceil(len p / q)
      const int P = c.p > c.q ? c.p : c.q, half = 10 * P;
      const unsigned long long top = (unsigned long long)j * (unsigned)c.q + (unsigned)half;
      const long long khi = (long long)(top / (unsigned)c.p);      // largest k with j q - k p >= -half
      const int rem = (int)(top - (unsigned long long)khi * (unsigned)c.p);
      const long long klo = khi - (2 * half - rem) / c.p;          // smallest k with j q - k p <= half
      const long long k1 = khi < hi ? khi : hi, k0 = klo > lo ? klo : lo;
      if (k1 >= k0) {
        int m = rem - half + (int)((khi - k1) * c.p);              // j q - k1 p
        const int qd = (m + half) / P;                             // floor(m / P) + 10
        int r = m + half - qd * P, odd = qd & 1;
        const float invP = 1.f / (float)P, P_over_pi = (float)P * 0.318309886f,
                    kb = kWavBeta2Over4 / ((float)half * (float)half);
        float acc = 0.f;
        for (long long k = k1; k >= k0; --k) {
          acc = fmaf(wav_tap(m, r, odd, P, invP, P_over_pi, half, kb), wav[src + k], acc);
          m += c.p;
          r += c.p;
          if (r >= P) {
            r -= P;
            odd ^= 1;
          }
        }
        v = acc * c.gain;
      }
    }
  }
  if (j < nlen) {                                                  // z + y .* Nratio (.m:123-135)
    const unsigned long long i = (unsigned long long)nsrc + (unsigned long long)j;
    if (i < (unsigned long long)noise_len) v = fmaf(ratio[n], noise[i], v);
  }
  z[(size_t)n * L + j] = v;
}

int xm_wav_batch(const float *wav, long long wav_len, const float *noise, long long noise_len, const long long *desc,
                 const float *ratio, int N, float *z, int L, void *stream) {
  if (N < 0 || L <= 0 || wav_len < 0 || noise_len < 0) return fail(XM_EINVAL, "wav_batch: bad sizes");
  if (N == 0) return XM_OK;
  if (!wav || !desc || !ratio || !z || (!noise && noise_len > 0)) return fail(XM_EINVAL, "wav_batch: NULL tensor");
  if (N > 65535) return fail(XM_ETOOBIG, "wav_batch: more than 65535 clips per call");
  void *ws = nullptr;
  int rc = ws_get((size_t)N * sizeof(WavClip), &ws, (hipStream_t)stream);
  if (rc != XM_OK) return rc;
  hipLaunchKernelGGL(wav_gain_kernel, dim3(N), dim3(1024), 0, (hipStream_t)stream, desc, (WavClip *)ws);
  XM_LAUNCH_CHECK();
  hipLaunchKernelGGL(wav_batch_kernel, dim3((L + 255) / 256, N), dim3(256), 0, (hipStream_t)stream, wav, wav_len, noise,
                     noise_len, desc, ratio, (const WavClip *)ws, z, L);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_spec_rownorm(const float *spec, int H, int W, int N, float *out, void *stream) {
  if (H <= 0 || W <= 1 || N <= 0) return fail(XM_EINVAL, "spec_rownorm: need H>0, W>1, N>0");
  if (!spec || !out) return fail(XM_EINVAL, "spec_rownorm: NULL tensor");
  if (N > 65535) return fail(XM_ETOOBIG, "spec_rownorm: more than 65535 clips per call");
  hipLaunchKernelGGL(spec_rownorm_kernel, dim3((H + 63) / 64, N), dim3(256), 0, (hipStream_t)stream,
                     spec, out, H, W, N);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_aggregate_logits(const float *frame_logits, int F_total, int E, const int *first,
                        const int *last, int N, int agg, float *out, float *max_label,
                        void *stream) {
  if (F_total <= 0 || E <= 0 || N <= 0) return fail(XM_EINVAL, "aggregate_logits: empty input");
  if (agg != XM_AGG_MAX && agg != XM_AGG_MEAN && agg != XM_AGG_PEAK)
    return fail(XM_EINVAL, "unrecognised aggregator %d", agg);
  hipLaunchKernelGGL(aggregate_logits_kernel, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                     frame_logits, F_total, E, first, last, N, agg, out, max_label);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_max_label(const float *x, int C, int N, float *labels, void *stream) {
  if (C <= 0 || N <= 0) return fail(XM_EINVAL, "max_label: empty input");
  if (!x || !labels) return fail(XM_EINVAL, "max_label: NULL tensor");
  hipLaunchKernelGGL(max_label_kernel, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, x, C, N,
                     labels);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_window_targets(const float *logits, int E, int n, const int *first, const int *last, int N, int agg, int P,
                      float *out, float *max_label, void *stream) {
  if (E < 1 || E > 64) return fail(XM_EINVAL, "window_targets: E = %d, need 1 .. 64", E);
  if (P < 1 || P > E) return fail(XM_EINVAL, "window_targets: numPredEmotions = %d, need 1 .. E = %d", P, E);
  if (n < 0 || N < 0) return fail(XM_EINVAL, "window_targets: negative n or N");
  if (agg != XM_AGG_MAX && agg != XM_AGG_MEAN) return fail(XM_EINVAL, "window_targets: unrecognised aggregator %d", agg);
  if (N == 0) return XM_OK;
  if (!first || !last || !out || !max_label || (n > 0 && !logits)) return fail(XM_EINVAL, "window_targets: NULL tensor");
  int G = 1;
  while (G < P) G *= 2;
  const int per = 64 / G;
  hipLaunchKernelGGL(window_targets_kernel, dim3((N + per - 1) / per), dim3(64), 0, (hipStream_t)stream, logits, E, n,
                     first, last, N, agg, P, G, out, max_label);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_class_stats(const float *x, const float *labels, int C, int N, float *correct,
                   float *population, void *stream) {
  if (C <= 0 || N <= 0) return fail(XM_EINVAL, "class_stats: empty input");
  if (C > 4096) return fail(XM_ETOOBIG, "class_stats: more than 4096 classes");
  if (!x || !labels || !correct || !population) return fail(XM_EINVAL, "class_stats: NULL tensor");
  hipLaunchKernelGGL(class_stats_kernel, dim3(1), dim3(256), sizeof(float) * 2 * C, (hipStream_t)stream,
                     x, labels, C, N, correct, population);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

__device__ __forceinline__ float bilin_u8(const float *__restrict__ p, int H, int W, double y, double x) {
  y = fmin(fmax(y, 0.0), (double)(H - 1));
  x = fmin(fmax(x, 0.0), (double)(W - 1));
  int y0 = (int)floor(y), x0 = (int)floor(x);
  int y1 = y0 + 1 < H ? y0 + 1 : y0, x1 = x0 + 1 < W ? x0 + 1 : x0;
  double fy = y - y0, fx = x - x0;
  double v = (1 - fy) * ((1 - fx) * p[y0 + (size_t)H * x0] + fx * p[y0 + (size_t)H * x1]) +
             fy * ((1 - fx) * p[y1 + (size_t)H * x0] + fx * p[y1 + (size_t)H * x1]);
  v = floor(v + 0.5);
  return (float)fmin(fmax(v, 0.0), 255.0);
}

// coordinates in double: the oracle's arithmetic, so the uint8 rounding lands on the same side
__global__ void crop_resize_face_kernel(const float *__restrict__ src, float *__restrict__ out, int Hin,
                                        int Win, int N, double ch, double cw, double h0, double w0, int Ho,
                                        int Wo, float a0, float a1, float a2) {
  size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  const size_t HWo = (size_t)Ho * Wo;
  if (idx >= HWo * N) return;
  int n = (int)(idx / HWo);
  size_t q = idx - (size_t)n * HWo;
  int j = (int)(q / Ho), i = (int)(q - (size_t)j * Ho);
  double y = (i + 0.5) * ch / Ho - 0.5 + h0, x = (j + 0.5) * cw / Wo - 0.5 + w0;
  const size_t HWi = (size_t)Hin * Win;
  const float *p = src + HWi * 3 * n;
  float r = bilin_u8(p, Hin, Win, y, x), g = bilin_u8(p + HWi, Hin, Win, y, x),
        b = bilin_u8(p + 2 * HWi, Hin, Win, y, x);
  float gr = fminf(floorf(0.2989f * r + 0.5870f * g + 0.1140f * b + 0.5f), 255.f);
  float *o = out + q + HWo * 3 * n;
  o[0] = gr - a0;
  o[HWo] = gr - a1;
  o[2 * HWo] = gr - a2;
}

int xm_crop_resize_face(const float *src, int Hin, int Win, int N, float crop, int Ho, int Wo,
                        const float *avg3, float *out, void *stream) {
  if (Hin <= 0 || Win <= 0 || N <= 0 || Ho <= 0 || Wo <= 0) return fail(XM_EINVAL, "crop_resize_face: empty input");
  if (!(crop > 0.f) || crop > 1.f) return fail(XM_EINVAL, "crop_resize_face: crop must be in (0, 1]");
  if (!src || !avg3 || !out) return fail(XM_EINVAL, "crop_resize_face: NULL tensor");
  if (too_big(Hin, Win, 3, N) || too_big(Ho, Wo, 3, N)) return fail(XM_ETOOBIG, "crop_resize_face: tensor too large");
  const double ch = (double)crop * Hin, cw = (double)crop * Win;
  size_t n = (size_t)Ho * Wo * N;
  hipLaunchKernelGGL(crop_resize_face_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, src, out, Hin, Win, N, ch, cw, 0.5 * (Hin - ch), 0.5 * (Win - cw), Ho,
                     Wo, avg3[0], avg3[1], avg3[2]);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

}  // extern "C"

namespace xm {

// bilin_u8 with the fused multiply-adds hipcc forms for it inside crop_resize_face_kernel written out, so that another
// kernel gets the same roundings whatever its surroundings make the compiler prefer (a sample that lands on k + 0.5
// rounds by the last bit of these products):  top = fma(fx, p01, (1 - fx) p00), bot likewise, v = fma(fy, bot, (1 - fy) top)
__device__ __forceinline__ float bilin_u8_pinned(const float *__restrict__ p, int H, int W, double y, double x) {
#pragma clang fp contract(off)
  y = fmin(fmax(y, 0.0), (double)(H - 1));
  x = fmin(fmax(x, 0.0), (double)(W - 1));
  int y0 = (int)floor(y), x0 = (int)floor(x);
  int y1 = y0 + 1 < H ? y0 + 1 : y0, x1 = x0 + 1 < W ? x0 + 1 : x0;
  double fy = y - y0, fx = x - x0;
  const double top = fma(fx, (double)p[y0 + (size_t)H * x1], (1 - fx) * (double)p[y0 + (size_t)H * x0]);
  const double bot = fma(fx, (double)p[y1 + (size_t)H * x1], (1 - fx) * (double)p[y1 + (size_t)H * x0]);
  double v = fma(fy, bot, (1 - fy) * top);
  v = floor(v + 0.5);
  return (float)fmin(fmax(v, 0.0), 255.0);
}

// crop_resize_face_kernel over images of different sizes (xm_jpeg_decode_batch, jpeg.hip): image n is Hin x Win x 3 at
// pixels + desc[n][col_pix] with Hin, Win in its descriptor row.  The window is computed as xm_crop_resize_face's host
// code does and every pixel with the operations crop_resize_face_kernel compiles to, spelled out with contraction off
// (bilin_u8_pinned, the grey sum), so the output equals xm_crop_resize_face of that image alone bit for bit
// (tests/test_gpu_jpeg.py holds it to that on sizes whose samples land on ties).  RGB: the resized R, G, B instead of
// the normalised grey.
template <bool RGB>
__global__ void crop_resize_face_ragged_kernel(const float *__restrict__ pixels, float *__restrict__ out,
                                               const long long *__restrict__ desc, int stride, int col_h, int col_w,
                                               int col_pix, int N, float crop, int Ho, int Wo, float a0, float a1,
                                               float a2) {
  size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  const size_t HWo = (size_t)Ho * Wo;
  if (idx >= HWo * N) return;
  int n = (int)(idx / HWo);
  size_t q = idx - (size_t)n * HWo;
  int j = (int)(q / Ho), i = (int)(q - (size_t)j * Ho);
  const long long *d = desc + (size_t)n * stride;
  const int Hin = (int)d[col_h], Win = (int)d[col_w];
  double ch, cw, h0, w0;
  {
#pragma clang fp contract(off)
    ch = (double)crop * Hin;
    cw = (double)crop * Win;
    const double dh = Hin - ch, dw = Win - cw;
    h0 = 0.5 * dh;
    w0 = 0.5 * dw;
  }
  double y, x;
  {
#pragma clang fp contract(off)
    y = (i + 0.5) * ch / Ho - 0.5 + h0;
    x = (j + 0.5) * cw / Wo - 0.5 + w0;
  }
  const size_t HWi = (size_t)Hin * Win;
  const float *p = pixels + d[col_pix];
  float r = bilin_u8_pinned(p, Hin, Win, y, x), g = bilin_u8_pinned(p + HWi, Hin, Win, y, x),
        b = bilin_u8_pinned(p + 2 * HWi, Hin, Win, y, x);
  float *o = out + q + HWo * 3 * n;
  if constexpr (RGB) {
    o[0] = r;
    o[HWo] = g;
    o[2 * HWo] = b;
  } else {
    float gr;   // crop_resize_face_kernel: 0.2989f r + 0.5870f g + 0.1140f b as fma(b, .., fma(r, .., 0.5870f g))
    {
#pragma clang fp contract(off)
      gr = fmaf(b, 0.1140f, fmaf(r, 0.2989f, 0.5870f * g)) + 0.5f;
    }
    gr = fminf(floorf(gr), 255.f);
    o[0] = gr - a0;
    o[HWo] = gr - a1;
    o[2 * HWo] = gr - a2;
  }
}

int face_ragged_launch(const float *pixels, const long long *desc, int stride, int col_h, int col_w, int col_pix, int N,
                       float crop, int Ho, int Wo, const float *avg3, float *out, hipStream_t st) {
  size_t n = (size_t)Ho * Wo * N;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  if (avg3)
    hipLaunchKernelGGL(crop_resize_face_ragged_kernel<false>, grid, block, 0, st, pixels, out, desc, stride, col_h, col_w,
                       col_pix, N, crop, Ho, Wo, avg3[0], avg3[1], avg3[2]);
  else
    hipLaunchKernelGGL(crop_resize_face_ragged_kernel<true>, grid, block, 0, st, pixels, out, desc, stride, col_h, col_w,
                       col_pix, N, crop, Ho, Wo, 0.f, 0.f, 0.f);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

}  // namespace xm

extern "C" {

int xm_normalize_face(const float *rgb, int H, int W, int N, const float *avg3, float *out,
                      void *stream) {
  if (H <= 0 || W <= 0 || N <= 0) return fail(XM_EINVAL, "normalize_face: empty input");
  if (!rgb || !avg3 || !out) return fail(XM_EINVAL, "normalize_face: NULL tensor");
  float a[3];
  // averageImage is a 3-vector of host-known constants in the reference (meta.normalization);
  // accept a HOST pointer here to keep the launch free of a device round trip.
  a[0] = avg3[0];
  a[1] = avg3[1];
  a[2] = avg3[2];
  size_t n = (size_t)H * W * N;
  hipLaunchKernelGGL(normalize_face_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, rgb, out, H * W, N, a[0], a[1], a[2]);
  XM_LAUNCH_CHECK();
  return XM_OK;
}
}

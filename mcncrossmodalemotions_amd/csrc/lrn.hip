// vl_nnnormalize on gfx950: cross-channel (local response) normalisation, forward and backward.
//
//   L(i,j,k,s) = KAPPA + ALPHA * sum_{t in G(k)} X(i,j,t,s)^2,   G(k) = [k - m1, k + m2] n [0, C),
//   m1 = floor((N - 1) / 2), m2 = N - 1 - m1
//   Y  = X .* L.^(-BETA)
//   DX(k) = DZDY(k) L(k)^(-BETA) - 2 ALPHA BETA X(k) sum_{t in [k - m2, k + m1]} DZDY(t) X(t) L(t)^(-BETA - 1)
//
// X is H x W x C x S with H contiguous: a channel step is P = H * W floats.  Lanes run along pixels (coalesced) and
// every lane walks the channels of its pixels, so X (and DZDY) are read once and Y / DX written once; the window lives in
// registers and is summed afresh for every channel in ascending channel order (no running add / subtract).  HBM-bound.
//
// A block owns kLrnPixels pixels of one sample: four per lane, as one 16-byte access when P is a multiple of four and the
// tensors are 16-byte aligned (then every channel plane is), else as four coalesced 4-byte accesses a block-width apart.
// Planes with few pixels and many channels are split along the channel axis into chunks of at least kLrnChannelsPerPass
// channels until the launch has kLrnTargetBlocks blocks; a chunk re-reads the halo its windows need (m1 + m2 channels of
// X on each side for the backward pass, m1 / m2 for the forward), which its neighbour has just pulled into L2.
// Windows of more than kLrnRegWindow channels take the general arm, which re-reads the window of every element through
// the cache: correct for any N (N > 2 C included), not fast.
#include "prof.h"
#include "xm_common.h"

namespace xm {

constexpr int kLrnThreads = 256;
constexpr int kLrnPixels = 4 * kLrnThreads;     // pixels of one sample a block owns
constexpr int kLrnChannelsPerPass = 16;         // shortest channel chunk of a split channel axis
constexpr int kLrnRegWindow = 8;                // widest window the register arm holds
constexpr size_t kLrnTargetBlocks = 1024;       // four per CU: the channel axis is split until the launch has these
constexpr size_t kLrnMaxGrid = size_t(1) << 20; // blocks walk the tasks with this stride at most

struct LrnPlan {
  size_t P;        // pixels of a channel plane
  size_t pblocks;  // pixel blocks of a plane
  size_t tasks;    // pblocks * nsplit * S
  int C, nsplit, chunk;
};

static LrnPlan lrn_plan(int H, int W, int C, int S) {
  LrnPlan g;
  g.P = (size_t)H * (size_t)W;
  g.pblocks = (g.P + kLrnPixels - 1) / kLrnPixels;
  g.C = C;
  const size_t base = g.pblocks * (size_t)S;
  const size_t most = (size_t)((C + kLrnChannelsPerPass - 1) / kLrnChannelsPerPass);
  size_t want = (kLrnTargetBlocks + base - 1) / base;
  if (want > most) want = most;
  if (want < 1) want = 1;
  g.chunk = (int)(((size_t)C + want - 1) / want);
  g.nsplit = (C + g.chunk - 1) / g.chunk;
  g.tasks = base * (size_t)g.nsplit;
  return g;
}

struct LrnF4 {
  float v[4];
};

// the four pixels of this lane inside a plane: offsets and which of them exist
template <bool VEC>
struct LrnLane {
  size_t off[4];
  bool ok[4];
  __device__ LrnLane(size_t pb, size_t P) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      off[j] = VEC ? pb * kLrnPixels + 4 * (size_t)threadIdx.x + j : pb * kLrnPixels + threadIdx.x + (size_t)j * kLrnThreads;
      ok[j] = off[j] < P;
    }
  }
  __device__ __forceinline__ LrnF4 load(const float *__restrict__ plane) const {
    LrnF4 r;
    if (VEC) {
      // P is a multiple of four here: the four pixels exist together
      const float4 t = ok[0] ? *reinterpret_cast<const float4 *>(plane + off[0]) : make_float4(0.f, 0.f, 0.f, 0.f);
      r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) r.v[j] = ok[j] ? plane[off[j]] : 0.f;
    }
    return r;
  }
  __device__ __forceinline__ void store(float *__restrict__ plane, const LrnF4 &r) const {
    if (VEC) {
      if (ok[0]) *reinterpret_cast<float4 *>(plane + off[0]) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (ok[j]) plane[off[j]] = r.v[j];
    }
  }
};

__device__ __forceinline__ LrnF4 lrn_zero() {
  LrnF4 r;
  r.v[0] = r.v[1] = r.v[2] = r.v[3] = 0.f;
  return r;
}

struct LrnTask {
  size_t pb, s;
  int c0, c1;
  __device__ LrnTask(size_t task, const LrnPlan &g) {
    pb = task % g.pblocks;
    const size_t rest = task / g.pblocks;
    c0 = (int)(rest % (size_t)g.nsplit) * g.chunk;
    c1 = min(g.C, c0 + g.chunk);
    s = rest / (size_t)g.nsplit;
  }
};

template <int N, bool VEC>
__global__ void __launch_bounds__(kLrnThreads)
lrn_forward_kernel(const float *__restrict__ x, float *__restrict__ y, LrnPlan g, float kappa, float alpha, float beta) {
  constexpr int M1 = (N - 1) / 2, M2 = N - 1 - M1;
  const int C = g.C;
  for (size_t task = blockIdx.x; task < g.tasks; task += gridDim.x) {
    const LrnTask tk(task, g);
    const LrnLane<VEC> ln(tk.pb, g.P);
    const float *xs = x + tk.s * (size_t)C * g.P;
    float *ys = y + tk.s * (size_t)C * g.P;
    LrnF4 w[N];   // at channel c: w[j] = X(c - M1 + j)
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int ch = tk.c0 - M1 + j;
      w[j] = (ch >= 0 && ch < C) ? ln.load(xs + (size_t)ch * g.P) : lrn_zero();
    }
    for (int c = tk.c0; c < tk.c1; ++c) {
      const int nc = c + 1 + M2;
      const LrnF4 nx = (c + 1 < tk.c1 && nc < C) ? ln.load(xs + (size_t)nc * g.P) : lrn_zero();
      LrnF4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < N; ++j) sum += w[j].v[e] * w[j].v[e];
        const float L = kappa + alpha * sum;
        o.v[e] = w[M1].v[e] * exp2f(-beta * log2f(L));
      }
      ln.store(ys + (size_t)c * g.P, o);
#pragma unroll
      for (int j = 0; j + 1 < N; ++j) w[j] = w[j + 1];
      w[N - 1] = nx;
    }
  }
}

template <int N, bool VEC>
__global__ void __launch_bounds__(kLrnThreads)
lrn_backward_kernel(const float *__restrict__ x, const float *__restrict__ dzdy, float *__restrict__ dx, LrnPlan g,
                    float kappa, float alpha, float beta) {
  constexpr int M1 = (N - 1) / 2, M2 = N - 1 - M1;
  const int C = g.C;
  const float k2 = 2.f * alpha * beta;
  for (size_t task = blockIdx.x; task < g.tasks; task += gridDim.x) {
    const LrnTask tk(task, g);
    const LrnLane<VEC> ln(tk.pb, g.P);
    const size_t so = tk.s * (size_t)C * g.P;
    const float *xs = x + so, *ds = dzdy + so;
    float *os = dx + so;
    // the front t runs M1 channels ahead of the output channel k = t - M1:
    //   xw[j] = X(t - M1 + j)             the window of L(t); xw[0] = X(k)
    //   rw[j] = R(t - (N - 1) + j)        R = DZDY X L^(-BETA - 1): the adjoint window [k - M2, k + M1] of k
    //   gw[j] = DZDY L^(-BETA) at k + j
    const int t0 = tk.c0 - M2, t1 = tk.c1 - 1 + M1;
    LrnF4 xw[N], rw[N], gw[M1 + 1];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int ch = t0 - M1 + j;
      xw[j] = (ch >= 0 && ch < C) ? ln.load(xs + (size_t)ch * g.P) : lrn_zero();
      rw[j] = lrn_zero();
    }
#pragma unroll
    for (int j = 0; j <= M1; ++j) gw[j] = lrn_zero();
    LrnF4 dz = (t0 >= 0 && t0 < C) ? ln.load(ds + (size_t)t0 * g.P) : lrn_zero();
    for (int t = t0; t <= t1; ++t) {
      const int nc = t + 1 + M2;
      const bool more = t < t1;
      const LrnF4 nx = (more && nc >= 0 && nc < C) ? ln.load(xs + (size_t)nc * g.P) : lrn_zero();
      const LrnF4 ndz = (more && t + 1 >= 0 && t + 1 < C) ? ln.load(ds + (size_t)(t + 1) * g.P) : lrn_zero();
      LrnF4 r = lrn_zero(), gg = lrn_zero();
      if (t >= 0 && t < C) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float sum = 0.f;
#pragma unroll
          for (int j = 0; j < N; ++j) sum += xw[j].v[e] * xw[j].v[e];
          const float lg = log2f(kappa + alpha * sum);
          gg.v[e] = dz.v[e] * exp2f(-beta * lg);
          r.v[e] = dz.v[e] * xw[M1].v[e] * exp2f(-(beta + 1.f) * lg);
        }
      }
#pragma unroll
      for (int j = 0; j + 1 < N; ++j) rw[j] = rw[j + 1];
      rw[N - 1] = r;
#pragma unroll
      for (int j = 0; j < M1; ++j) gw[j] = gw[j + 1];
      gw[M1] = gg;
      const int k = t - M1;
      if (k >= tk.c0) {
        LrnF4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float sum = 0.f;
#pragma unroll
          for (int j = 0; j < N; ++j) sum += rw[j].v[e];
          o.v[e] = gw[0].v[e] - k2 * xw[0].v[e] * sum;
        }
        ln.store(os + (size_t)k * g.P, o);
      }
#pragma unroll
      for (int j = 0; j + 1 < N; ++j) xw[j] = xw[j + 1];
      xw[N - 1] = nx;
      dz = ndz;
    }
  }
}

// ---- the general arm: any N >= 1 ----------------------------------------------------------------------------------
__device__ __forceinline__ float lrn_log2_l(const float *__restrict__ px, size_t P, int C, int t, long long m1, long long m2,
                                            float kappa, float alpha) {
  const int lo = (int)max(0LL, t - m1), hi = (int)min((long long)C - 1, t + m2);
  float sum = 0.f;
  for (int u = lo; u <= hi; ++u) {
    const float v = px[(size_t)u * P];
    sum += v * v;
  }
  return log2f(kappa + alpha * sum);
}

template <bool BWD>
__global__ void __launch_bounds__(kLrnThreads)
lrn_general_kernel(const float *__restrict__ x, const float *__restrict__ dzdy, float *__restrict__ out, LrnPlan g,
                   long long m1, long long m2, float kappa, float alpha, float beta) {
  const int C = g.C;
  const float k2 = 2.f * alpha * beta;
  for (size_t task = blockIdx.x; task < g.tasks; task += gridDim.x) {
    const LrnTask tk(task, g);
    for (int j = 0; j < 4; ++j) {
      const size_t p = tk.pb * kLrnPixels + threadIdx.x + (size_t)j * kLrnThreads;
      if (p >= g.P) continue;
      const size_t so = tk.s * (size_t)C * g.P + p;
      const float *px = x + so;
      for (int c = tk.c0; c < tk.c1; ++c) {
        const float lg = lrn_log2_l(px, g.P, C, c, m1, m2, kappa, alpha);
        if (!BWD) {
          out[so + (size_t)c * g.P] = px[(size_t)c * g.P] * exp2f(-beta * lg);
          continue;
        }
        const int lo = (int)max(0LL, c - m2), hi = (int)min((long long)C - 1, c + m1);
        float sum = 0.f;
        for (int t = lo; t <= hi; ++t)
          sum += dzdy[so + (size_t)t * g.P] * px[(size_t)t * g.P] *
                 exp2f(-(beta + 1.f) * lrn_log2_l(px, g.P, C, t, m1, m2, kappa, alpha));
        out[so + (size_t)c * g.P] = dzdy[so + (size_t)c * g.P] * exp2f(-beta * lg) - k2 * px[(size_t)c * g.P] * sum;
      }
    }
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------
// validation shared by both directions; *empty: nothing to do
static int lrn_check(const char *what, const float *x, const float *dzdy, bool bwd, int H, int W, int C, int S, int N,
                     const float *out, bool *empty) {
  *empty = false;
  if (N < 1) return fail(XM_EINVAL, "%s: PARAM(1) = N must be a positive integer (got %d)", what, N);
  if (H < 0 || W < 0 || C < 0 || S < 0)
    return fail(XM_EINVAL, "%s: X has a negative dimension (%d x %d x %d x %d)", what, H, W, C, S);
  if (H == 0 || W == 0 || C == 0 || S == 0) {
    *empty = true;
    return XM_OK;
  }
  if (!x || !out || (bwd && !dzdy)) return fail(XM_EINVAL, "%s: NULL tensor", what);
  if (out == x || (bwd && out == dzdy)) return fail(XM_EINVAL, "%s: the output may not alias an input", what);
  return XM_OK;
}

template <int N, bool VEC>
static void lrn_launch_reg(bool bwd, const float *x, const float *dzdy, float *out, const LrnPlan &g, unsigned grid,
                           float kappa, float alpha, float beta, hipStream_t st) {
  if (bwd)
    hipLaunchKernelGGL((lrn_backward_kernel<N, VEC>), dim3(grid), dim3(kLrnThreads), 0, st, x, dzdy, out, g, kappa, alpha, beta);
  else
    hipLaunchKernelGGL((lrn_forward_kernel<N, VEC>), dim3(grid), dim3(kLrnThreads), 0, st, x, out, g, kappa, alpha, beta);
}

template <bool VEC>
static void lrn_launch_n(int N, bool bwd, const float *x, const float *dzdy, float *out, const LrnPlan &g, unsigned grid,
                         float kappa, float alpha, float beta, hipStream_t st) {
  switch (N) {
#define XM_LRN_CASE(n) \
  case n: lrn_launch_reg<n, VEC>(bwd, x, dzdy, out, g, grid, kappa, alpha, beta, st); break;
    XM_LRN_CASE(1) XM_LRN_CASE(2) XM_LRN_CASE(3) XM_LRN_CASE(4) XM_LRN_CASE(5) XM_LRN_CASE(6) XM_LRN_CASE(7) XM_LRN_CASE(8)
#undef XM_LRN_CASE
  }
}

static int lrn_run(bool bwd, const float *x, const float *dzdy, int H, int W, int C, int S, int N, float kappa, float alpha,
                   float beta, float *out, hipStream_t st) {
  const LrnPlan g = lrn_plan(H, W, C, S);
  const unsigned grid = (unsigned)(g.tasks < kLrnMaxGrid ? g.tasks : kLrnMaxGrid);
  const double bytes = 4.0 * (double)g.P * C * S * (bwd ? 3 : 2);
  if (N <= kLrnRegWindow) {
    // the gate is on the addresses as passed: a view that starts off a 16-byte boundary takes the 4-byte accesses
    const bool vec = (g.P & 3) == 0 && ((((uintptr_t)x | (uintptr_t)dzdy | (uintptr_t)out) & 15) == 0);
    ProfScope ps(prof_key(kProfLrn, (bwd ? 2 : 0) + (vec ? 1 : 0)), 0, st, bytes);
    if (vec)
      lrn_launch_n<true>(N, bwd, x, dzdy, out, g, grid, kappa, alpha, beta, st);
    else
      lrn_launch_n<false>(N, bwd, x, dzdy, out, g, grid, kappa, alpha, beta, st);
  } else {
    const long long m1 = ((long long)N - 1) / 2, m2 = (long long)N - 1 - m1;
    ProfScope ps(prof_key(kProfLrn, bwd ? 5 : 4), 0, st, bytes);
    if (bwd)
      hipLaunchKernelGGL((lrn_general_kernel<true>), dim3(grid), dim3(kLrnThreads), 0, st, x, dzdy, out, g, m1, m2, kappa,
                         alpha, beta);
    else
      hipLaunchKernelGGL((lrn_general_kernel<false>), dim3(grid), dim3(kLrnThreads), 0, st, x, dzdy, out, g, m1, m2, kappa,
                         alpha, beta);
  }
  XM_LAUNCH_CHECK();
  return XM_OK;
}

}  // namespace xm

using namespace xm;

extern "C" {

int xm_nnnormalize_forward(const float *x, int H, int W, int C, int S, int N, float kappa, float alpha, float beta, float *y,
                           void *stream) {
  bool empty;
  const int rc = lrn_check("vl_nnnormalize", x, nullptr, false, H, W, C, S, N, y, &empty);
  if (rc != XM_OK || empty) return rc;
  return lrn_run(false, x, nullptr, H, W, C, S, N, kappa, alpha, beta, y, (hipStream_t)stream);
}

int xm_nnnormalize_backward(const float *x, const float *dzdy, int H, int W, int C, int S, int N, float kappa, float alpha,
                            float beta, float *dx, void *stream) {
  bool empty;
  const int rc = lrn_check("vl_nnnormalize (backward)", x, dzdy, true, H, W, C, S, N, dx, &empty);
  if (rc != XM_OK || empty) return rc;
  return lrn_run(true, x, dzdy, H, W, C, S, N, kappa, alpha, beta, dx, (hipStream_t)stream);
}

int xm_nnnormalize_geometry(int *pixels_per_block, int *channels_per_pass, int *window_in_registers) {
  if (pixels_per_block) *pixels_per_block = kLrnPixels;
  if (channels_per_pass) *channels_per_pass = kLrnChannelsPerPass;
  if (window_in_registers) *window_in_registers = kLrnRegWindow;
  return XM_OK;
}

}  // extern "C"

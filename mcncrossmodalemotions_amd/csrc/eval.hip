// The arithmetic of external/run_cross_val.m and external/emo_benchmarks.m on gfx950: MATLAB's nominal mnrfit
// (Newton-Raphson in fp64 from B = 0) and mnrval + confusionmat, G independent problems per launch, one workgroup per
// problem.  Every sum runs in a fixed order and there are no float atomics, so each problem's outputs are a function of
// its own inputs alone: the same bits whatever G is and whichever problems share the launch.
#include "xm_common.h"

namespace xm {

constexpr int kMnrThreads = 256;
constexpr int kMnrChunk = 32;       // training rows staged in LDS per pass of the Hessian accumulation
constexpr int kMnrMaxD = 64;        // (p + 1)(k - 1): 64 x 64 doubles of Hessian = 32 KB of LDS
constexpr int kMnrMaxEnt = (kMnrMaxD * (kMnrMaxD + 1) / 2 + kMnrThreads - 1) / kMnrThreads;   // 9 per thread
constexpr int kMnrMaxHalvings = 30;
constexpr double kMnrPivotTol = 1e-14;   // a Cholesky pivot <= this x the largest diagonal entry: not positive definite

// e-th entry (row-major) of a lower triangle: r >= c
__device__ __forceinline__ void tri_index(int e, int &r, int &c) {
  int q = (int)((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
  while (q * (q + 1) / 2 > e) --q;
  while ((q + 1) * (q + 2) / 2 <= e) ++q;
  r = q;
  c = e - q * (q + 1) / 2;
}

// log(1 + r) to a few ulps for r >= 0 without the library's log1p (Goldberg: the rounding of 1 + r cancels in the
// ratio).  With the library's log1p the deviance of separable data came back in steps of 2^-52, i.e. it behaved as
// log(1 + r): the log-likelihood then stops moving and every step is halved away.
__device__ __forceinline__ double log1p_acc(double r) {
  const double u = 1.0 + r;
  return u == 1.0 ? r : log(u) * (r / (u - 1.0));
}

struct MnrShape {
  int p, P1, km1, D, NT;   // features, p + 1, k - 1, parameters, lower-triangle entries
};

// log-likelihood L, gradient g = dL/dB and information matrix H = -d2L/dB2 (lower triangle, row-major D x D) at B, all
// training rows of the problem in their listed order.  Entry (r, c), r = a + P1 j, c = b + P1 l:
//   H = sum_i xt_a xt_b pi_j (delta_jl - pi_l),   g_r = sum_i xt_a ([y_i == j] - pi_j),   xt = [1, x],
// with 1 - pi_j taken from the other classes' terms.
// Every entry is one thread's running sum over the rows in order; L is summed in order by the last thread.
__device__ void mnr_eval(const MnrShape &s, const double *__restrict__ B, const float *__restrict__ x,
                         const int *__restrict__ labels, const int *__restrict__ rows, int nrow, double *H,
                         double *g, double *Lout, double *xs, double *pis, double *qis, double *lp, int *lab) {
  const int tid = threadIdx.x;
  double acc[kMnrMaxEnt];
  int ea[kMnrMaxEnt], eb[kMnrMaxEnt], ej[kMnrMaxEnt], el[kMnrMaxEnt];
#pragma unroll
  for (int q = 0; q < kMnrMaxEnt; ++q) {
    acc[q] = 0.0;
    int e = tid + q * kMnrThreads, r = 0, c = 0;
    if (e < s.NT) tri_index(e, r, c);
    ea[q] = r % s.P1;
    ej[q] = r / s.P1;
    eb[q] = c % s.P1;
    el[q] = c / s.P1;
  }
  const int ga = tid % s.P1, gj = tid / s.P1;
  double gacc = 0.0, Lacc = 0.0;
  for (int c0 = 0; c0 < nrow; c0 += kMnrChunk) {
    const int cnt = min(kMnrChunk, nrow - c0);
    __syncthreads();   // the previous chunk has been consumed
    if (tid < cnt) {
      const int row = rows[c0 + tid] - 1;   // validated by the caller
      const float *xr = x + (size_t)s.p * row;
      double *xt = xs + tid * s.P1;
      double *pr = pis + tid * s.km1;
      double *qr = qis + tid * s.km1;
      xt[0] = 1.0;
      for (int a = 0; a < s.p; ++a) xt[a + 1] = (double)xr[a];
      double m = 0.0;   // the reference category's eta is 0
      int jmax = s.km1;
      for (int j = 0; j < s.km1; ++j) {
        double eta = 0.0;
        for (int a = 0; a < s.P1; ++a) eta = fma(xt[a], B[a + s.P1 * j], eta);
        pr[j] = eta;
        if (eta > m) {
          m = eta;
          jmax = j;
        }
      }
      const int y = labels[row] - 1;
      const double etay = y == s.km1 ? 0.0 : pr[y], eref = exp(-m);
      // exponentials relative to the largest eta (that one is exactly 1); r = the sum of all others, so that
      // log S = log1p(r) and 1 - pi_j = (sum over l != j) / S keep their accuracy when the probabilities saturate
      // (separable data): 1 - pi_j formed by subtraction would round to 0 and empty the information matrix
      double r = jmax == s.km1 ? 0.0 : eref;
      for (int j = 0; j < s.km1; ++j) {
        const double ex = exp(pr[j] - m);
        pr[j] = ex;
        if (j != jmax) r += ex;
      }
      const double S = 1.0 + r;
      for (int j = 0; j < s.km1; ++j) {
        double o = eref;
        for (int l = 0; l < s.km1; ++l)
          if (l != j) o += pr[l];
        qr[j] = o / S;
      }
      for (int j = 0; j < s.km1; ++j) pr[j] /= S;
      lp[tid] = (etay - m) - log1p_acc(r);
      lab[tid] = y;
    }
    __syncthreads();
    for (int i = 0; i < cnt; ++i) {
      const double *xt = xs + i * s.P1;
      const double *pr = pis + i * s.km1, *qr = qis + i * s.km1;
#pragma unroll
      for (int q = 0; q < kMnrMaxEnt; ++q) {
        if (tid + q * kMnrThreads < s.NT) {
          const double w = pr[ej[q]] * (ej[q] == el[q] ? qr[el[q]] : -pr[el[q]]);
          acc[q] = fma(xt[ea[q]] * xt[eb[q]], w, acc[q]);
        }
      }
      if (tid < s.D) gacc += xt[ga] * (lab[i] == gj ? qr[gj] : -pr[gj]);
      if (tid == kMnrThreads - 1) Lacc += lp[i];
    }
  }
#pragma unroll
  for (int q = 0; q < kMnrMaxEnt; ++q) {
    int e = tid + q * kMnrThreads;
    if (e < s.NT) H[(ea[q] + s.P1 * ej[q]) * s.D + (eb[q] + s.P1 * el[q])] = acc[q];
  }
  if (tid < s.D) g[tid] = gacc;
  if (tid == kMnrThreads - 1) *Lout = Lacc;
  __syncthreads();
}

// in-place lower Cholesky of H (row-major D x D, lower triangle); false (uniform) when a pivot is not positive
__device__ bool mnr_cholesky(double *H, int D) {
  const int tid = threadIdx.x;
  __syncthreads();
  double dmax = 0.0;
  for (int i = 0; i < D; ++i) dmax = fmax(dmax, H[i * D + i]);
  const double tol = kMnrPivotTol * dmax;
  for (int kk = 0; kk < D; ++kk) {
    __syncthreads();
    const double d = H[kk * D + kk];
    if (!(d > tol) || !isfinite(d)) return false;   // every thread read the same value
    const int m = D - kk - 1, ne = m * (m + 1) / 2;
    for (int e = tid; e < ne; e += kMnrThreads) {
      int r, c;
      tri_index(e, r, c);
      const int i = kk + 1 + r, j = kk + 1 + c;
      H[i * D + j] -= H[i * D + kk] * H[j * D + kk] / d;
    }
    __syncthreads();
    const double piv = sqrt(d);
    if (tid == 0) H[kk * D + kk] = piv;
    for (int i = kk + 1 + tid; i < D; i += kMnrThreads) H[i * D + kk] /= piv;
  }
  __syncthreads();
  return true;
}

// delta = (L L')^-1 g by wave 0: lane i holds entry i, one shuffle per substitution step
__device__ void mnr_solve(const double *H, const double *g, double *delta, int D) {
  const int lane = threadIdx.x;
  if (lane < 64) {
    double v = lane < D ? g[lane] : 0.0;
    for (int i = 0; i < D; ++i) {
      const double yi = __shfl(v, i) / H[i * D + i];
      if (lane == i) v = yi;
      else if (lane > i && lane < D) v -= H[lane * D + i] * yi;
    }
    for (int i = D - 1; i >= 0; --i) {
      const double xi = __shfl(v, i) / H[i * D + i];
      if (lane == i) v = xi;
      else if (lane < i) v -= H[i * D + lane] * xi;
    }
    if (lane < D) delta[lane] = v;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(kMnrThreads)
mnrfit_kernel(const float *__restrict__ x, int p, int n, const int *__restrict__ labels, int k,
              const int *__restrict__ offsets, const int *__restrict__ rows, int nnz, int max_iter, double tol_x,
              double *__restrict__ b_out, double *__restrict__ dev_out, int *__restrict__ iters_out,
              int *__restrict__ status_out) {
  extern __shared__ double smem[];
  MnrShape s;
  s.p = p;
  s.P1 = p + 1;
  s.km1 = k - 1;
  s.D = s.P1 * s.km1;
  s.NT = s.D * (s.D + 1) / 2;
  const int D = s.D, tid = threadIdx.x, gidx = blockIdx.x;
  double *H = smem;                           // D x D
  double *Bc = H + D * D, *Bn = Bc + D, *delta = Bn + D, *g = delta + D;
  double *xs = g + D;                         // kMnrChunk x (p + 1)
  double *pis = xs + kMnrChunk * s.P1;        // kMnrChunk x (k - 1)
  double *qis = pis + kMnrChunk * s.km1;      // kMnrChunk x (k - 1): 1 - pi
  double *lp = qis + kMnrChunk * s.km1;       // kMnrChunk
  double *Ls = lp + kMnrChunk;                // [0] L at the current point, [1] at the trial point
  int *lab = (int *)(Ls + 2);                 // kMnrChunk
  int *cnt = lab + kMnrChunk;                 // k class counts, [k] = bad-input flag
  double *Bout = b_out + (size_t)gidx * D;

  // ---- validate the problem before any row of X is read
  const int off0 = offsets[gidx], off1 = offsets[gidx + 1];
  for (int i = tid; i <= k; i += kMnrThreads) cnt[i] = 0;
  __syncthreads();
  const bool csr_ok = off0 >= 0 && off1 >= off0 && off1 <= nnz;
  if (!csr_ok) {
    if (tid == 0) cnt[k] = 1;
  } else {
    for (int i = off0 + tid; i < off1; i += kMnrThreads) {
      const int row = rows[i];
      const int y = (row >= 1 && row <= n) ? labels[row - 1] : 0;
      if (y < 1 || y > k) atomicOr(&cnt[k], 1);
      else atomicAdd(&cnt[y - 1], 1);
    }
  }
  __syncthreads();
  bool bad = cnt[k] != 0;
  for (int c = 0; c < k; ++c) bad = bad || cnt[c] == 0;   // a class absent from the training rows
  if (bad) {
    for (int r = tid; r < D; r += kMnrThreads) Bout[r] = 0.0;
    if (tid == 0) {
      dev_out[gidx] = __longlong_as_double(0x7ff8000000000000ll);
      iters_out[gidx] = 0;
      status_out[gidx] = XM_MNR_BADINPUT;
    }
    return;
  }
  const int *prow = rows + off0;
  const int nrow = off1 - off0;

  // ---- Newton-Raphson from B = 0 with step halving
  for (int r = tid; r < D; r += kMnrThreads) Bc[r] = 0.0;
  __syncthreads();
  mnr_eval(s, Bc, x, labels, prow, nrow, H, g, &Ls[0], xs, pis, qis, lp, lab);
  int status = XM_MNR_ITERLIMIT, iters = 0;
  for (int it = 1; it <= max_iter; ++it) {
    if (!mnr_cholesky(H, D)) {
      status = XM_MNR_NOTPD;
      break;
    }
    mnr_solve(H, g, delta, D);
    double t = 1.0;
    bool ascent = false;
    for (int h = 0;; ++h) {
      for (int r = tid; r < D; r += kMnrThreads) Bn[r] = Bc[r] + t * delta[r];
      __syncthreads();
      mnr_eval(s, Bn, x, labels, prow, nrow, H, g, &Ls[1], xs, pis, qis, lp, lab);
      ascent = Ls[1] >= Ls[0];   // NaN compares false: halve
      if (ascent || h == kMnrMaxHalvings) break;
      t *= 0.5;
    }
    double step = 0.0, bmax = 0.0;
    for (int r = 0; r < D; ++r) {
      step = fmax(step, fabs(Bn[r] - Bc[r]));
      bmax = fmax(bmax, fabs(Bn[r]));
    }
    __syncthreads();   // every thread has read Bc / Ls before they move
    for (int r = tid; r < D; r += kMnrThreads) Bc[r] = Bn[r];
    if (tid == 0) Ls[0] = Ls[1];
    __syncthreads();
    iters = it;
    // a step that every halving failed to make an ascent is short, not converged
    if (ascent && step <= tol_x * fmax(1.0, bmax)) {
      status = XM_MNR_CONVERGED;
      break;
    }
  }
  for (int r = tid; r < D; r += kMnrThreads) Bout[r] = Bc[r];
  if (tid == 0) {
    dev_out[gidx] = -2.0 * Ls[0];
    iters_out[gidx] = iters;
    status_out[gidx] = status;
  }
}

// mnrval + max(preds, [], 2) + confusionmat(labels, cls, 'Order', 1:k): a thread per validation row
__global__ void __launch_bounds__(256)
mnrval_kernel(const double *__restrict__ b, const float *__restrict__ x, int p, int n, int k,
              const int *__restrict__ offsets, const int *__restrict__ rows, int nnz, const int *__restrict__ labels,
              double *__restrict__ probs, int *__restrict__ preds, int *__restrict__ conf) {
  extern __shared__ double smem[];
  const int P1 = p + 1, km1 = k - 1, D = P1 * km1, gidx = blockIdx.x, tid = threadIdx.x;
  double *Bs = smem;
  int *cnt = (int *)(Bs + D);   // k x k, column-major: (true, predicted)
  const double *Bg = b + (size_t)gidx * D;
  for (int r = tid; r < D; r += 256) Bs[r] = Bg[r];
  for (int i = tid; i < k * k; i += 256) cnt[i] = 0;
  __syncthreads();
  int off0 = offsets[gidx], off1 = offsets[gidx + 1];
  const bool csr_ok = off0 >= 0 && off1 >= off0 && off1 <= nnz;
  if (!csr_ok) off1 = off0;   // no row is touched; the counts stay 0
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  for (int i = off0 + tid; i < off1; i += 256) {
    const int row = rows[i] - 1;
    double *pr = probs ? probs + (size_t)i * k : nullptr;
    if (row < 0 || row >= n) {
      if (pr)
        for (int j = 0; j < k; ++j) pr[j] = qnan;
      preds[i] = 0;
      continue;
    }
    const float *xr = x + (size_t)p * row;
    double m = 0.0;
    for (int j = 0; j < km1; ++j) {
      double eta = Bs[P1 * j];
      for (int a = 0; a < p; ++a) eta = fma((double)xr[a], Bs[a + 1 + P1 * j], eta);
      m = fmax(m, eta);
    }
    double S = exp(-m);
    for (int j = 0; j < km1; ++j) {
      double eta = Bs[P1 * j];
      for (int a = 0; a < p; ++a) eta = fma((double)xr[a], Bs[a + 1 + P1 * j], eta);
      S += exp(eta - m);
    }
    double best = -1.0;
    int arg = 0;
    for (int j = 0; j < k; ++j) {
      double eta = 0.0;
      if (j < km1) {
        eta = Bs[P1 * j];
        for (int a = 0; a < p; ++a) eta = fma((double)xr[a], Bs[a + 1 + P1 * j], eta);
      }
      const double pj = exp(eta - m) / S;
      if (pr) pr[j] = pj;
      if (pj > best) {   // the first maximum wins, as max(preds, [], 2)
        best = pj;
        arg = j;
      }
    }
    preds[i] = arg + 1;
    if (labels && conf) {
      const int t = labels[row];
      if (t >= 1 && t <= k) atomicAdd(&cnt[(t - 1) + k * arg], 1);   // integer counts: exact in any order
    }
  }
  __syncthreads();
  if (conf)
    for (int i = tid; i < k * k; i += 256) conf[(size_t)gidx * k * k + i] = cnt[i];
}

static int mnr_check(const char *who, const float *x, int p, int n, int k, const int *offsets, const int *rows,
                     int nnz, int G) {
  if (p < 1 || n < 1 || k < 2 || G < 0 || nnz < 0)
    return fail(XM_EINVAL, "%s: need p >= 1, n >= 1, k >= 2 (got p=%d n=%d k=%d G=%d nnz=%d)", who, p, n, k, G, nnz);
  if ((p + 1) * (k - 1) > kMnrMaxD)
    return fail(XM_EINVAL, "%s: (p + 1)(k - 1) = %d parameters, at most %d are supported", who, (p + 1) * (k - 1),
                kMnrMaxD);
  if (G > 0 && (!x || !offsets || (nnz > 0 && !rows))) return fail(XM_EINVAL, "%s: NULL tensor", who);
  return XM_OK;
}

}  // namespace xm

using namespace xm;

extern "C" {

int xm_mnrfit(const float *x, int p, int n, const int *labels, int k, const int *offsets, const int *rows, int nnz,
              int G, int max_iter, double tol_x, double *b_out, double *dev_out, int *iters_out, int *status_out,
              void *stream) {
  int rc = mnr_check("mnrfit", x, p, n, k, offsets, rows, nnz, G);
  if (rc) return rc;
  if (max_iter < 0 || !(tol_x >= 0.0)) return fail(XM_EINVAL, "mnrfit: need max_iter >= 0 and tol_x >= 0");
  if (G == 0) return XM_OK;
  if (!labels || !b_out || !dev_out || !iters_out || !status_out) return fail(XM_EINVAL, "mnrfit: NULL tensor");
  const int P1 = p + 1, D = P1 * (k - 1);
  const size_t lds = sizeof(double) * ((size_t)D * D + 4 * D + kMnrChunk * (P1 + 2 * (k - 1) + 1) + 2) +
                     sizeof(int) * (kMnrChunk + k + 1);
  hipLaunchKernelGGL(mnrfit_kernel, dim3(G), dim3(kMnrThreads), lds, (hipStream_t)stream, x, p, n, labels, k, offsets,
                     rows, nnz, max_iter, tol_x, b_out, dev_out, iters_out, status_out);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_mnrval(const double *b, const float *x, int p, int n, int k, const int *offsets, const int *rows, int nnz, int G,
              const int *labels, double *probs_out, int *preds_out, int *conf_out, void *stream) {
  int rc = mnr_check("mnrval", x, p, n, k, offsets, rows, nnz, G);
  if (rc) return rc;
  if (G == 0) return XM_OK;
  if (!b || !preds_out) return fail(XM_EINVAL, "mnrval: NULL tensor");
  const int D = (p + 1) * (k - 1);
  const size_t lds = sizeof(double) * D + sizeof(int) * (size_t)k * k;
  hipLaunchKernelGGL(mnrval_kernel, dim3(G), dim3(256), lds, (hipStream_t)stream, b, x, p, n, k, offsets, rows, nnz,
                     labels, probs_out, preds_out, conf_out);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

}  // extern "C"

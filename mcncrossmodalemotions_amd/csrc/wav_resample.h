// The one resampler of the library: the taps of MATLAB's resample(x, p, q) evaluated in the kernel, shared by
// xm_wav_batch (misc.hip: clips cut from the decoded bank) and xm_wav_decode_resample_batch (wav.hip: files decoded and
// brought to one rate in one pass).  Both units run the same text, so a sample resampled by either has the same bits.
//
// The filter of resample(x, p, q) is never stored: with P = max(p, q), half = 10 P and the delay removed, output j is
//   y[j] = g sum_k u(j q - k p) x[k],  |j q - k p| <= half,  u(m) = sinc(m / P) I0(beta sqrt(1 - (m / half)^2)),
// g = p / sum_m u(m) (the constant 1 / (P I0(beta)) of the toolbox's taps cancels in p h / sum(h)).  sin(pi m / P)
// comes from r = m mod P and the parity of floor(m / P), both carried along the tap loop in integers (m moves by p per
// tap), so the argument of the sine is exact at every |m|; I0(beta sqrt(s)) is its power series in beta^2 s / 4, which
// needs no square root.  wav_gain_block (one workgroup of 1024 per clip) reduces p, q by their gcd and sums u in fp64.
#pragma once
#include "xm_common.h"

namespace xm {

struct WavClip {
  int p, q;     // reduced ratio; p == 0: the clip has nothing to resample (a crop, or an unusable descriptor)
  float gain;   // p / sum(u)
  float pad;
};
constexpr int kWavMaxRatio = 1 << 20;
constexpr float kWavBeta2Over4 = 6.25f;   // kaiser(L, 5): beta^2 / 4

// I0(2 sqrt(y)) = sum_k y^k / (k!)^2 on 0 <= y <= 6.25: the first dropped term is below 2e-11 of the sum
__device__ __forceinline__ float wav_i0(float y) {
  const float c[15] = {1.000000000e+00f, 1.000000000e+00f, 2.500000000e-01f, 2.777777778e-02f, 1.736111111e-03f,
                       6.944444444e-05f, 1.929012346e-06f, 3.936759889e-08f, 6.151187327e-10f, 7.594058428e-12f,
                       7.594058428e-14f, 6.276081346e-16f, 4.358389823e-18f, 2.578928890e-20f, 1.315780046e-22f};
  float s = c[14];
#pragma unroll
  for (int k = 13; k >= 0; --k) s = fmaf(s, y, c[k]);
  return s;
}

// u(m) for |m| <= half, given r = m mod P in [0, P) and odd = parity of floor(m / P)
__device__ __forceinline__ float wav_tap(int m, int r, int odd, int P, float invP, float P_over_pi, int half, float kb) {
  const int rr = 2 * r > P ? P - r : r;              // sin(pi r / P) = sin(pi (P - r) / P): argument in [0, pi / 2]
  float s = sinpif((float)rr * invP);
  s = odd ? -s : s;
  const float w = wav_i0((float)(half - m) * (float)(half + m) * kb);
  return m == 0 ? w : s * P_over_pi * __builtin_amdgcn_rcpf((float)m) * w;
}

// the gain of one clip, by a whole workgroup of 1024 threads: clip[n] = {p, q reduced, p / sum(u)}
__device__ __forceinline__ void wav_gain_block(long long p, long long q, WavClip *__restrict__ clip, int n) {
  __shared__ double part[16];
  const int tid = threadIdx.x;
  if (p < 1 || q < 1 || p > kWavMaxRatio || q > kWavMaxRatio || p == q) {   // the same for every thread of the block
    if (tid == 0) clip[n] = WavClip{0, 0, 0.f, 0.f};
    return;
  }
  long long a = p, b = q;
  while (b) {
    long long t = a % b;
    a = b;
    b = t;
  }
  p /= a;
  q /= a;
  const int P = (int)(p > q ? p : q), half = 10 * P;
  const float invP = 1.f / (float)P, P_over_pi = (float)P * 0.318309886f, kb = kWavBeta2Over4 / ((float)half * (float)half);
  double acc = 0.0;
  for (int m = 1 + tid; m < half; m += 1024) {   // u(-m) = u(m), u(half) = 0
    const int qd = m / P;
    acc += (double)wav_tap(m, m - qd * P, qd & 1, P, invP, P_over_pi, half, kb);
  }
  acc = xm_wave_sum_d(acc);
  if ((tid & 63) == 0) part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int w = 0; w < 16; ++w) s += part[w];
    s = 2.0 * s + (double)wav_tap(0, 0, 0, P, invP, P_over_pi, half, kb);
    clip[n] = WavClip{(int)p, (int)q, (float)((double)p / s), 0.f};
  }
}

}  // namespace xm

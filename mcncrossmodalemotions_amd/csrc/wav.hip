// audioinfo / audioread of a batch of WAV files on gfx950: what cnn_get_batch_wav_emo does to every clip and noise file
// (emoVoxCeleb/getBatchEmoVoxCeleb.m:79,97-117,126) and compute_audio_feats.m:173-175 to every test clip, decoded into
// the device waveform bank that xm_wav_batch and xm_spec_bucket_batch read.  include/xmodal.h documents the descriptor.
//
// xm_wav_plan (host, no device call) is csrc/wav_plan.h behind the C ABI.  xm_wav_decode_batch is ONE launch of
//   wav_decode_kernel    a fixed-size grid walks the batch's output floats [desc[0][out], desc[N-1][out] + its floats) in
//                        tiles of kWavTile floats.  A thread makes 16-byte pieces of the OUTPUT (aligned by address, so
//                        a piece may begin before the batch or straddle two files): it finds the file by bisection over
//                        the descriptors' output offsets -- narrowed per tile on block-uniform values first --, and
//                        * a piece inside one mono file reads the aligned dwords covering its 4 .. 32 source bytes,
//                          funnel-shifts them to the sample boundary, converts and stores 16 bytes;
//                        * a piece inside one interleaved file gathers its four samples (two or three dwords each) and
//                          stores 16 bytes -- channel c of a frames x channels matrix is contiguous in MATLAB layout;
//                        * a piece at a boundary is done float by float.
//                        A dword index is clamped to the dwords that hold the file's data range, itself clamped to the
//                        buffer; an output index is compared against the batch's range and out_floats before the store.
//                        No atomics, no workspace; every output float has exactly one writer.
//
// xm_wav_plan_fs / xm_wav_decode_resample_batch (ABI 122) bring files of any rate to one: [z, Fs] = audioread(f);
// z = resample(z(:, c), fs, Fs) for a whole batch in one pass, no native-rate bank in between.  TWO launches:
//   wav_rate_gain_kernel  one workgroup per file: the fp64 sum of the filter's taps (wav_resample.h, shared with misc.hip)
//   wav_resample_kernel   laid out by the output like the kernel above; a tile's (file, channel) pieces are cut into
//                         runs whose source window fits LDS, the window is decoded once and the taps run from there.
//                         Documented in front of the kernel, further down.
#include <algorithm>

#include "prof.h"
#include "wav_plan.h"
#include "wav_resample.h"
#include "xm_common.h"

namespace xm {

constexpr int kWavDesc = XM_WAV_DESC;
constexpr int kWavQuads = 4;                        // 16-byte pieces per thread and tile
constexpr int kWavTile = 256 * 4 * kWavQuads;       // output floats per tile
constexpr int kWavMaxBlocks = 256 * 8;

struct WavFile {
  long long kmin, kmax;    // first and last dword that hold bytes of the data range
  long long begin;         // first byte of frame `first`
  long long frames, out, count;
  int nch, fmt, cw, sel, bps;
};

__device__ __forceinline__ int wav_find(const long long *__restrict__ desc, int lo, int hi, long long a) {
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (desc[(long long)mid * kWavDesc + WD_OUT] <= a) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ int wav_bps(int fmt) {
  return fmt == XM_WAV_U8 ? 1 : fmt == XM_WAV_S16 ? 2 : fmt == XM_WAV_S24 ? 3 : fmt == XM_WAV_F64 ? 8 : 4;
}

__device__ __forceinline__ WavFile wav_file(const long long *__restrict__ desc, int i, long long nbytes) {
  const long long *d = desc + (long long)i * kWavDesc;
  WavFile f;
  const long long b = min(max(d[WD_BEGIN], 0LL), nbytes), e = min(max(d[WD_END], b), nbytes);
  f.kmin = b >> 2;
  f.kmax = e > b ? (e - 1) >> 2 : f.kmin;
  f.kmax = min(f.kmax, max((nbytes - 1) >> 2, 0LL));
  f.kmin = min(f.kmin, f.kmax);
  f.nch = (int)min(max(d[WD_NCH], 1LL), 64LL);
  f.fmt = (int)min(max(d[WD_FMT], 0LL), (long long)XM_WAV_F64);
  f.bps = wav_bps(f.fmt);
  f.cw = (int)min(max(d[WD_CW], 1LL), (long long)f.nch);
  f.sel = (int)min(max(d[WD_SEL], -1LL), (long long)f.nch - 1);
  f.frames = max(d[WD_FRAMES], 0LL);
  f.begin = b + max(d[WD_FIRST], 0LL) * f.nch * f.bps;
  f.out = d[WD_OUT];
  f.count = f.frames * f.cw;
  return f;
}

// NW dwords of bytes starting at byte p (any alignment): NW + 1 aligned dword loads, every index clamped to [kmin, kmax]
template <int NW>
__device__ __forceinline__ void wav_window(const uint32_t *__restrict__ words, long long p, long long kmin, long long kmax,
                                           uint32_t (&a)[NW]) {
  const long long k0 = p >> 2;
  const int sh = (int)(p & 3) * 8;
  uint32_t w[NW + 1];
#pragma unroll
  for (int j = 0; j <= NW; ++j) w[j] = words[min(max(k0 + j, kmin), kmax)];
#pragma unroll
  for (int j = 0; j < NW; ++j) a[j] = (uint32_t)((((unsigned long long)w[j + 1] << 32) | w[j]) >> sh);
}

// ---- sample values: single(audioread's double), as bits -----------------------------------------------------------
__device__ __forceinline__ uint32_t wav_u8(uint32_t v) { return __float_as_uint((float)((int)(v & 0xFFu) - 128) * 0x1p-7f); }
__device__ __forceinline__ uint32_t wav_s16(uint32_t v) { return __float_as_uint((float)(int)(short)(v & 0xFFFFu) * 0x1p-15f); }
__device__ __forceinline__ uint32_t wav_s24(uint32_t v) { return __float_as_uint((float)((int)(v << 8) >> 8) * 0x1p-23f); }
// int -> float rounds to nearest even; the scaling by a power of two is exact (no result is below 2^-31)
__device__ __forceinline__ uint32_t wav_s32(uint32_t v) { return __float_as_uint((float)(int)v * 0x1p-31f); }
// double -> float, round to nearest even, in integer arithmetic: independent of the kernel's denormal mode.  A NaN keeps
// its sign and the top 22 payload bits and becomes quiet, as a conversion instruction makes it.
__device__ __forceinline__ uint32_t wav_f64(uint32_t lo, uint32_t hi) {
  const uint32_t sign = hi & 0x80000000u;
  const int ex = (int)((hi >> 20) & 0x7FFu);
  const unsigned long long mant = ((unsigned long long)(hi & 0xFFFFFu) << 32) | lo;
  if (ex == 0x7FF) return mant ? (sign | 0x7FC00000u | (uint32_t)(mant >> 29)) : (sign | 0x7F800000u);
  if (ex == 0) return sign;                                    // zero or a double denormal: far below 2^-150
  const int e = ex - 1023 + 127;
  if (e >= 255) return sign | 0x7F800000u;
  if (e >= 1) {
    const uint32_t r = (uint32_t)(mant >> 29), rem = (uint32_t)mant & 0x1FFFFFFFu;
    const uint32_t up = (rem > 0x10000000u || (rem == 0x10000000u && (r & 1u))) ? 1u : 0u;
    return sign | ((((uint32_t)e << 23) | r) + up);            // a carry runs into the exponent, up to infinity
  }
  const int shift = 30 - e;                                     // a float denormal: 1.m x 2^(e - 127) in units of 2^-149
  if (shift > 53) return sign;
  const unsigned long long m53 = mant | (1ULL << 52);
  const unsigned long long q = m53 >> shift, rem = m53 & ((1ULL << shift) - 1), half = 1ULL << (shift - 1);
  const uint32_t up = (rem > half || (rem == half && (q & 1ULL))) ? 1u : 0u;
  return sign | ((uint32_t)q + up);
}

// one sample at byte p
__device__ __forceinline__ uint32_t wav_sample(const uint32_t *__restrict__ words, const WavFile &f, long long p) {
  if (f.fmt == XM_WAV_F64) {
    uint32_t a[2];
    wav_window<2>(words, p, f.kmin, f.kmax, a);
    return wav_f64(a[0], a[1]);
  }
  uint32_t a[1];
  wav_window<1>(words, p, f.kmin, f.kmax, a);
  switch (f.fmt) {
    case XM_WAV_U8: return wav_u8(a[0]);
    case XM_WAV_S16: return wav_s16(a[0]);
    case XM_WAV_S24: return wav_s24(a[0]);
    case XM_WAV_S32: return wav_s32(a[0]);
    default: return a[0];
  }
}

// four consecutive samples of a mono file starting at byte p
__device__ __forceinline__ uint4 wav_four(const uint32_t *__restrict__ words, const WavFile &f, long long p) {
  switch (f.fmt) {
    case XM_WAV_U8: {
      uint32_t a[1];
      wav_window<1>(words, p, f.kmin, f.kmax, a);
      return make_uint4(wav_u8(a[0]), wav_u8(a[0] >> 8), wav_u8(a[0] >> 16), wav_u8(a[0] >> 24));
    }
    case XM_WAV_S16: {
      uint32_t a[2];
      wav_window<2>(words, p, f.kmin, f.kmax, a);
      return make_uint4(wav_s16(a[0]), wav_s16(a[0] >> 16), wav_s16(a[1]), wav_s16(a[1] >> 16));
    }
    case XM_WAV_S24: {
      uint32_t a[3];
      wav_window<3>(words, p, f.kmin, f.kmax, a);
      return make_uint4(wav_s24(a[0]), wav_s24((a[0] >> 24) | (a[1] << 8)), wav_s24((a[1] >> 16) | (a[2] << 16)), wav_s24(a[2] >> 8));
    }
    case XM_WAV_S32: {
      uint32_t a[4];
      wav_window<4>(words, p, f.kmin, f.kmax, a);
      return make_uint4(wav_s32(a[0]), wav_s32(a[1]), wav_s32(a[2]), wav_s32(a[3]));
    }
    case XM_WAV_F32: {
      uint32_t a[4];
      wav_window<4>(words, p, f.kmin, f.kmax, a);
      return make_uint4(a[0], a[1], a[2], a[3]);
    }
    default: {
      uint32_t a[8];
      wav_window<8>(words, p, f.kmin, f.kmax, a);
      return make_uint4(wav_f64(a[0], a[1]), wav_f64(a[2], a[3]), wav_f64(a[4], a[5]), wav_f64(a[6], a[7]));
    }
  }
}

// byte position of output float `rel` of the file: frames x channels-written, channel c at + c frames
__device__ __forceinline__ long long wav_pos(const WavFile &f, long long rel) {
  long long c = 0, fr = rel;
  if (f.cw > 1) {
    c = (long long)((unsigned long long)rel / (unsigned long long)max(f.frames, 1LL));
    fr = rel - c * f.frames;
  }
  const long long src = f.sel >= 0 ? f.sel : c;
  return f.begin + (fr * f.nch + src) * f.bps;
}

__global__ void __launch_bounds__(256)
wav_decode_kernel(const uint32_t *__restrict__ words, long long nbytes, const long long *__restrict__ desc, int N,
                  uint32_t *__restrict__ out, long long out_floats) {
  // the batch's output range, inside [0, out_floats)
  const long long lo = min(max(desc[WD_OUT], 0LL), out_floats);
  const long long *dl = desc + (long long)(N - 1) * kWavDesc;
  const long long hi = min(max(dl[WD_OUT] + max(dl[WD_FRAMES], 0LL) * min(max(dl[WD_CW], 1LL), 64LL), lo), out_floats);
  if (hi <= lo) return;
  const long long mis = (long long)(((uintptr_t)out >> 2) & 3);      // piece q holds floats 4 q - mis .. 4 q - mis + 3
  const long long qlo = (lo + mis) >> 2, qhi = (hi - 1 + mis) >> 2;
  const long long ntiles = (qhi - qlo + 256 * kWavQuads) / (256 * kWavQuads);
  WavFile f;
  f.out = 0;
  f.count = -1;                                                      // nothing cached
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long q0 = qlo + t * (256 * kWavQuads);
    // block-uniform: the files of the tile's first and last float
    const long long ta = max(4 * q0 - mis, lo), tb = min(4 * (q0 + 256 * kWavQuads) - mis, hi) - 1;
    const int i0 = wav_find(desc, 0, N - 1, ta), i1 = wav_find(desc, i0, N - 1, max(tb, ta));
#pragma unroll
    for (int k = 0; k < kWavQuads; ++k) {
      const long long q = q0 + k * 256 + threadIdx.x;
      const long long a0 = 4 * q - mis;
      const long long first = max(a0, lo), last = min(a0 + 3, hi - 1);
      if (first > last) continue;
      if (!(first >= f.out && first - f.out < f.count)) f = wav_file(desc, wav_find(desc, i0, i1, first), nbytes);
      const long long rel = a0 - f.out;
      if (a0 >= lo && a0 + 3 < hi && rel >= 0 && rel + 3 < f.count) {
        uint4 v;
        if (f.nch == 1) {
          v = wav_four(words, f, f.begin + rel * f.bps);
        } else if (f.cw == 1 || (unsigned long long)rel % (unsigned long long)f.frames + 3 < (unsigned long long)f.frames) {
          // four frames of one channel: a constant stride in the file
          const long long p = wav_pos(f, rel), step = (long long)f.nch * f.bps;
          v = make_uint4(wav_sample(words, f, p), wav_sample(words, f, p + step), wav_sample(words, f, p + 2 * step),
                         wav_sample(words, f, p + 3 * step));
        } else {
          v = make_uint4(wav_sample(words, f, wav_pos(f, rel)), wav_sample(words, f, wav_pos(f, rel + 1)),
                         wav_sample(words, f, wav_pos(f, rel + 2)), wav_sample(words, f, wav_pos(f, rel + 3)));
        }
        *(uint4 *)(out + a0) = v;
      } else {
        for (long long a = first; a <= last; ++a) {
          if (!(a >= f.out && a - f.out < f.count)) f = wav_file(desc, wav_find(desc, i0, i1, a), nbytes);
          const long long r = a - f.out;
          out[a] = (r >= 0 && r < f.count) ? wav_sample(words, f, wav_pos(f, r)) : 0u;
        }
      }
    }
  }
}

// ---- decode and resample in one pass (xm_wav_decode_resample_batch) -----------------------------------------------
// The plan's slots 14, 15 hold p, q = fs / SampleRate reduced; file i takes ceil(frames p / q) floats per channel written
// and output j of a channel is gain sum_k u(j q - k p) x[k] over the decoded frames 0 <= k < frames (wav_resample.h; the
// tap loop is wav_batch_kernel's, k descending, so the bits are those of xm_wav_batch on the decoded bank).  The work is
// laid out by the OUTPUT as above: tiles of kWavRateTile output floats, the files of a tile found by bisection.  Inside a
// tile the block walks the pieces (file, channel) and cuts each into runs of outputs whose source window -- at most
// (n - 1) q / p + 20 max(p, q) / p + 1 frames for n outputs -- fits the kWavRateWin frames of LDS: the window is decoded
// into LDS once and every tap reads it there.  p == q copies the decoded sample.  Every loop bound around a barrier is
// block-uniform; a ratio outside the plan's bounds is treated as 1 / 1, so a forged descriptor cannot widen the window.
constexpr int kWavRateTile = 2048;                  // output floats per tile
constexpr int kWavRateWin = 4096;                   // source frames of one channel held in LDS (16 KB)
static_assert(kWavPlanMaxRatio == kWavMaxRatio, "the plan refuses what xm_wav_batch's taps cannot take");
static_assert(kWavRateWin - 1 >= 20 * kWavPlanMaxStep, "the window of a run of one output fits LDS at the steepest ratio");

// wav_file with the resampled counts: p, q of the plan (1, 1 when unusable), frames per channel written at the new rate
__device__ __forceinline__ WavFile wav_rate_file(const long long *__restrict__ desc, int i, long long nbytes, int &p, int &q,
                                                 long long &oframes) {
  WavFile f = wav_file(desc, i, nbytes);
  const long long *d = desc + (long long)i * kWavDesc;
  long long pp = d[WD_P], qq = d[WD_Q];
  if (pp < 1 || qq < 1 || pp > kWavPlanMaxRatio || qq > kWavPlanMaxRatio || qq > kWavPlanMaxStep * pp || pp > kWavPlanMaxStep * qq)
    pp = qq = 1;
  f.frames = min(f.frames, 1LL << 32);
  p = (int)pp;
  q = (int)qq;
  oframes = (f.frames * pp + qq - 1) / qq;
  f.count = oframes * f.cw;
  return f;
}

__global__ void __launch_bounds__(1024)
wav_rate_gain_kernel(const long long *__restrict__ desc, WavClip *__restrict__ clip) {
  const int n = blockIdx.x;
  const long long *d = desc + (long long)n * kWavDesc;
  wav_gain_block(d[WD_P], d[WD_Q], clip, n);
}

__global__ void __launch_bounds__(256)
wav_resample_kernel(const uint32_t *__restrict__ words, long long nbytes, const long long *__restrict__ desc, int N,
                    const WavClip *__restrict__ clip, uint32_t *__restrict__ out, long long out_floats) {
  __shared__ uint32_t win[kWavRateWin];
  const int tid = threadIdx.x;
  // the batch's output range, inside [0, out_floats)
  const long long lo = min(max(desc[WD_OUT], 0LL), out_floats);
  long long hi;
  {
    int pl, ql;
    long long ol;
    const WavFile fl = wav_rate_file(desc, N - 1, nbytes, pl, ql, ol);
    hi = min(max(fl.out + fl.count, lo), out_floats);
  }
  if (hi <= lo) return;
  const long long ntiles = (hi - lo + kWavRateTile - 1) / kWavRateTile;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long ta = lo + t * kWavRateTile, tb = min(ta + kWavRateTile, hi);
    const int i0 = wav_find(desc, 0, N - 1, ta), i1 = wav_find(desc, i0, N - 1, tb - 1);
    for (int i = i0; i <= i1; ++i) {
      int p, q;
      long long oframes;
      const WavFile f = wav_rate_file(desc, i, nbytes, p, q, oframes);
      const long long a0 = max(ta, f.out), a1 = min(tb, f.out + f.count);
      if (f.count <= 0 || a0 >= a1) continue;                 // a file of 0 frames, or one outside this tile
      const float gain = p != q ? clip[i].gain : 1.f;
      const int P = p > q ? p : q, half = 10 * P;
      // outputs per run: (n - 1) q + 2 half <= (kWavRateWin - 1) p, whole passes of the block where it can be
      long long run = ((long long)(kWavRateWin - 1) * p - 2LL * half) / q + 1;
      run = min(max(run, 1LL), (long long)kWavRateTile);
      if (run >= 256) run &= ~255LL;
      const long long step = (long long)f.nch * f.bps;
      const long long c0 = (a0 - f.out) / oframes, c1 = (a1 - 1 - f.out) / oframes;
      for (long long c = c0; c <= c1; ++c) {
        const long long cbase = f.out + c * oframes;
        const long long jA = max(a0, cbase) - cbase, jB = min(a1, cbase + oframes) - cbase;
        const long long pbase = f.begin + (f.sel >= 0 ? f.sel : c) * f.bps;
        if (p == q) {                                          // the file's own rate: a copy of the decoded samples
          for (long long j = jA + tid; j < jB; j += 256) out[cbase + j] = wav_sample(words, f, pbase + j * step);
          continue;
        }
        for (long long j0 = jA; j0 < jB; j0 += run) {
          const long long n = min(run, jB - j0);
          // the window of the run: from the first tap of its first output to the last tap of its last, inside the file
          const unsigned long long top0 = (unsigned long long)j0 * (unsigned)q + (unsigned)half;
          const long long khi0 = (long long)(top0 / (unsigned)p);
          const long long kbase = max(khi0 - (2 * half - (int)(top0 - (unsigned long long)khi0 * (unsigned)p)) / p, 0LL);
          long long ktop = (long long)(((unsigned long long)(j0 + n - 1) * (unsigned)q + (unsigned)half) / (unsigned)p);
          ktop = min(min(ktop, f.frames - 1), kbase + kWavRateWin - 1);
          __syncthreads();                                     // the run before has been read
          for (long long k = kbase + tid; k <= ktop; k += 256) win[k - kbase] = wav_sample(words, f, pbase + k * step);
          __syncthreads();
          for (long long j = j0 + tid; j < j0 + n; j += 256) {
            const unsigned long long top = (unsigned long long)j * (unsigned)q + (unsigned)half;
            const long long khi = (long long)(top / (unsigned)p);      // largest k with j q - k p >= -half
            const int rem = (int)(top - (unsigned long long)khi * (unsigned)p);
            const long long klo = khi - (2 * half - rem) / p;          // smallest k with j q - k p <= half
            const long long k1 = khi < ktop ? khi : ktop, k0 = klo > kbase ? klo : kbase;
            float v = 0.f;
            if (k1 >= k0) {
              int m = rem - half + (int)((khi - k1) * p);              // j q - k1 p
              const int qd = (m + half) / P;                           // floor(m / P) + 10
              int r = m + half - qd * P, odd = qd & 1;
              const float invP = 1.f / (float)P, P_over_pi = (float)P * 0.318309886f,
                          kb = kWavBeta2Over4 / ((float)half * (float)half);
              float acc = 0.f;
              for (int k = (int)(k1 - kbase); k >= (int)(k0 - kbase); --k) {
                acc = fmaf(wav_tap(m, r, odd, P, invP, P_over_pi, half, kb), __uint_as_float(win[k]), acc);
                m += p;
                r += p;
                if (r >= P) {
                  r -= P;
                  odd ^= 1;
                }
              }
              v = acc * gain;
            }
            out[cbase + j] = __float_as_uint(v);
          }
        }
      }
    }
  }
}

}  // namespace xm

using namespace xm;

extern "C" {

int xm_wav_plan_fs(const unsigned char *bytes, const long long *offsets, int N, const long long *ranges, int channel,
                   long long fs, long long out_base, long long *desc, long long *sizes) {
  char msg[256];
  msg[0] = 0;
  const int rc = wav_plan_batch_fs(bytes, offsets, N, ranges, channel, fs, out_base, desc, sizes, msg, (int)sizeof msg);
  return rc ? fail(rc, "%s", msg) : XM_OK;
}

int xm_wav_resample_geometry(int *tile, int *launches) {
  if (tile) *tile = kWavRateTile;
  if (launches) *launches = 2;
  return XM_OK;
}

int xm_wav_decode_resample_batch(const unsigned char *bytes, long long nbytes, const long long *desc, int N, float *out,
                                 long long out_floats, void *stream) {
  if (N < 0 || nbytes < 0 || out_floats < 0)
    return fail(XM_EINVAL, "wav_decode_resample_batch: need N >= 0, nbytes >= 0, out_floats >= 0 (got N=%d nbytes=%lld out_floats=%lld)",
                N, nbytes, out_floats);
  if (N == 0) return XM_OK;
  if (!bytes || !desc || !out) return fail(XM_EINVAL, "wav_decode_resample_batch: NULL argument");
  if (((uintptr_t)bytes & 15) || ((uintptr_t)desc & 7) || ((uintptr_t)out & 3))
    return fail(XM_EINVAL, "wav_decode_resample_batch: bytes must be 16-byte aligned, desc 8-byte and out 4-byte aligned");
  if (nbytes == 0 || out_floats == 0) return XM_OK;   // no data chunk holds a byte: nothing to write
  hipStream_t st = (hipStream_t)stream;
  void *ws = nullptr;
  const int rc = ws_get((size_t)N * sizeof(WavClip), &ws, st);
  if (rc != XM_OK) return rc;
  {
    ProfScope ps(prof_key(kProfWavRate, 0), 0, st);
    hipLaunchKernelGGL(wav_rate_gain_kernel, dim3((unsigned)N), dim3(1024), 0, st, desc, (WavClip *)ws);
    XM_LAUNCH_CHECK();
  }
  const long long tiles = (out_floats + kWavRateTile - 1) / kWavRateTile;   // an upper bound of the kernel's tile count
  ProfScope ps(prof_key(kProfWavRate, 1), 0, st);
  hipLaunchKernelGGL(wav_resample_kernel, dim3((unsigned)std::min<long long>(tiles, kWavMaxBlocks)), dim3(256), 0, st,
                     (const uint32_t *)bytes, nbytes, desc, N, (const WavClip *)ws, (uint32_t *)out, out_floats);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_wav_plan(const unsigned char *bytes, const long long *offsets, int N, const long long *ranges, int channel,
                long long out_base, long long *desc, long long *sizes) {
  char msg[256];
  msg[0] = 0;
  const int rc = wav_plan_batch(bytes, offsets, N, ranges, channel, out_base, desc, sizes, msg, (int)sizeof msg);
  return rc ? fail(rc, "%s", msg) : XM_OK;
}

int xm_wav_decode_batch(const unsigned char *bytes, long long nbytes, const long long *desc, int N, float *out,
                        long long out_floats, void *stream) {
  if (N < 0 || nbytes < 0 || out_floats < 0)
    return fail(XM_EINVAL, "wav_decode_batch: need N >= 0, nbytes >= 0, out_floats >= 0 (got N=%d nbytes=%lld out_floats=%lld)", N,
                nbytes, out_floats);
  if (N == 0) return XM_OK;
  if (!bytes || !desc || !out) return fail(XM_EINVAL, "wav_decode_batch: NULL argument");
  if (((uintptr_t)bytes & 15) || ((uintptr_t)desc & 7) || ((uintptr_t)out & 3))
    return fail(XM_EINVAL, "wav_decode_batch: bytes must be 16-byte aligned, desc 8-byte and out 4-byte aligned");
  if (nbytes == 0 || out_floats == 0) return XM_OK;   // no data chunk holds a byte: nothing to write
  hipStream_t st = (hipStream_t)stream;
  const long long tiles = (out_floats + 6 + kWavTile) / kWavTile;     // an upper bound of the kernel's tile count
  ProfScope ps(prof_key(kProfWav), 0, st);
  hipLaunchKernelGGL(wav_decode_kernel, dim3((unsigned)std::min<long long>(tiles, kWavMaxBlocks)), dim3(256), 0, st,
                     (const uint32_t *)bytes, nbytes, desc, N, (uint32_t *)out, out_floats);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

}  // extern "C"

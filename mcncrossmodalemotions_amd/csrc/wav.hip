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
#include <algorithm>

#include "prof.h"
#include "wav_plan.h"
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

}  // namespace xm

using namespace xm;

extern "C" {

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

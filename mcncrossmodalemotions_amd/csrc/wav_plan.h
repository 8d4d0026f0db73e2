// Host-side planning of vl.audioread: the RIFF / WAVE parse of a batch of files and the layout of their samples in the
// waveform bank -- what audioinfo reports (getBatchEmoVoxCeleb.m:79) plus where audioread's samples go.  Byte arithmetic
// only, nothing from HIP (compiles with g++ -std=c++17; tests/wav_plan_check.cpp parses every truncation and
// single-byte mutation of a valid file per format under the address and undefined-behaviour sanitizers).
// include/xmodal.h documents the descriptor row; csrc/wav.hip holds the C entry point and the device decode.
// wav_plan_batch_fs is the same plan towards one sample rate (xm_wav_plan_fs: p / q = fs / SampleRate per file, output
// offsets at that rate); tests/wav_rate_plan_check.cpp does for it what wav_plan_check.cpp does for wav_plan_batch.
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/xmodal.h"

namespace xm {

// descriptor columns (XM_WAV_DESC int64 per file)
enum { WD_BEGIN = 0, WD_END, WD_RATE, WD_NCH, WD_BITS, WD_FMT, WD_TOTAL, WD_FIRST, WD_FRAMES, WD_CW, WD_SEL, WD_OUT,
       WD_STATUS, WD_ALIGN, WD_P, WD_Q };

// xm_wav_plan_fs: the reduced ratio p / q = fs / SampleRate a file may have.  kWavPlanMaxRatio is xm_wav_batch's limit
// (kWavMaxRatio, wav_resample.h); kWavPlanMaxStep bounds the tap loop (20 max(p, q) / p + 1 taps per output) and the
// window of source frames a tile of the decode-and-resample kernel holds in LDS.
constexpr long long kWavPlanMaxRatio = 1 << 20;
constexpr long long kWavPlanMaxStep = 16;

struct WavInfo {
  long long begin = 0, end = 0;   // byte range of the sample data inside the file, clamped to it
  long long rate = 0, nch = 0, bits = 0, fmt = 0, align = 0, total = 0, status = 0;
};

static inline int wav_fail(char *err, int errlen, int code, const char *fmt, ...) {
  if (err && errlen > 0) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, (size_t)errlen, fmt, ap);
    va_end(ap);
  }
  return code;
}

static inline uint32_t wav_u16(const unsigned char *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
static inline uint32_t wav_u32(const unsigned char *p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
static inline bool wav_tag(const unsigned char *p, const char *t) {
  return p[0] == (unsigned char)t[0] && p[1] == (unsigned char)t[1] && p[2] == (unsigned char)t[2] && p[3] == (unsigned char)t[3];
}

// one file of n bytes at d.  XM_OK, or XM_EINVAL (malformed) / XM_ENOTSUP (a valid file this build does not decode) with
// a message that names the file's index.
static inline int wav_parse_one(int idx, const unsigned char *d, long long n, WavInfo &w, char *err, int errlen) {
#define WBAD(...) return wav_fail(err, errlen, XM_EINVAL, __VA_ARGS__)
#define WNOT(...) return wav_fail(err, errlen, XM_ENOTSUP, __VA_ARGS__)
  if (n >= 4 && (wav_tag(d, "RF64") || wav_tag(d, "BW64"))) WNOT("wav_plan: file %d: RF64 / BW64 containers are not supported", idx);
  if (n >= 4 && wav_tag(d, "RIFX")) WNOT("wav_plan: file %d: big-endian RIFX containers are not supported", idx);
  if (n < 12 || !wav_tag(d, "RIFF") || !wav_tag(d + 8, "WAVE")) WBAD("wav_plan: file %d: not a RIFF / WAVE file", idx);
  bool have_fmt = false;
  long long pos = 12;
  for (;;) {
    if (pos == n) WBAD("wav_plan: file %d: no data chunk", idx);
    if (n - pos < 8) WBAD("wav_plan: file %d: cut inside a chunk header at byte %lld", idx, pos);
    const unsigned char *c = d + pos;
    const long long size = (long long)wav_u32(c + 4), body = pos + 8;
    if (wav_tag(c, "data")) {
      if (!have_fmt) WBAD("wav_plan: file %d: the data chunk comes before the fmt chunk", idx);
      w.begin = body;
      w.end = body + size;
      if (w.end > n) {   // a streamed writer's 0xFFFFFFFF, or a file cut short: decode what is there
        w.end = n;
        w.status |= XM_WAV_TRUNCATED;
      }
      w.total = (w.end - w.begin) / w.align;   // a trailing partial frame is dropped
      return XM_OK;
    }
    if (wav_tag(c, "fmt ") && !have_fmt) {
      if (size < 16) WBAD("wav_plan: file %d: fmt chunk of %lld bytes, at least 16 are required", idx, size);
      if (n - body < size) WBAD("wav_plan: file %d: cut inside the fmt chunk", idx);
      const unsigned char *f = d + body;
      uint32_t tag = wav_u16(f);
      w.nch = wav_u16(f + 2);
      w.rate = wav_u32(f + 4);
      w.align = wav_u16(f + 12);
      w.bits = wav_u16(f + 14);
      if (tag == 0xFFFE) {   // WAVE_FORMAT_EXTENSIBLE: cbSize >= 22, valid bits, channel mask, SubFormat GUID
        if (size < 40 || wav_u16(f + 16) < 22) WBAD("wav_plan: file %d: extensible fmt chunk of %lld bytes, 40 are required", idx, size);
        static const unsigned char tail[14] = {0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71};
        for (int k = 0; k < 14; ++k)
          if (f[26 + k] != tail[k]) WNOT("wav_plan: file %d: extensible SubFormat is not a KSDATAFORMAT_SUBTYPE of a wave format tag", idx);
        const uint32_t valid = wav_u16(f + 18);
        tag = wav_u16(f + 24);
        if (tag != 1 && tag != 3) WNOT("wav_plan: file %d: extensible SubFormat tag 0x%04X (only PCM and IEEE float are decoded)", idx, tag);
        if (valid != (uint32_t)w.bits)
          WNOT("wav_plan: file %d: %u valid bits in a %lld-bit container are not supported", idx, valid, w.bits);
      }
      if (tag == 1) {
        w.fmt = w.bits == 8 ? XM_WAV_U8 : w.bits == 16 ? XM_WAV_S16 : w.bits == 24 ? XM_WAV_S24 : w.bits == 32 ? XM_WAV_S32 : -1;
      } else if (tag == 3) {
        w.fmt = w.bits == 32 ? XM_WAV_F32 : w.bits == 64 ? XM_WAV_F64 : -1;
      } else {
        WNOT("wav_plan: file %d: format tag 0x%04X (A-law, mu-law, ADPCM, MPEG ... are not decoded; only PCM and IEEE float)", idx, tag);
      }
      if (w.fmt < 0) WNOT("wav_plan: file %d: %lld bits per sample with format tag %u are not supported", idx, w.bits, tag);
      if (w.nch < 1 || w.rate < 1) WBAD("wav_plan: file %d: %lld channels at %lld Hz", idx, w.nch, w.rate);
      if (w.nch > 64) WNOT("wav_plan: file %d: %lld channels, at most 64 are supported", idx, w.nch);
      if (w.align != w.nch * w.bits / 8)
        WBAD("wav_plan: file %d: block align %lld, %lld channels of %lld bits need %lld", idx, w.align, w.nch, w.bits, w.nch * w.bits / 8);
      have_fmt = true;
    }
    // any other chunk (LIST, fact, bext, a second fmt ...) is skipped, with the pad byte after an odd size
    const long long next = body + size + (size & 1);
    if (next > n) WBAD("wav_plan: file %d: no data chunk (a %c%c%c%c chunk runs past the end of the file)", idx,
                       c[0] >= 32 && c[0] < 127 ? c[0] : '?', c[1] >= 32 && c[1] < 127 ? c[1] : '?',
                       c[2] >= 32 && c[2] < 127 ? c[2] : '?', c[3] >= 32 && c[3] < 127 ? c[3] : '?');
    pos = next;
  }
#undef WBAD
#undef WNOT
}

// the batch: file i is bytes[offsets[i] .. offsets[i + 1]); ranges (optional) N x 2 1-based inclusive [first last],
// last == -1: to the end; channel -1: all channels, c >= 0: that one; out_base: first float of the batch in the bank.
// Writes N rows of XM_WAV_DESC int64 and sizes = {output floats, N}.
// fs == 0: the files' own rates (xm_wav_plan).  fs >= 1 (xm_wav_plan_fs): every file resampled to fs -- p, q = fs /
// SampleRate reduced go to slots 14, 15 and a file takes ceil(frames p / q) output floats per channel written.
static inline int wav_plan_batch_rate(const unsigned char *bytes, const long long *offsets, int N, const long long *ranges,
                                      int channel, long long fs, long long out_base, long long *desc, long long *sizes, char *err,
                                      int errlen) {
  if (N < 0 || out_base < 0 || channel < -1)
    return wav_fail(err, errlen, XM_EINVAL, "wav_plan: need N >= 0, out_base >= 0, channel >= -1 (got N=%d out_base=%lld channel=%d)", N,
                    out_base, channel);
  if (!sizes) return wav_fail(err, errlen, XM_EINVAL, "wav_plan: NULL sizes");
  sizes[0] = 0;
  sizes[1] = 0;
  if (N == 0) return XM_OK;
  if (!bytes || !offsets || !desc) return wav_fail(err, errlen, XM_EINVAL, "wav_plan: NULL argument");
  long long out = out_base;
  for (int i = 0; i < N; ++i) {
    if (offsets[i] < 0 || offsets[i + 1] < offsets[i] || (i == 0 && offsets[0] != 0))
      return wav_fail(err, errlen, XM_EINVAL, "wav_plan: file %d: offsets must ascend from 0", i);
    WavInfo w;
    const int rc = wav_parse_one(i, bytes + offsets[i], offsets[i + 1] - offsets[i], w, err, errlen);
    if (rc) return rc;
    long long first = 0, frames = w.total;
    if (ranges) {
      const long long a = ranges[2 * i], b = ranges[2 * i + 1] == -1 ? w.total : ranges[2 * i + 1];
      if (a < 1 || b > w.total || a > b)
        return wav_fail(err, errlen, XM_EINVAL, "wav_plan: file %d: range [%lld %lld] is outside 1..%lld or empty", i, ranges[2 * i],
                        ranges[2 * i + 1], w.total);
      first = a - 1;
      frames = b - a + 1;
    }
    if (channel >= w.nch)
      return wav_fail(err, errlen, XM_EINVAL, "wav_plan: file %d: channel %d of a file with %lld channels", i, channel, w.nch);
    const long long cw = channel >= 0 ? 1 : w.nch;
    long long *d = desc + (long long)i * XM_WAV_DESC;
    for (int k = 0; k < XM_WAV_DESC; ++k) d[k] = 0;
    d[WD_BEGIN] = offsets[i] + w.begin;
    d[WD_END] = offsets[i] + w.end;
    d[WD_RATE] = w.rate;
    d[WD_NCH] = w.nch;
    d[WD_BITS] = w.bits;
    d[WD_FMT] = w.fmt;
    d[WD_TOTAL] = w.total;
    d[WD_FIRST] = first;
    d[WD_FRAMES] = frames;
    d[WD_CW] = cw;
    d[WD_SEL] = channel;
    d[WD_OUT] = out;
    d[WD_STATUS] = w.status;
    d[WD_ALIGN] = w.align;
    long long oframes = frames;
    if (fs > 0) {
      long long a = fs, b = w.rate;
      while (b) {
        const long long t = a % b;
        a = b;
        b = t;
      }
      const long long p = fs / a, q = w.rate / a;
      if (p > kWavPlanMaxRatio || q > kWavPlanMaxRatio)
        return wav_fail(err, errlen, XM_ENOTSUP, "wav_plan: file %d: %lld Hz to %lld Hz is the ratio %lld / %lld, terms above 2^20 are not supported",
                        i, w.rate, fs, p, q);
      if (q > kWavPlanMaxStep * p)
        return wav_fail(err, errlen, XM_ENOTSUP, "wav_plan: file %d: %lld Hz to %lld Hz is below 1 / 16 of the file's rate", i, w.rate, fs);
      if (p > kWavPlanMaxStep * q)
        return wav_fail(err, errlen, XM_ENOTSUP, "wav_plan: file %d: %lld Hz to %lld Hz is above 16 times the file's rate", i, w.rate, fs);
      d[WD_P] = p;
      d[WD_Q] = q;
      oframes = (frames * p + q - 1) / q;     // frames < 2^32 and p <= 2^20
    }
    out += oframes * cw;
  }
  sizes[0] = out - out_base;
  sizes[1] = N;
  return XM_OK;
}

static inline int wav_plan_batch(const unsigned char *bytes, const long long *offsets, int N, const long long *ranges, int channel,
                                 long long out_base, long long *desc, long long *sizes, char *err, int errlen) {
  return wav_plan_batch_rate(bytes, offsets, N, ranges, channel, 0, out_base, desc, sizes, err, errlen);
}

static inline int wav_plan_batch_fs(const unsigned char *bytes, const long long *offsets, int N, const long long *ranges, int channel,
                                    long long fs, long long out_base, long long *desc, long long *sizes, char *err, int errlen) {
  if (fs < 1) return wav_fail(err, errlen, XM_EINVAL, "wav_plan: need fs >= 1 (got %lld)", fs);
  return wav_plan_batch_rate(bytes, offsets, N, ranges, channel, fs, out_base, desc, sizes, err, errlen);
}

}  // namespace xm

// Host-side planning of vl.pixcsv_decode: the line / field parse of a FER2013-style CSV whose `pixels` column holds an
// image as space-separated decimal numbers (imdb = getFerPlusImdb(opts.dataDir), ferplus_baselines.m:106).  It finds
// where every row's pixel field lies and reads the two small columns next to it; the numbers themselves are parsed on
// the device (csrc/pixcsv.hip).  Byte arithmetic only, nothing from HIP (compiles with g++ -std=c++17;
// tests/pixcsv_plan_check.cpp plans every truncation and single-byte mutation of a small file under the address and
// undefined-behaviour sanitizers).  include/xmodal.h documents the rules and the descriptor row.
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/xmodal.h"

namespace xm {

// descriptor columns (XM_PIX_DESC int64 per row)
enum { PD_BEGIN = 0, PD_END, PD_EMOTION, PD_USAGE, PD_LINE, PD_OUT };
constexpr int kPixMaxCols = 64;   // columns looked at in a line; later ones are skipped over

static inline int pix_fail(char *err, int errlen, int code, const char *fmt, ...) {
  if (err && errlen > 0) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, (size_t)errlen, fmt, ap);
    va_end(ap);
  }
  return code;
}

// [a, b) without one pair of enclosing double quotes and without blanks around what is left
static inline void pix_trim(const unsigned char *d, long long &a, long long &b, bool blanks) {
  if (b - a >= 2 && d[a] == '"' && d[b - 1] == '"') {
    ++a;
    --b;
  }
  if (!blanks) return;
  while (a < b && (d[a] == ' ' || d[a] == '\t')) ++a;
  while (b > a && (d[b - 1] == ' ' || d[b - 1] == '\t')) --b;
}

static inline bool pix_is(const unsigned char *d, long long a, long long b, const char *name) {
  long long k = 0;
  for (; a + k < b && name[k]; ++k)
    if (d[a + k] != (unsigned char)name[k]) return false;
  return a + k == b && !name[k];
}

// the fields of the line [a, b): split at commas outside double quotes.  Returns the number of fields (all of them are
// counted, the first kPixMaxCols are stored), or -1 when a quote is still open at the end of the line.
static inline long long pix_split(const unsigned char *d, long long a, long long b, long long (*f)[2]) {
  long long n = 0, start = a;
  bool quoted = false;
  for (long long p = a; p <= b; ++p) {
    if (p < b && d[p] == '"') quoted = !quoted;
    if (p == b || (d[p] == ',' && !quoted)) {
      if (n < kPixMaxCols) {
        f[n][0] = start;
        f[n][1] = p;
      }
      ++n;
      start = p + 1;
    }
  }
  return quoted ? -1 : n;
}

// desc == nullptr: count only (max_rows is not looked at).  sizes = {rows, longest pixel field in bytes}.
static inline int pixcsv_plan(const unsigned char *bytes, long long nbytes, long long *desc, long long max_rows, long long *sizes,
                              char *err, int errlen) {
  if (!sizes) return pix_fail(err, errlen, XM_EINVAL, "pixcsv_plan: NULL sizes");
  sizes[0] = 0;
  sizes[1] = 0;
  if (nbytes < 0 || (desc && max_rows < 0))
    return pix_fail(err, errlen, XM_EINVAL, "pixcsv_plan: need nbytes >= 0 and max_rows >= 0 (got %lld, %lld)", nbytes, max_rows);
  if (nbytes == 0) return XM_OK;
  if (!bytes) return pix_fail(err, errlen, XM_EINVAL, "pixcsv_plan: NULL bytes");
  long long pos = 0, line = 0, rows = 0, longest = 0;
  if (nbytes >= 3 && bytes[0] == 0xEF && bytes[1] == 0xBB && bytes[2] == 0xBF) pos = 3;   // UTF-8 byte order mark
  int c_emotion = 0, c_pixels = 1, c_usage = 2;   // the columns of a file without a header: emotion,pixels,Usage
  long long ncols = 3;
  bool first = true;
  long long f[kPixMaxCols][2];
  while (pos < nbytes) {
    const void *nl = memchr(bytes + pos, '\n', (size_t)(nbytes - pos));
    const long long eol = nl ? (long long)((const unsigned char *)nl - bytes) : nbytes;
    const long long next = eol < nbytes ? eol + 1 : eol;
    long long b = eol;
    if (b > pos && bytes[b - 1] == '\r') --b;   // CRLF
    const long long a = pos;
    pos = next;
    ++line;
    if (a == b) continue;                        // an empty line
    const long long nf = pix_split(bytes, a, b, f);
    if (nf < 0) return pix_fail(err, errlen, XM_EINVAL, "pixcsv_plan: line %lld: unterminated quote", line);
    if (first) {
      first = false;
      if (!(bytes[a] >= '0' && bytes[a] <= '9')) {   // a header: the columns are found by name
        c_emotion = c_pixels = c_usage = -1;
        ncols = nf;
        for (long long k = 0; k < nf && k < kPixMaxCols; ++k) {
          long long u = f[k][0], v = f[k][1];
          pix_trim(bytes, u, v, true);
          if (c_pixels < 0 && pix_is(bytes, u, v, "pixels")) c_pixels = (int)k;
          else if (c_emotion < 0 && pix_is(bytes, u, v, "emotion")) c_emotion = (int)k;
          else if (c_usage < 0 && pix_is(bytes, u, v, "Usage")) c_usage = (int)k;
        }
        if (c_pixels < 0) return pix_fail(err, errlen, XM_EINVAL, "pixcsv_plan: line %lld: the header has no pixels column", line);
        continue;
      }
    }
    if (nf < ncols)
      return pix_fail(err, errlen, XM_EINVAL, "pixcsv_plan: line %lld: %lld fields, the header has %lld", line, nf, ncols);
    long long pa = f[c_pixels][0], pb = f[c_pixels][1];
    pix_trim(bytes, pa, pb, false);
    if (desc) {
      if (rows >= max_rows) return pix_fail(err, errlen, XM_EINVAL, "pixcsv_plan: line %lld: more rows than max_rows = %lld", line, max_rows);
      long long emotion = -1, usage = -1;
      if (c_emotion >= 0) {
        long long u = f[c_emotion][0], v = f[c_emotion][1];
        pix_trim(bytes, u, v, true);
        if (v > u && v - u <= 9) {               // up to nine decimal digits; anything else counts as absent
          emotion = 0;
          for (long long k = u; k < v; ++k) {
            if (bytes[k] < '0' || bytes[k] > '9') {
              emotion = -1;
              break;
            }
            emotion = emotion * 10 + (bytes[k] - '0');
          }
        }
      }
      if (c_usage >= 0) {
        long long u = f[c_usage][0], v = f[c_usage][1];
        pix_trim(bytes, u, v, true);
        usage = pix_is(bytes, u, v, "Training") ? 0 : pix_is(bytes, u, v, "PublicTest") ? 1 : pix_is(bytes, u, v, "PrivateTest") ? 2 : -1;
      }
      long long *d = desc + rows * XM_PIX_DESC;
      for (int k = 0; k < XM_PIX_DESC; ++k) d[k] = 0;
      d[PD_BEGIN] = pa;
      d[PD_END] = pb;
      d[PD_EMOTION] = emotion;
      d[PD_USAGE] = usage;
      d[PD_LINE] = line;
      d[PD_OUT] = rows;
    }
    if (pb - pa > longest) longest = pb - pa;
    ++rows;
  }
  sizes[0] = rows;
  sizes[1] = longest;
  return XM_OK;
}

}  // namespace xm

// Host-side planning of vl.imreadjpeg(progressive=True): the header and scan-script parse of a batch of JPEG files that
// may be progressive (SOF2) as well as baseline (SOF0).  It walks every file marker by marker, checks each scan against
// T.81 G.1.1.1.1, gives it a level (the launch of the entropy stage it runs in) and a raster, splits its entropy data at
// the RSTn markers into lanes and takes the Huffman tables as they stand at that scan.  Byte arithmetic only, nothing
// from HIP (compiles with g++ -std=c++17); the device side is csrc/jpeg_prog.hip.  include/xmodal.h documents the
// descriptor, scan, lane and table layouts.  The layout constants, the zigzag order and the two table helpers are
// shared with xm_jpeg_plan (csrc/jpeg.hip).
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/xmodal.h"

namespace xm {

constexpr int kJpegDesc = XM_JPEG_DESC, kJpegLane = XM_JPEG_LANE, kJpegScan = XM_JPEG_SCAN;
constexpr int kQtBytes = XM_JPEG_QT_BYTES, kHtBytes = XM_JPEG_HT_BYTES;
constexpr int kJpegMaxSide = 4096;   // H, W <= 4096
constexpr int kJpegMaxScans = XM_JPEG_MAX_SCANS;   // per file; libjpeg's standard scripts have 10 (colour) and 6 (grey)

// descriptor columns
enum { D_SCAN0 = 0, D_SCAN1, D_H, D_W, D_NCOMP, D_HS, D_VS, D_RI, D_MX, D_MY, D_QT, D_DC = 13, D_AC = 16, D_COEF = 19,
       D_PLANE, D_PIX, D_LANE0, D_NLANES };
// scan columns (XM_JPEG_SCAN int64 per (image, scan))
enum { S_IMG = 0, S_NS, S_COMP, S_SS = 5, S_SE, S_AH, S_AL, S_DC, S_AC = 12, S_B0 = 15, S_B1, S_BW, S_BH, S_LEVEL, S_LANE0,
       S_NLANES, S_RI, S_KIND };

static const unsigned char kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                           41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                           30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// jpeg_make_d_derived_tbl into the 1024-byte device form; false = invalid code lengths
static inline bool derive_table(const unsigned char *counts, const unsigned char *vals, int nvals, unsigned char *out) {
  memset(out, 0, kHtBytes);
  unsigned short *lut = (unsigned short *)out;
  unsigned char *hv = out + 512;
  int *maxcode = (int *)(out + 768), *valoff = (int *)(out + 836);
  int sizes[257], codes[257], n = 0;
  for (int l = 1; l <= 16; ++l)
    for (int i = 0; i < counts[l - 1]; ++i) sizes[n++] = l;
  if (n != nvals || n > 256) return false;
  int code = 0, si = n ? sizes[0] : 0, p = 0;
  while (p < n) {
    while (p < n && sizes[p] == si) codes[p++] = code++;
    if (code > (1 << si)) return false;
    code <<= 1;
    ++si;
  }
  p = 0;
  maxcode[0] = -1;
  for (int l = 1; l <= 16; ++l) {
    if (counts[l - 1]) {
      valoff[l] = p - codes[p];
      p += counts[l - 1];
      maxcode[l] = codes[p - 1];
    } else {
      maxcode[l] = -1;
    }
  }
  p = 0;
  for (int l = 1; l <= 8; ++l)
    for (int i = 0; i < counts[l - 1]; ++i, ++p) {
      const int look = codes[p] << (8 - l);
      for (int c = 0; c < (1 << (8 - l)); ++c) lut[look + c] = (unsigned short)((l << 8) | vals[p]);
    }
  memcpy(hv, vals, n);
  return true;
}

template <int B>
static inline int intern(std::vector<unsigned char> &pool, const unsigned char *t) {
  const int n = (int)(pool.size() / B);
  for (int i = 0; i < n; ++i)
    if (!memcmp(&pool[(size_t)i * B], t, B)) return i;
  pool.insert(pool.end(), t, t + B);
  return n;
}

// ---- xm_jpeg_plan_prog ---------------------------------------------------------------------------------------------
static inline int jpeg_scan_fail(char *err, int errlen, int code, const char *fmt, ...) {
  if (err && errlen > 0) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, (size_t)errlen, fmt, ap);
    va_end(ap);
  }
  return code;
}

struct JpegScanTables {   // what DQT / DHT have defined so far in the file
  bool hasq[4] = {false, false, false, false}, hash[2][4] = {{false, false, false, false}, {false, false, false, false}};
  unsigned short q[4][64];
  unsigned char h[2][4][kHtBytes];
};

struct JpegScanFile {   // one file while it is parsed
  int H = 0, W = 0, ncomp = 0, hs = 1, vs = 1, mx = 0, my = 0, ri0 = 0;
  bool progressive = false;
  int tq[3] = {0, 0, 0}, fid[3] = {0, 0, 0};
  int qslot[3] = {0, 0, 0}, dcslot[3] = {0, 0, 0}, acslot[3] = {0, 0, 0};
  int bits[3][64], level[3][64];   // per coefficient: Al of the last scan that sent it (-1: none yet) and that scan's level
  long long data0 = 0, data1 = 0;  // entropy data of the first scan .. of the last one
  int nscans = 0;
  bool smooth = false;             // libjpeg's block smoothing applies (jpeg_scan_smoothing)
};

// zigzag 0 .. 9 in row-major order: the coefficients libjpeg's block smoothing estimates
static const unsigned char kJpegSmoothPos[10] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24};

// jdcoefct.c smoothing_ok: a progressive file, the DC of every component sent, one of the coefficients 1 .. 9 (zigzag)
// of some component not yet exact, and none of the six quantiser entries the estimates always divide by zero
static inline bool jpeg_scan_smoothing(const JpegScanFile &im, const JpegScanTables &tb) {
  if (!im.progressive || im.nscans == 0) return false;
  bool useful = false;
  for (int c = 0; c < im.ncomp; ++c) {
    if (im.bits[c][0] < 0) return false;
    for (int z = 0; z < 6; ++z)
      if (tb.q[im.tq[c]][kJpegSmoothPos[z]] == 0) return false;
    for (int z = 1; z < 10; ++z) useful = useful || im.bits[c][z] != 0;
  }
  return useful;
}

// the end of the entropy data that starts at `pos`: the first marker that is neither a stuffed zero, a fill byte nor
// RSTn (n when there is none); the RSTn markers on the way go to `cuts`
static inline long long jpeg_scan_end(const unsigned char *d, long long n, long long pos, std::vector<long long> &cuts) {
  long long i = pos;
  while (i < n) {
    const unsigned char *f = (const unsigned char *)memchr(d + i, 0xFF, (size_t)(n - i));
    if (!f || f + 1 >= d + n) break;
    const long long j = f - d;
    const int b = d[j + 1];
    if (b == 0) {
      i = j + 2;
    } else if (b == 0xFF) {
      i = j + 1;
    } else if (b >= 0xD0 && b <= 0xD7) {
      cuts.push_back(j);
      i = j + 2;
    } else {
      return j;
    }
  }
  return n;
}

// Plans file `idx` (d[0 .. n), at `base` in the batch): appends its scan rows and lane rows, interns its tables and
// fills `im`.  scan0 is the batch-wide row of the file's first scan, lane0 that of its first lane.
static inline int jpeg_scan_parse(int idx, const unsigned char *d, long long n, long long base, JpegScanFile &im,
                                  JpegScanTables &tb, std::vector<unsigned char> &qpool, std::vector<unsigned char> &hpool,
                                  std::vector<long long> &scan_rows, std::vector<long long> &lane_rows,
                                  std::vector<long long> &cuts, int &levels, char *err, int errlen) {
#define JBAD(...) return jpeg_scan_fail(err, errlen, XM_EINVAL, __VA_ARGS__)
#define JNOT(...) return jpeg_scan_fail(err, errlen, XM_ENOTSUP, __VA_ARGS__)
  if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) JBAD("jpeg_plan_prog: file %d: no SOI marker", idx);
  for (int c = 0; c < 3; ++c)
    for (int k = 0; k < 64; ++k) im.bits[c][k] = im.level[c][k] = -1;
  long long pos = 2;
  bool have_frame = false;
  int adobe = -1, ri = 0;
  for (;;) {
    // a file that ends after one of its scans -- at EOI, or cut -- is whole as far as it goes
    const bool started = im.nscans > 0;
    if (pos + 2 > n) {
      if (started) break;
      JBAD("jpeg_plan_prog: file %d: cut inside its headers", idx);
    }
    if (d[pos] != 0xFF) {
      if (started) break;
      JBAD("jpeg_plan_prog: file %d: marker expected at byte %lld", idx, pos);
    }
    while (pos < n && d[pos] == 0xFF) ++pos;
    if (pos + 1 > n) {
      if (started) break;
      JBAD("jpeg_plan_prog: file %d: cut inside its headers", idx);
    }
    const int m = d[pos++];
    if (m == 0xD9) {
      if (started) break;
      JBAD("jpeg_plan_prog: file %d: EOI before SOS", idx);
    }
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;   // TEM, a stray RSTn: no segment
    if (pos + 2 > n) {
      if (started) break;
      JBAD("jpeg_plan_prog: file %d: cut inside its headers", idx);
    }
    const long long L = (d[pos] << 8) | d[pos + 1];
    if (L < 2) JBAD("jpeg_plan_prog: file %d: bad segment length", idx);
    if (pos + L > n) {
      if (started) break;
      JBAD("jpeg_plan_prog: file %d: cut inside its headers", idx);
    }
    const unsigned char *s = d + pos + 2;
    const long long sl = L - 2;
    if (m == 0xDB) {
      long long q = 0;
      while (q < sl) {
        const int pq = s[q] >> 4, tq = s[q] & 15;
        if (pq) JNOT("jpeg_plan_prog: file %d: 16-bit quantiser table", idx);
        if (tq > 3 || q + 65 > sl) JBAD("jpeg_plan_prog: file %d: bad DQT segment", idx);
        if (!started || !tb.hasq[tq]) {   // a component's table is the one that stood at the file's first scan
          for (int k = 0; k < 64; ++k) tb.q[tq][kNatural[k]] = s[q + 1 + k];
          tb.hasq[tq] = true;
        }
        q += 65;
      }
    } else if (m == 0xC4) {
      long long q = 0;
      while (q < sl) {
        if (q + 17 > sl) JBAD("jpeg_plan_prog: file %d: bad DHT segment", idx);
        const int tc = s[q] >> 4, th = s[q] & 15;
        int tot = 0;
        for (int k = 0; k < 16; ++k) tot += s[q + 1 + k];
        if (tc > 1 || th > 3 || tot > 256 || q + 17 + tot > sl) JBAD("jpeg_plan_prog: file %d: bad DHT segment", idx);
        if (!derive_table(s + q + 1, s + q + 17, tot, tb.h[tc][th]))
          JBAD("jpeg_plan_prog: file %d: invalid Huffman code lengths", idx);
        tb.hash[tc][th] = true;
        q += 17 + tot;
      }
    } else if (m == 0xC0 || m == 0xC2) {
      if (have_frame) JBAD("jpeg_plan_prog: file %d: a second SOF segment", idx);
      if (sl < 6) JBAD("jpeg_plan_prog: file %d: bad SOF segment", idx);
      if (s[0] != 8) JNOT("jpeg_plan_prog: file %d: %d-bit samples", idx, (int)s[0]);
      im.H = (s[1] << 8) | s[2];
      im.W = (s[3] << 8) | s[4];
      const int nf = s[5];
      if (nf != 1 && nf != 3) JNOT("jpeg_plan_prog: file %d: %d components (grey and YCbCr only)", idx, nf);
      if (sl < 6 + 3 * nf || im.H == 0 || im.W == 0) JBAD("jpeg_plan_prog: file %d: bad SOF segment", idx);
      if (im.H > kJpegMaxSide || im.W > kJpegMaxSide)
        JNOT("jpeg_plan_prog: file %d: %d x %d, supported up to %d x %d", idx, im.H, im.W, kJpegMaxSide, kJpegMaxSide);
      im.ncomp = nf;
      im.progressive = m == 0xC2;
      for (int i = 0; i < nf; ++i) {
        im.fid[i] = s[6 + 3 * i];
        const int h = s[7 + 3 * i] >> 4, v = s[7 + 3 * i] & 15;
        im.tq[i] = s[8 + 3 * i];
        if (i == 0) {
          im.hs = h;
          im.vs = v;
        } else if (h != 1 || v != 1) {
          JNOT("jpeg_plan_prog: file %d: chroma sampling %d x %d (1 x 1 only)", idx, h, v);
        }
      }
      if (nf == 3) {
        if (!((im.hs == 1 && im.vs == 1) || (im.hs == 2 && im.vs == 1) || (im.hs == 2 && im.vs == 2)))
          JNOT("jpeg_plan_prog: file %d: luma sampling %d x %d (1 x 1, 2 x 1, 2 x 2 only)", idx, im.hs, im.vs);
      } else {
        im.hs = im.vs = 1;   // a single component is never interleaved
      }
      im.mx = (im.W + 8 * im.hs - 1) / (8 * im.hs);
      im.my = (im.H + 8 * im.vs - 1) / (8 * im.vs);
      have_frame = true;
    } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8) {
      JNOT("jpeg_plan_prog: file %d: SOF%d (arithmetic, lossless, hierarchical or 12-bit coding); SOF0 and SOF2 only", idx,
           m - 0xC0);
    } else if (m == 0xDD) {
      if (sl < 2) JBAD("jpeg_plan_prog: file %d: bad DRI segment", idx);
      ri = (s[0] << 8) | s[1];
    } else if (m == 0xEE && sl >= 12 && !memcmp(s, "Adobe", 5)) {
      adobe = s[11];
    } else if (m == 0xDA) {
      const int sn = im.nscans;
      if (!have_frame) JBAD("jpeg_plan_prog: file %d: SOS before SOF", idx);
      if (sn >= kJpegMaxScans) JNOT("jpeg_plan_prog: file %d: more than %d scans", idx, kJpegMaxScans);
      const int ns = sl ? s[0] : 0;
      if (sl < 1 + 2 * ns + 3) JBAD("jpeg_plan_prog: file %d: scan %d: bad SOS segment", idx, sn);
      if (im.ncomp == 3 && adobe == 0) JNOT("jpeg_plan_prog: file %d: Adobe transform 0 (RGB / CMYK data)", idx);
      if (!im.progressive && ns != im.ncomp)
        JNOT("jpeg_plan_prog: file %d: multi-scan SOF0 file (%d of %d components in the first scan)", idx, ns, im.ncomp);
      if (ns < 1 || ns > im.ncomp) JBAD("jpeg_plan_prog: file %d: scan %d: %d components in a frame of %d", idx, sn, ns, im.ncomp);
      int comp[3] = {-1, -1, -1}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
      for (int i = 0; i < ns; ++i) {
        int c = -1;
        for (int j = 0; j < im.ncomp; ++j)
          if (s[1 + 2 * i] == im.fid[j]) c = j;
        if (c < 0) JBAD("jpeg_plan_prog: file %d: scan %d: component %d is not in the frame", idx, sn, (int)s[1 + 2 * i]);
        if ((i > 0 && c <= comp[i - 1]) || (!im.progressive && c != i))
          JNOT("jpeg_plan_prog: file %d: scan components out of frame order", idx);
        comp[i] = c;
        td[i] = s[2 + 2 * i] >> 4;
        ta[i] = s[2 + 2 * i] & 15;
      }
      int Ss = 0, Se = 63, Ah = 0, Al = 0, kind = XM_JPEG_SCAN_SEQ, level = 0;
      if (im.progressive) {
        Ss = s[1 + 2 * ns];
        Se = s[2 + 2 * ns];
        Ah = s[3 + 2 * ns] >> 4;
        Al = s[3 + 2 * ns] & 15;
        if (Ss > Se || Se > 63) JBAD("jpeg_plan_prog: file %d: scan %d: band %d .. %d (need Ss <= Se <= 63)", idx, sn, Ss, Se);
        if (Ss == 0 && Se != 0) JBAD("jpeg_plan_prog: file %d: scan %d: band 0 .. %d mixes DC and AC", idx, sn, Se);
        if (Ss > 0 && ns != 1) JBAD("jpeg_plan_prog: file %d: scan %d: an AC scan of %d components", idx, sn, ns);
        if (Al > 13) JBAD("jpeg_plan_prog: file %d: scan %d: Al %d (at most 13)", idx, sn, Al);
        if (Ah != 0 && Ah != Al + 1) JBAD("jpeg_plan_prog: file %d: scan %d: Ah %d is not Al + 1 = %d", idx, sn, Ah, Al + 1);
        for (int i = 0; i < ns; ++i)
          for (int k = Ss; k <= Se; ++k) {
            const int have = im.bits[comp[i]][k];
            if (Ah == 0 && have >= 0)
              JBAD("jpeg_plan_prog: file %d: scan %d: coefficient %d of component %d is sent twice", idx, sn, k, comp[i]);
            if (Ah != 0 && have < 0)
              JBAD("jpeg_plan_prog: file %d: scan %d: refines coefficient %d of component %d, which no earlier scan sent", idx,
                   sn, k, comp[i]);
            if (Ah != 0 && have != Ah)
              JBAD("jpeg_plan_prog: file %d: scan %d: Ah %d, the previous scan of coefficient %d had Al %d", idx, sn, Ah, k, have);
            if (im.level[comp[i]][k] + 1 > level) level = im.level[comp[i]][k] + 1;
          }
        for (int i = 0; i < ns; ++i)
          for (int k = Ss; k <= Se; ++k) {
            im.bits[comp[i]][k] = Al;
            im.level[comp[i]][k] = level;
          }
        kind = Ss == 0 ? (Ah == 0 ? XM_JPEG_SCAN_DC_FIRST : XM_JPEG_SCAN_DC_REFINE)
                       : (Ah == 0 ? XM_JPEG_SCAN_AC_FIRST : XM_JPEG_SCAN_AC_REFINE);
      }
      const bool need_dc = kind == XM_JPEG_SCAN_SEQ || kind == XM_JPEG_SCAN_DC_FIRST;
      const bool need_ac = kind == XM_JPEG_SCAN_SEQ || kind == XM_JPEG_SCAN_AC_FIRST || kind == XM_JPEG_SCAN_AC_REFINE;
      for (int i = 0; i < ns; ++i)
        if (td[i] > 3 || ta[i] > 3 || (need_dc && !tb.hash[0][td[i]]) || (need_ac && !tb.hash[1][ta[i]]))
          JBAD("jpeg_plan_prog: file %d: scan %d: component %d names a table the file does not define", idx, sn, comp[i]);
      if (sn == 0) {
        for (int i = 0; i < im.ncomp; ++i)
          if (im.tq[i] > 3 || !tb.hasq[im.tq[i]])
            JBAD("jpeg_plan_prog: file %d: component %d names a table the file does not define", idx, i);
        im.ri0 = ri;
      }
      long long row[kJpegScan];
      for (int k = 0; k < kJpegScan; ++k) row[k] = 0;
      if (!im.progressive) {   // the slots, and the order they are interned in, are those of xm_jpeg_plan
        for (int c = 0; c < 3; ++c) {
          const int sc = c < im.ncomp ? c : 0;
          im.qslot[c] = intern<kQtBytes>(qpool, (const unsigned char *)tb.q[im.tq[sc]]);
          im.dcslot[c] = intern<kHtBytes>(hpool, tb.h[0][td[sc]]);
          im.acslot[c] = intern<kHtBytes>(hpool, tb.h[1][ta[sc]]);
        }
        for (int i = 0; i < ns; ++i) {
          row[S_DC + i] = im.dcslot[i];
          row[S_AC + i] = im.acslot[i];
        }
      } else {
        if (sn == 0)
          for (int c = 0; c < 3; ++c)
            im.qslot[c] = intern<kQtBytes>(qpool, (const unsigned char *)tb.q[im.tq[c < im.ncomp ? c : 0]]);
        for (int i = 0; i < ns; ++i) {
          row[S_DC + i] = need_dc ? intern<kHtBytes>(hpool, tb.h[0][td[i]]) : 0;
          row[S_AC + i] = need_ac ? intern<kHtBytes>(hpool, tb.h[1][ta[i]]) : 0;
        }
      }
      pos += L;
      cuts.clear();
      const long long end = jpeg_scan_end(d, n, pos, cuts);
      // the raster: MCUs of an interleaved scan; the component's own blocks, without the MCU padding, otherwise
      long long bw = im.mx, bh = im.my;
      if (ns == 1 && im.ncomp == 3) {
        const int hc = comp[0] == 0 ? im.hs : 1, vc = comp[0] == 0 ? im.vs : 1;
        bw = ((im.W * hc + im.hs - 1) / im.hs + 7) / 8;
        bh = ((im.H * vc + im.vs - 1) / im.vs + 7) / 8;
      }
      row[S_IMG] = idx;
      row[S_NS] = ns;
      for (int i = 0; i < 3; ++i) row[S_COMP + i] = comp[i];
      row[S_SS] = Ss;
      row[S_SE] = Se;
      row[S_AH] = Ah;
      row[S_AL] = Al;
      row[S_B0] = base + pos;
      row[S_B1] = base + end;
      row[S_BW] = bw;
      row[S_BH] = bh;
      row[S_LEVEL] = level;
      row[S_LANE0] = (long long)(lane_rows.size() / kJpegLane);
      row[S_RI] = ri;
      row[S_KIND] = kind;
      // one lane per restart interval; markers past the last interval of the scan are ignored
      const long long srow = (long long)(scan_rows.size() / kJpegScan), total = bw * bh;
      long long begin = pos, k = 0;
      if (ri > 0) {
        for (size_t c = 0; c < cuts.size() && (k + 1) * ri < total; ++c, ++k) {
          const long long lr[4] = {srow, base + begin, base + cuts[c], k * ri};
          lane_rows.insert(lane_rows.end(), lr, lr + 4);
          begin = cuts[c] + 2;
        }
      }
      const long long lr[4] = {srow, base + begin, base + end, ri > 0 ? k * ri : 0};
      lane_rows.insert(lane_rows.end(), lr, lr + 4);
      row[S_NLANES] = (long long)(lane_rows.size() / kJpegLane) - row[S_LANE0];
      scan_rows.insert(scan_rows.end(), row, row + kJpegScan);
      if (sn == 0) im.data0 = pos;
      im.data1 = end;
      ++im.nscans;
      if (level + 1 > levels) levels = level + 1;
      if (!im.progressive) break;   // as xm_jpeg_plan: what follows the scan of a baseline file is not looked at
      pos = end;
      continue;
    }
    pos += L;
  }
  im.smooth = jpeg_scan_smoothing(im, tb);
  return XM_OK;
#undef JBAD
#undef JNOT
}

// sizes: XM_JPEG_PROG_SIZES int64 -- the eight of xm_jpeg_plan, then scans, levels and whether any file is smoothed
static inline int jpeg_plan_prog(const unsigned char *bytes, const long long *offsets, int N, long long *desc, long long *scans,
                                 long long scans_cap, long long *lanes, long long lanes_cap, unsigned char *tables,
                                 long long tables_cap, long long *sizes, char *err, int errlen) {
  if (N < 0 || scans_cap < 0 || lanes_cap < 0 || tables_cap < 0)
    return jpeg_scan_fail(err, errlen, XM_EINVAL,
                          "jpeg_plan_prog: need N >= 0, scans_cap >= 0, lanes_cap >= 0, tables_cap >= 0 (got N=%d scans_cap=%lld "
                          "lanes_cap=%lld tables_cap=%lld)", N, scans_cap, lanes_cap, tables_cap);
  if (!sizes) return jpeg_scan_fail(err, errlen, XM_EINVAL, "jpeg_plan_prog: NULL sizes");
  for (int k = 0; k < XM_JPEG_PROG_SIZES; ++k) sizes[k] = 0;
  if (N == 0) return XM_OK;
  if (!bytes || !offsets || !desc || !scans || !lanes || !tables)
    return jpeg_scan_fail(err, errlen, XM_EINVAL, "jpeg_plan_prog: NULL argument");
  std::vector<unsigned char> qpool, hpool;
  std::vector<long long> scan_rows, lane_rows, cuts;
  long long coef = 0, plane = 0, pix = 0;
  int levels = 0, rc = XM_OK;
  bool smooth = false;
  JpegScanTables *tb = new JpegScanTables;
  for (int i = 0; i < N && rc == XM_OK; ++i) {
    if (offsets[i] < 0 || offsets[i + 1] < offsets[i]) {
      rc = jpeg_scan_fail(err, errlen, XM_EINVAL, "jpeg_plan_prog: file %d: offsets must ascend from 0", i);
      break;
    }
    JpegScanFile im;
    *tb = JpegScanTables();
    const long long base = offsets[i], lane0 = (long long)(lane_rows.size() / kJpegLane);
    rc = jpeg_scan_parse(i, bytes + base, offsets[i + 1] - base, base, im, *tb, qpool, hpool, scan_rows, lane_rows, cuts, levels,
                         err, errlen);
    if (rc) break;
    long long *d = desc + (long long)i * kJpegDesc;
    d[D_SCAN0] = base + im.data0;
    d[D_SCAN1] = base + im.data1;
    d[D_H] = im.H;
    d[D_W] = im.W;
    d[D_NCOMP] = im.ncomp;
    d[D_HS] = im.hs;
    d[D_VS] = im.vs;
    d[D_RI] = im.ri0;
    d[D_MX] = im.mx;
    d[D_MY] = im.my;
    for (int c = 0; c < 3; ++c) {
      d[D_QT + c] = im.qslot[c];
      d[D_DC + c] = im.progressive ? 0 : im.dcslot[c];
      d[D_AC + c] = im.progressive ? 0 : im.acslot[c];
      if (im.smooth && c < im.ncomp) {   // marker, then a nibble per coefficient: the Al it stands at + 1, 0 = never sent
        long long w = XM_JPEG_SMOOTH;
        for (int z = 0; z < 10; ++z) w |= (long long)(im.bits[c][z] + 1) << (4 * z);
        d[D_DC + c] = w;
      }
    }
    smooth = smooth || im.smooth;
    const long long total = (long long)im.mx * im.my;
    const long long nblocks = total * im.hs * im.vs + (im.ncomp == 3 ? 2 * total : 0);
    d[D_COEF] = coef;
    d[D_PLANE] = plane;
    d[D_PIX] = pix;
    coef += nblocks * 64;
    plane += nblocks * 64;
    pix += 3LL * im.H * im.W;
    d[D_LANE0] = lane0;
    d[D_NLANES] = (long long)(lane_rows.size() / kJpegLane) - lane0;
    if (coef >= (1LL << 31) || pix >= (1LL << 31))
      rc = jpeg_scan_fail(err, errlen, XM_ETOOBIG,
                          "jpeg_plan_prog: the batch holds 2^31 or more coefficients or pixel values at file %d", i);
  }
  delete tb;
  if (rc) return rc;
  const long long nq = (long long)(qpool.size() / kQtBytes), nh = (long long)(hpool.size() / kHtBytes);
  const long long nl = (long long)(lane_rows.size() / kJpegLane), nsc = (long long)(scan_rows.size() / kJpegScan);
  sizes[0] = (long long)(qpool.size() + hpool.size());
  sizes[1] = nq;
  sizes[2] = nh;
  sizes[3] = coef;
  sizes[4] = plane;
  sizes[5] = pix;
  sizes[6] = nl;
  sizes[7] = N;
  sizes[8] = nsc;
  sizes[9] = levels;
  sizes[10] = smooth ? 1 : 0;
  if (nsc > scans_cap) return jpeg_scan_fail(err, errlen, XM_ENOMEM, "jpeg_plan_prog: %lld scans, room for %lld", nsc, scans_cap);
  if (nl > lanes_cap) return jpeg_scan_fail(err, errlen, XM_ENOMEM, "jpeg_plan_prog: %lld lanes, room for %lld", nl, lanes_cap);
  if (sizes[0] > tables_cap)
    return jpeg_scan_fail(err, errlen, XM_ENOMEM, "jpeg_plan_prog: %lld table bytes, room for %lld", sizes[0], tables_cap);
  memcpy(scans, scan_rows.data(), scan_rows.size() * sizeof(long long));
  memcpy(lanes, lane_rows.data(), lane_rows.size() * sizeof(long long));
  memcpy(tables, qpool.data(), qpool.size());
  memcpy(tables + qpool.size(), hpool.data(), hpool.size());
  return XM_OK;
}

}  // namespace xm

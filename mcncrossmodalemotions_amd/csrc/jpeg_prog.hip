// Progressive JPEG decode of a batch of face frames on gfx950: vl.imreadjpeg(progressive=True).  The plan
// (xm_jpeg_plan_prog, jpeg_scan_plan.h) turns every file into scans -- a baseline file into one -- and every scan into
// lanes, one per restart interval, and gives each scan a level: 0 if no earlier scan of its image sends a coefficient
// it sends, else one more than the highest level among those that do.  Scans of one level write disjoint coefficients;
// a refinement scan reads what the level before it wrote, so a level is a launch:
//   jpeg_clear_kernel          as xm_jpeg_decode_batch
//   jpeg_entropy_prog_kernel   once per level, over all lanes: a lane of another level leaves at once.  kJpegLanes lanes
//                              per 64-thread block as in jpeg_entropy_kernel, the tables its scan uses (at most three DC
//                              and three AC) copied into LDS by the block, the same clamped byte reader.  Five kinds of
//                              scan: the sequential one of a baseline file (decode_block, shared with
//                              jpeg_entropy_kernel), DC first, DC refinement, AC first, AC refinement (T.81 G.1.2).
//                              The DC predictors and the end-of-band run start from zero in every lane.  Coefficients
//                              are int16 and are read and written as int16 alone: lanes of one level may own
//                              neighbouring coefficients of one block.
//   jpeg_idct_kernel, jpeg_colour_kernel, crop_resize_face_ragged_kernel   as xm_jpeg_decode_batch, unchanged: the
//                              entropy stages only ever write raw coefficients, dequantisation is the IDCT's
//   jpeg_smooth_kernel, jpeg_smooth_dc_kernel   only when the plan says that a file of the batch ends before its first
//                              coefficients have arrived in full: libjpeg's block smoothing (described at the kernels)
// The number of launches is 4 + levels (+ 2 with smoothing, + 1 with faces), whatever N and the sizes are.  A block's
// position comes from the lane's MCU counter and the scan's raster and is checked against the image's block count; a
// coefficient index is at most 63; a byte position is clamped to the lane's range, itself clamped to the scan's and
// the buffer.
#include "jpeg_entropy.h"
#include "prof.h"
#include "xm_common.h"

namespace xm {

struct ProgScan {   // lane-uniform: what the scan asks for
  int kind, Ss, Se, Al;
};

// one block of a progressive scan: 0 = fine, else XM_JPEG_BADCODE.  `out` holds the block's 64 coefficients in
// row-major order: zero before the first scan that sends them, what the earlier levels wrote afterwards.
__device__ __forceinline__ int prog_block(const ProgScan &g, BitReader &br, const unsigned char *dc, const unsigned char *ac,
                                          const unsigned char *nat, int &pred, int &eobrun, short *__restrict__ out) {
  if (g.kind == XM_JPEG_SCAN_DC_FIRST) {
    const int s = huff_decode(dc, br);
    if (s < 0 || s > 15) return XM_JPEG_BADCODE;
    pred += huff_extend(br.take(s), s);
    out[0] = (short)(pred * (1 << g.Al));
    return 0;
  }
  if (g.kind == XM_JPEG_SCAN_DC_REFINE) {
    if (br.take(1)) out[0] = (short)(out[0] | (1 << g.Al));
    return 0;
  }
  if (g.kind == XM_JPEG_SCAN_AC_FIRST) {
    if (eobrun > 0) {
      --eobrun;
      return 0;
    }
    for (int k = g.Ss; k <= g.Se; ++k) {
      const int rs = huff_decode(ac, br);
      if (rs < 0) return XM_JPEG_BADCODE;
      const int r = rs >> 4, s = rs & 15;
      if (s) {
        k += r;
        if (k > g.Se) return XM_JPEG_BADCODE;
        out[nat[k & 63]] = (short)(huff_extend(br.take(s), s) * (1 << g.Al));
      } else if (r == 15) {
        k += 15;
      } else {
        eobrun = (1 << r) + br.take(r) - 1;   // this block and eobrun more end here
        break;
      }
    }
    return 0;
  }
  // AC refinement (G.1.2.3): a new coefficient is +/- (1 << Al); every coefficient with history that the run passes
  // takes one correction bit, and so do those of the rest of the band under an end-of-band run
  const int p1 = 1 << g.Al, m1 = -p1;
  int k = g.Ss;
  if (eobrun == 0) {
    for (; k <= g.Se; ++k) {
      const int rs = huff_decode(ac, br);
      if (rs < 0) return XM_JPEG_BADCODE;
      int r = rs >> 4;
      const int s = rs & 15;
      int val = 0;
      if (s) {
        if (s != 1) return XM_JPEG_BADCODE;
        val = br.take(1) ? p1 : m1;
      } else if (r != 15) {
        eobrun = (1 << r) + br.take(r);
        break;
      }
      do {
        short *c = out + nat[k & 63];
        const int cur = *c;
        if (cur != 0) {
          if (br.take(1) && (cur & p1) == 0) *c = (short)(cur >= 0 ? cur + p1 : cur + m1);
        } else if (--r < 0) {
          break;
        }
        ++k;
      } while (k <= g.Se);
      if (s) {
        if (k > g.Se) return XM_JPEG_BADCODE;
        out[nat[k & 63]] = (short)val;
      }
    }
  }
  if (eobrun > 0) {
    for (; k <= g.Se; ++k) {
      short *c = out + nat[k & 63];
      const int cur = *c;
      if (cur != 0 && br.take(1) && (cur & p1) == 0) *c = (short)(cur >= 0 ? cur + p1 : cur + m1);
    }
    --eobrun;
  }
  return 0;
}

__global__ void __launch_bounds__(64)
jpeg_entropy_prog_kernel(const uint4 *__restrict__ bytes, long long nbytes, const long long *__restrict__ desc, int N,
                         const long long *__restrict__ scans, int nscans, const long long *__restrict__ lanes, int nlanes,
                         const unsigned char *__restrict__ huff, int nh, short *__restrict__ coef, int *__restrict__ status,
                         int level) {
  __shared__ __attribute__((aligned(16))) unsigned char s_tab[kJpegLanes][6][kHtBytes];
  __shared__ unsigned char s_nat[64];
  const int tid = threadIdx.x;
  s_nat[tid] = kNaturalDev[tid];
  // every lane of this level: the DC and AC tables of its scan's components, where the kind of scan reads them
  for (int j = tid; j < kJpegLanes * 6 * (kHtBytes / 16); j += 64) {
    const int l = j / (6 * (kHtBytes / 16)), rem = j - l * (6 * (kHtBytes / 16));
    const int tb = rem / (kHtBytes / 16), q = rem - tb * (kHtBytes / 16);
    const long long gl = (long long)blockIdx.x * kJpegLanes + l;
    if (gl >= nlanes) continue;
    const long long *sc = scans + min(max(lanes[gl * kJpegLane], 0LL), (long long)nscans - 1) * kJpegScan;
    if (sc[S_LEVEL] != level) continue;
    const int kind = (int)sc[S_KIND], i = tb < 3 ? tb : tb - 3;
    const bool wanted = tb < 3 ? (kind == XM_JPEG_SCAN_SEQ || kind == XM_JPEG_SCAN_DC_FIRST)
                               : (kind == XM_JPEG_SCAN_SEQ || kind == XM_JPEG_SCAN_AC_FIRST || kind == XM_JPEG_SCAN_AC_REFINE);
    if (!wanted || i >= sc[S_NS]) continue;
    const long long sl = min(max(sc[(tb < 3 ? S_DC : S_AC) + i], 0LL), (long long)nh - 1);
    ((uint4 *)&s_tab[l][tb][0])[q] = ((const uint4 *)(huff + sl * kHtBytes))[q];
  }
  __syncthreads();
  const long long gl = (long long)blockIdx.x * kJpegLanes + tid;
  if (tid >= kJpegLanes || gl >= nlanes) return;
  const long long *sc = scans + min(max(lanes[gl * kJpegLane], 0LL), (long long)nscans - 1) * kJpegScan;
  if (sc[S_LEVEL] != level) return;
  const long long img = min(max(sc[S_IMG], 0LL), (long long)N - 1);
  const long long *d = desc + img * kJpegDesc;
  // the lane's byte range, inside the scan's, inside the buffer
  const long long i0 = min(max(sc[S_B0], 0LL), nbytes), i1 = min(max(sc[S_B1], i0), nbytes);
  BitReader br;
  br.base = bytes;
  br.pos = min(max(lanes[gl * kJpegLane + 1], i0), i1);
  br.end = min(max(lanes[gl * kJpegLane + 2], br.pos), i1);
  br.cidx = -1;
  br.chunk = make_uint4(0, 0, 0, 0);
  br.acc = 0;
  br.nbits = 0;
  br.fake = 0;
  ProgScan g;
  g.kind = (int)sc[S_KIND];
  g.Ss = (int)min(max(sc[S_SS], 0LL), 63LL);
  g.Se = (int)min(max(sc[S_SE], (long long)g.Ss), 63LL);
  g.Al = (int)min(max(sc[S_AL], 0LL), 13LL);
  const int ns = (int)min(max(sc[S_NS], 1LL), 3LL);
  const int c0 = (int)min(max(sc[S_COMP], 0LL), 2LL), c1 = (int)min(max(sc[S_COMP + 1], 0LL), 2LL),
            c2 = (int)min(max(sc[S_COMP + 2], 0LL), 2LL);
  const int ncomp = (int)d[D_NCOMP], hs = min(max((int)d[D_HS], 1), 2), vs = min(max((int)d[D_VS], 1), 2);
  const int mx = max((int)d[D_MX], 1), my = max((int)d[D_MY], 0);
  // the scan's raster: MCUs of an interleaved scan, the component's own blocks otherwise (each one an MCU)
  const int bw = (int)min(max(sc[S_BW], 1LL), (long long)mx * hs), bh = (int)min(max(sc[S_BH], 0LL), (long long)my * vs);
  const long long ri = sc[S_RI], total = (long long)bw * bh, tot = (long long)mx * my;
  const long long mcu0 = min(max(lanes[gl * kJpegLane + 3], 0LL), total);
  const long long stop = ri > 0 ? min(mcu0 + ri, total) : total;
  const long long nbY = tot * hs * vs, nblocks = nbY + (ncomp == 3 ? 2 * tot : 0);
  short *cbase = coef + d[D_COEF];
  int p0 = 0, p1 = 0, p2 = 0, eobrun = 0, st = 0;
  for (long long mcu = mcu0; mcu < stop && !st; ++mcu) {
    const int ym = (int)(mcu / bw), xm = (int)(mcu - (long long)ym * bw);
    for (int i = 0; i < ns && !st; ++i) {
      const int c = i == 0 ? c0 : (i == 1 ? c1 : c2);
      const int hc = (ns > 1 && c == 0) ? hs : 1, vc = (ns > 1 && c == 0) ? vs : 1;
      int pred = i == 0 ? p0 : (i == 1 ? p1 : p2);
      for (int blk = 0; blk < hc * vc && !st; ++blk) {
        const int by = ym * vc + blk / hc, bx = xm * hc + blk % hc;
        const long long b = c == 0 ? (long long)by * (mx * hs) + bx : nbY + (c - 1) * tot + (long long)by * mx + bx;
        if (b < 0 || b >= nblocks) {   // not with a plan of xm_jpeg_plan_prog
          st = XM_JPEG_BADCODE;
        } else if (g.kind == XM_JPEG_SCAN_SEQ) {
          st = decode_block(br, s_tab[tid][i], s_tab[tid][3 + i], s_nat, pred, cbase + b * 64);
        } else {
          st = prog_block(g, br, s_tab[tid][i], s_tab[tid][3 + i], s_nat, pred, eobrun, cbase + b * 64);
        }
      }
      p0 = i == 0 ? pred : p0;
      p1 = i == 1 ? pred : p1;
      p2 = i == 2 ? pred : p2;
    }
    if (br.starved()) st |= XM_JPEG_TRUNCATED;
  }
  if (!st && eobrun > 0) st = XM_JPEG_BADCODE;   // an end-of-band run that leaves the restart interval
  if (st) atomicOr(status + img, st);
}

// ---- block smoothing -----------------------------------------------------------------------------------------------
// What libjpeg does, and with it vl_imreadjpeg, to a progressive file that ends before the first ten coefficients (in
// zigzag order) of every component have arrived in full (jdcoefct.c decompress_smooth_data, the 5 x 5 form of
// libjpeg-turbo 2.1 and later): such a coefficient, while it is still zero, is estimated from the DC values of the
// 5 x 5 blocks around its block -- edges replicated inside the component's own raster -- and kept below 1 << Al; while
// no AC bit of the component has arrived at all the DC itself is smoothed too and four more coefficients are estimated.
// The plan marks such an image in its descriptor (XM_JPEG_SMOOTH and a nibble per coefficient in columns 13-15).
// jpeg_smooth_kernel: one thread per block; it reads DC values and its own block, writes its own AC coefficients in place
// and the new DC into the first bytes of the block's (still unused) plane bytes; jpeg_smooth_dc_kernel moves that DC in.
struct SmoothSite {
  bool on, change_dc;
  int c, by, bx, bw, bh, cb[10];
  long long first, pitch;   // block index of the component's (0, 0) inside the batch and its padded pitch
  const unsigned short *q;
};

__device__ __forceinline__ SmoothSite smooth_site(const long long *__restrict__ desc, int N, const unsigned char *__restrict__ qtabs,
                                                  int nq, long long nblocks_all, long long g) {
  SmoothSite s;
  s.on = false;
  if (g >= nblocks_all) return s;
  const int img = find_image(desc, N, D_COEF, 64, g);
  const long long *d = desc + (long long)img * kJpegDesc;
  const int hs = min(max((int)d[D_HS], 1), 2), vs = min(max((int)d[D_VS], 1), 2), mx = max((int)d[D_MX], 1), my = max((int)d[D_MY], 0);
  const int ncomp = (int)d[D_NCOMP], H = (int)d[D_H], W = (int)d[D_W];
  const long long total = (long long)mx * my, nbY = total * hs * vs;
  const long long b = g - d[D_COEF] / 64;
  if (b < 0 || b >= nbY + (ncomp == 3 ? 2 * total : 0)) return s;
  s.c = b < nbY ? 0 : (b < nbY + total ? 1 : 2);
  const long long w = d[D_DC + s.c];
  if ((w >> 40) != 1) return s;   // XM_JPEG_SMOOTH: not a table slot
  const long long lb = s.c == 0 ? b : b - nbY - (s.c - 1) * total;
  s.pitch = s.c == 0 ? (long long)mx * hs : mx;
  s.by = (int)(lb / s.pitch);
  s.bx = (int)(lb - s.by * s.pitch);
  const int cw = s.c == 0 || ncomp == 1 ? W : (W + hs - 1) / hs, ch = s.c == 0 || ncomp == 1 ? H : (H + vs - 1) / vs;
  s.bw = min((cw + 7) / 8, (int)s.pitch);
  s.bh = min((ch + 7) / 8, s.c == 0 ? my * vs : my);
  if (s.bx >= s.bw || s.by >= s.bh) return s;   // MCU padding: no pixel of the image comes from it
  s.first = d[D_COEF] / 64 + (s.c == 0 ? 0 : nbY + (s.c - 1) * total);
  s.change_dc = true;
#pragma unroll
  for (int z = 0; z < 10; ++z) {
    s.cb[z] = (int)((w >> (4 * z)) & 15) - 1;
    if (z > 0 && s.cb[z] != -1) s.change_dc = false;
  }
  s.q = (const unsigned short *)(qtabs + min(max(d[D_QT + s.c], 0LL), (long long)nq - 1) * kQtBytes);
  s.on = true;
  return s;
}

// jdcoefct.c: the estimate num / (256 Q), rounded away from zero at the half, below 1 << Al when Al > 0
__device__ __forceinline__ int smooth_pred(long long num, int Q, int Al) {
  const long long a = num >= 0 ? num : -num;
  int pred = (int)((((long long)Q << 7) + a) / ((long long)Q << 8));
  if (Al > 0 && pred >= (1 << Al)) pred = (1 << Al) - 1;
  return num >= 0 ? pred : -pred;
}

__global__ void __launch_bounds__(256)
jpeg_smooth_kernel(short *__restrict__ coef, long long nblocks_all, const long long *__restrict__ desc, int N,
                   const unsigned char *__restrict__ qtabs, int nq, unsigned char *__restrict__ planes) {
  const long long g = blockIdx.x * (long long)256 + threadIdx.x;
  const SmoothSite s = smooth_site(desc, N, qtabs, nq, nblocks_all, g);
  if (!s.on) return;
  // DC(r, c): the DC of the block r rows and c columns away, the raster's edge replicated
  int D[5][5];
#pragma unroll
  for (int r = 0; r < 5; ++r)
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      const int y = min(max(s.by + r - 2, 0), s.bh - 1), x = min(max(s.bx + c - 2, 0), s.bw - 1);
      D[r][c] = coef[(s.first + (long long)y * s.pitch + x) * 64];
    }
  const bool cd = s.change_dc;
  long long num[10];
  // DC01 .. DC25 of jdcoefct.c are D[0][0] .. D[4][4], row by row
  num[1] = cd ? -D[0][0] - D[0][1] + D[0][3] + D[0][4] - 3 * D[1][0] + 13 * D[1][1] - 13 * D[1][3] + 3 * D[1][4] - 3 * D[2][0] +
                    38 * D[2][1] - 38 * D[2][3] + 3 * D[2][4] - 3 * D[3][0] + 13 * D[3][1] - 13 * D[3][3] + 3 * D[3][4] - D[4][0] -
                    D[4][1] + D[4][3] + D[4][4]
              : -7 * D[2][0] + 50 * D[2][1] - 50 * D[2][3] + 7 * D[2][4];
  num[2] = cd ? -D[0][0] - D[1][0] + D[3][0] + D[4][0] - 3 * D[0][1] + 13 * D[1][1] - 13 * D[3][1] + 3 * D[4][1] - 3 * D[0][2] +
                    38 * D[1][2] - 38 * D[3][2] + 3 * D[4][2] - 3 * D[0][3] + 13 * D[1][3] - 13 * D[3][3] + 3 * D[4][3] - D[0][4] -
                    D[1][4] + D[3][4] + D[4][4]
              : -7 * D[0][2] + 50 * D[1][2] - 50 * D[3][2] + 7 * D[4][2];
  num[3] = cd ? D[0][2] + 2 * D[1][1] + 7 * D[1][2] + 2 * D[1][3] - 5 * D[2][1] - 14 * D[2][2] - 5 * D[2][3] + 2 * D[3][1] +
                    7 * D[3][2] + 2 * D[3][3] + D[4][2]
              : -D[0][2] + 13 * D[1][2] - 24 * D[2][2] + 13 * D[3][2] - D[4][2];
  num[4] = cd ? -D[0][0] + D[0][4] + 9 * D[1][1] - 9 * D[1][3] - 9 * D[3][1] + 9 * D[3][3] + D[4][0] - D[4][4]
              : -D[0][1] + D[0][3] - D[1][0] + 10 * D[1][1] - 10 * D[1][3] + D[1][4] + D[3][0] - 10 * D[3][1] + 10 * D[3][3] -
                    D[3][4] + D[4][1] - D[4][3];
  num[5] = cd ? D[2][0] + 2 * D[1][1] + 7 * D[2][1] + 2 * D[3][1] - 5 * D[1][2] - 14 * D[2][2] - 5 * D[3][2] + 2 * D[1][3] +
                    7 * D[2][3] + 2 * D[3][3] + D[2][4]
              : -D[2][0] + 13 * D[2][1] - 24 * D[2][2] + 13 * D[2][3] - D[2][4];
  num[6] = D[1][1] - D[1][3] + 2 * D[2][1] - 2 * D[2][3] + D[3][1] - D[3][3];
  num[7] = D[1][1] - 3 * D[1][2] + D[1][3] - D[3][1] + 3 * D[3][2] - D[3][3];
  num[8] = D[1][1] - 3 * D[2][1] + D[3][1] - D[1][3] + 3 * D[2][3] - D[3][3];
  num[9] = D[1][1] - D[3][1] + 2 * D[1][2] - 2 * D[3][2] + D[1][3] - D[3][3];
  num[0] = -2 * (D[0][0] + D[0][4] + D[4][0] + D[4][4]) -
           6 * (D[0][1] + D[0][3] + D[1][0] + D[1][4] + D[3][0] + D[3][4] + D[4][1] + D[4][3]) -
           8 * (D[0][2] + D[2][0] + D[2][4] + D[4][2]) + 6 * (D[1][1] + D[1][3] + D[3][1] + D[3][3]) +
           42 * (D[1][2] + D[2][1] + D[2][3] + D[3][2]) + 152 * D[2][2];
  const int pos[10] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24};
  const int Q00 = s.q[0];
  short *blk = coef + g * 64;
#pragma unroll
  for (int z = 1; z < 10; ++z) {
    const int Q = s.q[pos[z]];
    if ((z < 6 || cd) && s.cb[z] != 0 && Q != 0 && blk[pos[z]] == 0) blk[pos[z]] = (short)smooth_pred(num[z] * Q00, Q, s.cb[z]);
  }
  if (cd && Q00 != 0) *(short *)(planes + g * 64) = (short)smooth_pred(num[0] * Q00, Q00, 0);
}

__global__ void __launch_bounds__(256)
jpeg_smooth_dc_kernel(short *__restrict__ coef, long long nblocks_all, const long long *__restrict__ desc, int N,
                      const unsigned char *__restrict__ qtabs, int nq, const unsigned char *__restrict__ planes) {
  const long long g = blockIdx.x * (long long)256 + threadIdx.x;
  const SmoothSite s = smooth_site(desc, N, qtabs, nq, nblocks_all, g);
  if (s.on && s.change_dc && s.q[0] != 0) coef[g * 64] = *(const short *)(planes + g * 64);
}

namespace {

struct ProgStage : JpegEntropyStage {
  const unsigned char *bytes;
  long long nbytes;
  const long long *desc, *scans, *lanes;
  const unsigned char *tables;
  long long coef_elems;
  int N, nscans, nlanes, nq, nh, *status, levels, smooth;
  int min_huff() const override { return 1; }   // a file that ends after its DC scan
  int launch(short *coef, const unsigned char *huff, unsigned char *planes, hipStream_t st) const override {
    for (int level = 0; level < levels; ++level) {
      {
        ProfScope ps(prof_key(kProfJpegProg, 0), 0, st);
        hipLaunchKernelGGL(jpeg_entropy_prog_kernel, dim3((unsigned)((nlanes + kJpegLanes - 1) / kJpegLanes)), dim3(64), 0, st,
                           (const uint4 *)bytes, nbytes, desc, N, scans, nscans, lanes, nlanes, huff, nh, coef, status, level);
      }
      XM_LAUNCH_CHECK();
    }
    if (!smooth) return XM_OK;
    const long long nb = coef_elems / 64;
    {
      ProfScope ps(prof_key(kProfJpegProg, 1), 0, st);
      hipLaunchKernelGGL(jpeg_smooth_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, coef, nb, desc, N, tables, nq,
                         planes);
    }
    XM_LAUNCH_CHECK();
    {
      ProfScope ps(prof_key(kProfJpegProg, 2), 0, st);
      hipLaunchKernelGGL(jpeg_smooth_dc_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, coef, nb, desc, N, tables, nq,
                         (const unsigned char *)planes);
    }
    XM_LAUNCH_CHECK();
    return XM_OK;
  }
};

}  // namespace

}  // namespace xm

using namespace xm;

extern "C" {

int xm_jpeg_plan_prog(const unsigned char *bytes, const long long *offsets, int N, long long *desc, long long *scans,
                      long long scans_cap, long long *lanes, long long lanes_cap, unsigned char *tables, long long tables_cap,
                      long long *sizes) {
  char msg[256];
  msg[0] = 0;
  const int rc = jpeg_plan_prog(bytes, offsets, N, desc, scans, scans_cap, lanes, lanes_cap, tables, tables_cap, sizes, msg,
                                (int)sizeof msg);
  return rc ? fail(rc, "%s", msg) : XM_OK;
}

int xm_jpeg_decode_batch_prog(const unsigned char *bytes, long long nbytes, const long long *desc, int N,
                              const long long *lanes, int nlanes, const unsigned char *tables, int nq, int nh,
                              long long coef_elems, long long plane_bytes, long long pixel_floats, float *pixels, float *faces,
                              float crop, int Ho, int Wo, const float *avg3, int *status, const long long *scans, int nscans,
                              int levels, int smooth, void *stream) {
  if (N > 0 && (!scans || ((uintptr_t)scans & 7)))
    return fail(XM_EINVAL, "jpeg_decode_batch_prog: scans must be an 8-byte aligned device pointer");
  if (N > 0 && (nscans < N || nlanes < nscans || levels < 1 || levels > XM_JPEG_MAX_LEVELS))
    return fail(XM_EINVAL, "jpeg_decode_batch_prog: need N <= nscans <= nlanes and 1 <= levels <= %d (got %d, %d, %d)",
                XM_JPEG_MAX_LEVELS, nscans, nlanes, levels);
  ProgStage stage;
  stage.bytes = bytes;
  stage.nbytes = nbytes;
  stage.desc = desc;
  stage.scans = scans;
  stage.lanes = lanes;
  stage.N = N;
  stage.nscans = nscans;
  stage.nlanes = nlanes;
  stage.nh = nh;
  stage.status = status;
  stage.levels = levels;
  stage.smooth = smooth;
  stage.tables = tables;
  stage.nq = nq;
  stage.coef_elems = coef_elems;
  return jpeg_decode_launch(bytes, nbytes, desc, N, lanes, nlanes, tables, nq, nh, coef_elems, plane_bytes, pixel_floats,
                            pixels, faces, crop, Ho, Wo, avg3, status, stage, stream);
}

}  // extern "C"

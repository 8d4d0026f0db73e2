// Baseline JPEG decode of a batch of face frames on gfx950: what vl_imreadjpeg does in front of the frozen teacher
// (emoVoxCeleb/fetch_emovoxceleb_imdb.m:160-172, external/compute_visual_feats.m:130-143), with libjpeg's default
// integer arithmetic (ISLOW IDCT, fancy chroma upsampling, 16-bit fixed-point YCbCr -> RGB), so results are compared
// for equality.  include/xmodal.h documents the descriptor, lane and table layouts.
//
// xm_jpeg_plan (host, no device call) parses the headers, splits the entropy data at the RSTn markers into lanes, builds
// the quantiser and Huffman lookup tables (shared between images with equal tables) and lays the ragged buffers out.
// xm_jpeg_decode_batch enqueues a fixed number of launches, whatever N and the sizes are:
//   jpeg_clear_kernel    zeroes the coefficients (the entropy kernel writes only the non-zero ones) and the status
//   jpeg_entropy_kernel  one lane per restart interval (per image without DRI), kJpegLanes lanes per 64-thread block:
//                        lanes diverge by design, so a wave carries few of them and the grid has many waves.  The
//                        block's threads copy each lane's six Huffman tables into LDS; a lane reads its bytes in
//                        16-byte pieces held in registers, unstuffs FF 00 and feeds a 64-bit accumulator.  A byte
//                        position outside the lane's range -- itself clamped to the image's range and the buffer --
//                        yields zero bits; using one sets TRUNCATED.  A block index comes from the MCU counter and is
//                        below the image's block count, a coefficient index is at most 63; an invalid code or a run past
//                        63 sets BADCODE and ends the lane.
//   jpeg_idct_kernel     one thread per 8 x 8 block: dequantise, jpeg_idct_islow in int32 (13-bit constants,
//                        PASS1_BITS 2), range limit, eight 8-byte stores into the component's uint8 plane
//   jpeg_colour_kernel   one thread per pixel: triangle upsampling of the chroma (h2v1 / h2v2, edges replicated, planes
//                        of one or two columns replicated as libjpeg does), YCbCr -> RGB, cropped to H x W, written as
//                        H x W x 3 single in MATLAB layout
//   crop_resize_face_ragged_kernel (misc.hip, next to the kernel it must equal bit for bit)   the teacher's input
// xm_jpeg_decode_batch_split enqueues the same launches with jpeg_entropy_split_kernel as the entropy stage: one block
// per lane, one thread per segment of seg_bytes raw bytes, for files without restart markers (described at the kernel).
// The byte reader, the Huffman lookup and the block decode live in jpeg_entropy.h and the layout constants and table
// helpers in jpeg_scan_plan.h, shared with the progressive decode (csrc/jpeg_prog.hip), which also runs its entropy
// stage between the launches of jpeg_decode_launch below.
#include <algorithm>
#include <vector>

#include "jpeg_entropy.h"
#include "prof.h"
#include "xm_common.h"

namespace xm {

// ---- jpeg_clear_kernel ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) jpeg_clear_kernel(uint4 *__restrict__ coef, size_t n16, int *__restrict__ status, int N) {
  const size_t tid = blockIdx.x * (size_t)256 + threadIdx.x, step = (size_t)gridDim.x * 256;
  for (size_t i = tid; i < n16; i += step) coef[i] = make_uint4(0, 0, 0, 0);
  for (size_t i = tid; i < (size_t)N; i += step) status[i] = XM_JPEG_OK;
}

// ---- jpeg_entropy_kernel -------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
jpeg_entropy_kernel(const uint4 *__restrict__ bytes, long long nbytes, const long long *__restrict__ desc, int N,
                    const long long *__restrict__ lanes, int nlanes, const unsigned char *__restrict__ huff,
                    int nh, short *__restrict__ coef, int *__restrict__ status) {
  __shared__ __attribute__((aligned(16))) unsigned char s_tab[kJpegLanes][6][kHtBytes];
  __shared__ unsigned char s_nat[64];
  const int tid = threadIdx.x;
  s_nat[tid] = kNaturalDev[tid];
  // every lane's tables: DC and AC of its three components (a grey image repeats component 0)
  for (int j = tid; j < kJpegLanes * 6 * (kHtBytes / 16); j += 64) {
    const int l = j / (6 * (kHtBytes / 16)), rem = j - l * (6 * (kHtBytes / 16));
    const int tb = rem / (kHtBytes / 16), q = rem - tb * (kHtBytes / 16);
    const long long gl = min((long long)blockIdx.x * kJpegLanes + l, (long long)nlanes - 1);
    const long long img = min(max(lanes[gl * kJpegLane], 0LL), (long long)N - 1);
    const long long slot = desc[img * kJpegDesc + (tb < 3 ? D_DC + tb : D_AC + tb - 3)];
    const long long sl = min(max(slot, 0LL), (long long)nh - 1);
    ((uint4 *)&s_tab[l][tb][0])[q] = ((const uint4 *)(huff + sl * kHtBytes))[q];
  }
  __syncthreads();
  const long long gl = (long long)blockIdx.x * kJpegLanes + tid;
  if (tid >= kJpegLanes || gl >= nlanes) return;
  const long long img = min(max(lanes[gl * kJpegLane], 0LL), (long long)N - 1);
  const long long *d = desc + img * kJpegDesc;
  // the lane's byte range, inside the image's, inside the buffer
  const long long i0 = min(max(d[D_SCAN0], 0LL), nbytes), i1 = min(max(d[D_SCAN1], i0), nbytes);
  BitReader br;
  br.base = bytes;
  br.pos = min(max(lanes[gl * kJpegLane + 1], i0), i1);
  br.end = min(max(lanes[gl * kJpegLane + 2], br.pos), i1);
  br.cidx = -1;
  br.chunk = make_uint4(0, 0, 0, 0);
  br.acc = 0;
  br.nbits = 0;
  br.fake = 0;
  const int ncomp = (int)d[D_NCOMP], hs = (int)d[D_HS], vs = (int)d[D_VS], mx = (int)d[D_MX], my = (int)d[D_MY];
  const long long ri = d[D_RI], total = (long long)mx * my;
  const long long mcu0 = min(max(lanes[gl * kJpegLane + 3], 0LL), total);
  const long long stop = ri > 0 ? min(mcu0 + ri, total) : total;
  const long long nbY = total * hs * vs, nblocks = nbY + (ncomp == 3 ? 2 * total : 0);
  short *cbase = coef + d[D_COEF];
  int pred0 = 0, pred1 = 0, pred2 = 0, st = 0;
  for (long long mcu = mcu0; mcu < stop && !st; ++mcu) {
    const int ym = (int)(mcu / mx), xm = (int)(mcu - (long long)ym * mx);
    for (int blk = 0; blk < hs * vs && !st; ++blk) {
      const int by = ym * vs + blk / hs, bx = xm * hs + blk % hs;
      const long long b = (long long)by * (mx * hs) + bx;
      if (b < nblocks) st = decode_block(br, s_tab[tid][0], s_tab[tid][3], s_nat, pred0, cbase + b * 64);
    }
    if (ncomp == 3 && !st) {
      const long long b = nbY + mcu;
      if (b < nblocks) st = decode_block(br, s_tab[tid][1], s_tab[tid][4], s_nat, pred1, cbase + b * 64);
      if (!st && b + total < nblocks)
        st = decode_block(br, s_tab[tid][2], s_tab[tid][5], s_nat, pred2, cbase + (b + total) * 64);
    }
    if (br.starved()) st |= XM_JPEG_TRUNCATED;
  }
  if (st) atomicOr(status + img, st);
}

// ---- jpeg_entropy_split_kernel -------------------------------------------------------------------------------------
// The entropy stage of xm_jpeg_decode_batch_split: one block per lane, one thread per segment of seg_bytes raw bytes, a
// lane of more than kJpegSplitThreads segments in consecutive passes.  A decoder state is (bit position, block inside
// the MCU, coefficient index k; k == 0: a DC symbol comes next) or "ended".  A bit position is canonical: 8 x the raw
// offset of a byte the reader delivers (never the 00 of an FF 00 pair) + 0 .. 7, so two threads at the same bit compare
// equal whatever they hold in their accumulators; past the end of the entropy data it goes on counting the zero bits
// consumed.  A thread decodes symbols until one starts at or past its segment's end and publishes the state there.
// Once the front of its reader stands at or past the end of the data (the lane's last byte or a marker inside it) a
// thread is in the tail: it publishes "ended", and in the writing pass it is the thread that goes on, over zero bits,
// to the end of the MCU, as jpeg_entropy_kernel does before it sets TRUNCATED.
//   rounds   round 0: thread 0 decodes from the pass's confirmed entry, every other thread from the first byte of its
//            segment with (block 0, k 0) -- there an invalid code or a run past 63 drops one bit and resets k, the
//            thread is guessing.  Then every thread whose predecessor's exit differs from its own entry takes it and
//            decodes again (an invalid code now ends the chain), and so does a thread whose guessed entry turned out
//            right but whose decode had skipped an invalid symbol, until no thread did: thread i is final after round i,
//            so the loop is bounded by the pass's segments and its condition is block-uniform (__syncthreads_or).
//            Each decode also counts the blocks completed and sums the DC differences per component.
//   scan     exclusive over (blocks, dc0, dc1, dc2, ended): a thread's first block ordinal and DC predictors
//   write    decode once more from the final entry; block ordinal n of the lane is block n % blocks_per_mcu of MCU
//            mcu0 + n / blocks_per_mcu, at jpeg_entropy_kernel's address.  Ordinals at or past the lane's block count
//            write nothing and flag nothing; the status bits are set by the one thread that meets the condition.
// Every loop consumes at least one bit per iteration or leaves: the symbol loop ends at the segment's end, at the
// lane's block count or, in the tail, at the next MCU boundary.
constexpr int kJpegSplitThreads = 64;   // segments per pass
constexpr int kJpegEnded = 1 << 9;      // state word: blk | k << 3 | ended

struct SegReader {
  const uint4 *base;
  long long pos, end;    // next byte to fetch (counts on past `end`, where bytes are zero) and the end of the data
  long long cidx;
  unsigned c0, c1, c2, c3;      // the 16-byte piece cidx
  unsigned long long acc, sk;   // next bit at the top; sk: a one under the last bit of a byte that a stuffed 00 followed
  int nbits;

  __device__ __forceinline__ unsigned byte_at(long long p) {
    if ((p >> 4) != cidx) {
      cidx = p >> 4;
      const uint4 c = base[cidx];
      c0 = c.x;
      c1 = c.y;
      c2 = c.z;
      c3 = c.w;
    }
    const int w = (int)(p >> 2) & 3;
    const unsigned v = w == 0 ? c0 : (w == 1 ? c1 : (w == 2 ? c2 : c3));
    return (v >> (((int)p & 3) * 8)) & 255u;
  }
  __device__ __forceinline__ void refill() {
    while (nbits <= 56) {
      unsigned b = 0;
      if (pos < end) {
        b = byte_at(pos++);
        if (b == 0xFFu && pos < end) {
          if (byte_at(pos) == 0) {
            ++pos;                 // FF 00: a stuffed zero
            sk |= 1ull << (56 - nbits);
          } else {                 // a marker inside the range: the entropy data ends here, this byte is the first zero
            end = pos - 1;
            b = 0;
          }
        }
      } else {
        ++pos;
      }
      acc |= (unsigned long long)b << (56 - nbits);
      nbits += 8;
    }
  }
  __device__ __forceinline__ void drop(int n) {
    acc <<= n;
    sk <<= n;
    nbits -= n;
  }
  __device__ __forceinline__ int take(int n) {   // n in 0 .. 16
    refill();
    const int v = n ? (int)(acc >> (64 - n)) : 0;
    drop(n);
    return v;
  }
  // canonical position of the next bit
  __device__ __forceinline__ long long front() const {
    return (pos - ((nbits + 7) >> 3) - __popcll(sk)) * 8 + ((8 - (nbits & 7)) & 7);
  }
  __device__ __forceinline__ void start(const uint4 *b, long long bit, long long e) {
    base = b;
    pos = bit >> 3;
    end = e;
    cidx = -1;
    c0 = c1 = c2 = c3 = 0;
    acc = sk = 0;
    nbits = 0;
    refill();
    drop((int)(bit & 7));
  }
};

__device__ __forceinline__ int huff_decode_seg(const unsigned char *t, SegReader &br) {   // huff_decode on a SegReader
  br.refill();
  const unsigned w = (unsigned)(br.acc >> 48);
  const unsigned e = ((const unsigned short *)t)[w >> 8];
  if (e >> 8) {
    br.drop((int)(e >> 8));
    return (int)(e & 255u);
  }
  const int *maxcode = (const int *)(t + 768), *valoff = (const int *)(t + 836);
  for (int l = 9; l <= 16; ++l) {
    const int code = (int)(w >> (16 - l));
    if (code <= maxcode[l]) {
      br.drop(l);
      return t[512 + ((code + valoff[l]) & 255)];
    }
  }
  return -1;
}

struct SplitLane {   // block-uniform: the lane and its image
  long long begin, end, mcu0, total, nbY, nblocks, nlb;
  int hv, hs, vs, mx, bpm;
  short *cbase;
};

// the 64 coefficients of block ordinal n of the lane; NULL where jpeg_entropy_kernel would not write
__device__ __forceinline__ short *split_block(const SplitLane &g, long long n) {
  const long long mcu = g.mcu0 + n / g.bpm;
  const int j = (int)(n % g.bpm);
  long long b;
  if (j < g.hv) {
    const int ym = (int)(mcu / g.mx), xm = (int)(mcu - (long long)ym * g.mx);
    b = (long long)(ym * g.vs + j / g.hs) * (g.mx * g.hs) + xm * g.hs + j % g.hs;
  } else {
    b = g.nbY + mcu + (j - g.hv) * g.total;
  }
  return (n < g.nlb && b >= 0 && b < g.nblocks) ? g.cbase + b * 64 : nullptr;
}

// Decodes from state (bit, m) to the end of the segment.  WRITE false: counts blocks into n and DC differences into
// p0 .. p2 (all zero on entry) and returns the exit state in (bit, m); guess: recover from invalid symbols, and return
// 1 if that happened -- such a result serves as a guess for the threads after it but must never become final.  WRITE
// true: n is the first block ordinal, p0 .. p2 the DC predictors; stores coefficients and returns the status bits.
template <bool WRITE>
__device__ __forceinline__ int split_run(const SplitLane &g, const uint4 *bytes, const unsigned char *tab,
                                         const unsigned char *nat, long long seg_end, bool guess, long long &bit, int &m,
                                         long long &n, int &p0, int &p1, int &p2) {
  SegReader br;
  br.start(bytes, bit, g.end);
  int blk = m & 7, k = (m >> 3) & 63, recovered = 0;
  short *out = nullptr;
  if (WRITE && k > 0) out = split_block(g, n);
  for (;;) {
    br.refill();
    if (WRITE && n >= g.nlb) return 0;
    if (br.pos >= seg_end || br.pos >= br.end) {   // near an end: look at the exact position
      const long long f = br.front();
      const bool tail = f >= br.end * 8;
      if (!tail && f >= seg_end * 8) {
        bit = f;
        m = blk | (k << 3);
        return WRITE ? 0 : recovered;
      }
      if (tail && !WRITE) {
        bit = 0;
        m = kJpegEnded;
        return recovered;
      }
    }
    const int c = blk < g.hv ? 0 : blk - g.hv + 1;
    bool bad = false;
    if (k == 0) {
      const int s = huff_decode_seg(tab + c * kHtBytes, br);
      if (s < 0 || s > 15) {
        bad = true;
      } else {
        const int diff = huff_extend(br.take(s), s);
        const int pred = (c == 0 ? p0 : (c == 1 ? p1 : p2)) + diff;
        p0 = c == 0 ? pred : p0;
        p1 = c == 1 ? pred : p1;
        p2 = c == 2 ? pred : p2;
        if (WRITE) {
          out = split_block(g, n);
          if (out) out[0] = (short)pred;
        }
        k = 1;
      }
    } else {
      const int rs = huff_decode_seg(tab + (3 + c) * kHtBytes, br);
      if (rs < 0) {
        bad = true;
      } else {
        const int r = rs >> 4, s = rs & 15;
        if (s == 0) {
          k = r != 15 ? 64 : k + 16;
        } else {
          k += r;
          if (k > 63) {
            bad = true;
          } else {
            const int v = huff_extend(br.take(s), s);
            if (WRITE && out) out[nat[k & 63]] = (short)v;
            ++k;
          }
        }
      }
    }
    if (bad) {
      if (WRITE) return XM_JPEG_BADCODE | (br.front() > br.end * 8 ? XM_JPEG_TRUNCATED : 0);
      if (!guess) {
        bit = 0;
        m = kJpegEnded;
        return 0;
      }
      br.refill();
      br.drop(1);   // a guess went wrong: one bit on, a DC symbol next
      k = 0;
      recovered = 1;
      continue;
    }
    if (k >= 64) {
      k = 0;
      ++n;
      blk = blk + 1 == g.bpm ? 0 : blk + 1;
      if (WRITE && (n >= g.nlb || blk == 0) && br.front() > br.end * 8) return XM_JPEG_TRUNCATED;
    }
  }
}

__global__ void __launch_bounds__(kJpegSplitThreads)
jpeg_entropy_split_kernel(const uint4 *__restrict__ bytes, long long nbytes, const long long *__restrict__ desc, int N,
                          const long long *__restrict__ lanes, int nlanes, const unsigned char *__restrict__ huff, int nh,
                          short *__restrict__ coef, int *__restrict__ status, int seg_bytes, int *__restrict__ rounds) {
  constexpr int T = kJpegSplitThreads;
  __shared__ __attribute__((aligned(16))) unsigned char s_tab[6 * kHtBytes];
  __shared__ unsigned char s_nat[64];
  __shared__ long long s_bit[T + 1];           // exit states; [T]: the confirmed entry of the pass
  __shared__ int s_m[T + 1];
  __shared__ int s_cnt[T][4];                  // blocks, dc0, dc1, dc2
  __shared__ long long s_n0;                   // blocks before the pass
  __shared__ int s_pred[3];
  const int tid = threadIdx.x;
  const long long gl = blockIdx.x;
  if (gl >= nlanes) return;
  const long long img = min(max(lanes[gl * kJpegLane], 0LL), (long long)N - 1);
  const long long *d = desc + img * kJpegDesc;
  s_nat[tid] = kNaturalDev[tid];
  for (int j = tid; j < 6 * (kHtBytes / 16); j += T) {
    const int tb = j / (kHtBytes / 16), q = j - tb * (kHtBytes / 16);
    const long long slot = d[tb < 3 ? D_DC + tb : D_AC + tb - 3];
    const long long sl = min(max(slot, 0LL), (long long)nh - 1);
    ((uint4 *)(s_tab + tb * kHtBytes))[q] = ((const uint4 *)(huff + sl * kHtBytes))[q];
  }
  // the lane's byte range, inside the image's, inside the buffer
  const long long i0 = min(max(d[D_SCAN0], 0LL), nbytes), i1 = min(max(d[D_SCAN1], i0), nbytes);
  SplitLane g;
  g.begin = min(max(lanes[gl * kJpegLane + 1], i0), i1);
  g.end = min(max(lanes[gl * kJpegLane + 2], g.begin), i1);
  const int ncomp = (int)d[D_NCOMP];
  g.hs = min(max((int)d[D_HS], 1), 2);
  g.vs = min(max((int)d[D_VS], 1), 2);
  g.mx = max((int)d[D_MX], 1);
  g.hv = g.hs * g.vs;
  g.bpm = g.hv + (ncomp == 3 ? 2 : 0);
  g.total = (long long)g.mx * max((int)d[D_MY], 0);
  const long long ri = d[D_RI];
  g.mcu0 = min(max(lanes[gl * kJpegLane + 3], 0LL), g.total);
  const long long stop = ri > 0 ? min(g.mcu0 + ri, g.total) : g.total;
  g.nbY = g.total * g.hv;
  g.nblocks = g.nbY + (ncomp == 3 ? 2 * g.total : 0);
  g.nlb = (stop - g.mcu0) * g.bpm;
  g.cbase = coef + d[D_COEF];
  const long long nseg = max((g.end - g.begin + seg_bytes - 1) / seg_bytes, 1LL);
  if (tid == 0) {
    s_bit[T] = g.begin * 8;
    s_m[T] = 0;
    s_n0 = 0;
    s_pred[0] = s_pred[1] = s_pred[2] = 0;
  }
  __syncthreads();
  int total_rounds = 0;
  for (long long seg0 = 0; seg0 < nseg; seg0 += T) {
    if (s_m[T] & kJpegEnded) break;            // the chain ended in an earlier pass (block-uniform)
    const int nact = (int)min((long long)T, nseg - seg0);
    const bool active = tid < nact;
    const long long sb = min(g.begin + (seg0 + tid) * seg_bytes, g.end), se = min(sb + seg_bytes, g.end);
    long long ebit = s_bit[T], xbit = 0, cnt = 0;
    int em = s_m[T], xm = 0, c0 = 0, c1 = 0, c2 = 0;
    if (tid > 0 && active) {                   // a guess: the first byte of the segment, or the one after a stuffed 00
      const unsigned char *raw = (const unsigned char *)bytes;
      const bool stuffed = sb > g.begin && sb < g.end && raw[sb] == 0 && raw[sb - 1] == 0xFFu;
      ebit = (sb + (stuffed ? 1 : 0)) * 8;
      em = 0;
    }
    bool redo = active, guess = tid > 0, unconfirmed = false;
    for (int r = 0;; ++r) {
      if (redo) {
        xbit = ebit;
        xm = em;
        cnt = 0;
        c0 = c1 = c2 = 0;
        unconfirmed = split_run<false>(g, bytes, s_tab, s_nat, se, guess, xbit, xm, cnt, c0, c1, c2) != 0;
        s_bit[tid] = xbit;
        s_m[tid] = xm;
      }
      __syncthreads();
      redo = false;
      guess = false;
      if (tid > 0 && active) {
        const long long pb = s_bit[tid - 1];
        const int pm = s_m[tid - 1];
        if (pb != ebit || pm != em) {
          ebit = pb;
          em = pm;
          redo = !(pm & kJpegEnded);           // an ended entry: keep the result, the scan marks this thread dead
        } else if (unconfirmed && !(em & kJpegEnded)) {   // the guess was right, but its decode skipped an invalid symbol
          redo = true;
        }
      }
      const int any = __syncthreads_or(redo);
      if (!any || r + 2 > nact) {
        total_rounds += r + 1;
        break;
      }
    }
    // scan: every thread sums what the threads before it published, at most T - 1 steps of five LDS reads -- small
    // next to a segment decode at T = 64; a wave scan would be the thing to use if T grew
    s_cnt[tid][0] = (int)cnt;
    s_cnt[tid][1] = c0;
    s_cnt[tid][2] = c1;
    s_cnt[tid][3] = c2;
    __syncthreads();
    long long n0 = s_n0;
    int p0 = s_pred[0], p1 = s_pred[1], p2 = s_pred[2];
    bool dead = !active || (em & kJpegEnded);
    for (int j = 0; j < tid && j < nact; ++j) {
      n0 += s_cnt[j][0];
      p0 += s_cnt[j][1];
      p1 += s_cnt[j][2];
      p2 += s_cnt[j][3];
      dead = dead || (s_m[j] & kJpegEnded);
    }
    // write
    if (!dead) {
      long long wbit = ebit, wn = n0;
      int wm = em, q0 = p0, q1 = p1, q2 = p2;
      const int st = split_run<true>(g, bytes, s_tab, s_nat, se, false, wbit, wm, wn, q0, q1, q2);
      if (st) atomicOr(status + img, st);
    }
    __syncthreads();
    if (tid == nact - 1) {                     // the carry into the next pass
      const bool ended = dead || (xm & kJpegEnded);
      s_bit[T] = ended ? 0 : xbit;
      s_m[T] = ended ? kJpegEnded : xm;
      s_n0 = n0 + cnt;
      s_pred[0] = p0 + c0;
      s_pred[1] = p1 + c1;
      s_pred[2] = p2 + c2;
    }
    __syncthreads();
  }
  if (rounds && tid == 0) rounds[gl] = total_rounds;
}

// ---- jpeg_idct_kernel ----------------------------------------------------------------------------------------------
#define XM_IDCT_1D(x0, x1, x2, x3, x4, x5, x6, x7, SHIFT)                                                   \
  {                                                                                                         \
    int z2 = x2, z3 = x6;                                                                                   \
    int z1 = (z2 + z3) * 4433;                                                                              \
    int tmp2 = z1 - z3 * 15137, tmp3 = z1 + z2 * 6270;                                                      \
    int tmp0 = (x0 + x4) * 8192, tmp1 = (x0 - x4) * 8192;                                                   \
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;           \
    tmp0 = x7;                                                                                              \
    tmp1 = x5;                                                                                              \
    tmp2 = x3;                                                                                              \
    tmp3 = x1;                                                                                              \
    z1 = tmp0 + tmp3;                                                                                       \
    z2 = tmp1 + tmp2;                                                                                       \
    z3 = tmp0 + tmp2;                                                                                       \
    int z4 = tmp1 + tmp3;                                                                                   \
    const int z5 = (z3 + z4) * 9633;                                                                        \
    tmp0 *= 2446;                                                                                           \
    tmp1 *= 16819;                                                                                          \
    tmp2 *= 25172;                                                                                          \
    tmp3 *= 12299;                                                                                          \
    z1 *= -7373;                                                                                            \
    z2 *= -20995;                                                                                           \
    z3 = z3 * -16069 + z5;                                                                                  \
    z4 = z4 * -3196 + z5;                                                                                   \
    tmp0 += z1 + z3;                                                                                        \
    tmp1 += z2 + z4;                                                                                        \
    tmp2 += z2 + z3;                                                                                        \
    tmp3 += z1 + z4;                                                                                        \
    const int rnd = 1 << ((SHIFT)-1);                                                                       \
    x0 = (tmp10 + tmp3 + rnd) >> (SHIFT);                                                                   \
    x7 = (tmp10 - tmp3 + rnd) >> (SHIFT);                                                                   \
    x1 = (tmp11 + tmp2 + rnd) >> (SHIFT);                                                                   \
    x6 = (tmp11 - tmp2 + rnd) >> (SHIFT);                                                                   \
    x2 = (tmp12 + tmp1 + rnd) >> (SHIFT);                                                                   \
    x5 = (tmp12 - tmp1 + rnd) >> (SHIFT);                                                                   \
    x3 = (tmp13 + tmp0 + rnd) >> (SHIFT);                                                                   \
    x4 = (tmp13 - tmp0 + rnd) >> (SHIFT);                                                                   \
  }

// libjpeg's range_limit table after the IDCT: the 10-bit two's-complement value plus 128, clamped to 0 .. 255
__device__ __forceinline__ unsigned idct_limit(int v) {
  v &= 1023;
  v = v >= 512 ? v - 1024 : v;
  return (unsigned)min(max(v + 128, 0), 255);
}

__global__ void __launch_bounds__(256)
jpeg_idct_kernel(const short *__restrict__ coef, long long nblocks_all, const long long *__restrict__ desc, int N,
                 const unsigned char *__restrict__ qtabs, int nq, unsigned char *__restrict__ planes) {
  const long long g = blockIdx.x * (long long)256 + threadIdx.x;
  if (g >= nblocks_all) return;
  const int img = find_image(desc, N, D_COEF, 64, g);
  const long long *d = desc + (long long)img * kJpegDesc;
  const int hs = (int)d[D_HS], vs = (int)d[D_VS], mx = (int)d[D_MX], my = (int)d[D_MY], ncomp = (int)d[D_NCOMP];
  const long long total = (long long)mx * my, nbY = total * hs * vs;
  const long long b = g - d[D_COEF] / 64;
  if (b >= nbY + (ncomp == 3 ? 2 * total : 0)) return;
  const int c = b < nbY ? 0 : (b < nbY + total ? 1 : 2);
  const long long lb = c == 0 ? b : b - nbY - (c - 1) * total;
  const int bw = c == 0 ? mx * hs : mx;
  const int by = (int)(lb / bw), bx = (int)(lb - (long long)by * bw);
  const long long slot = min(max(d[D_QT + c], 0LL), (long long)nq - 1);
  const uint4 *q4 = (const uint4 *)(qtabs + slot * kQtBytes);
  const uint4 *c4 = (const uint4 *)(coef + g * 64);
  int x[64];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint4 cv = c4[r], qv = q4[r];
    const unsigned cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[r * 8 + 2 * j] = (int)(short)(cw[j] & 0xFFFFu) * (int)(qw[j] & 0xFFFFu);
      x[r * 8 + 2 * j + 1] = (int)(short)(cw[j] >> 16) * (int)(qw[j] >> 16);
    }
  }
#pragma unroll
  for (int u = 0; u < 8; ++u)     // pass 1: columns
    XM_IDCT_1D(x[u], x[8 + u], x[16 + u], x[24 + u], x[32 + u], x[40 + u], x[48 + u], x[56 + u], 11);
  const long long ph = c == 0 ? (long long)my * vs * 8 : (long long)my * 8, pw = (long long)bw * 8;
  const long long pY = (long long)my * vs * 8 * ((long long)mx * hs * 8), pC = (long long)my * 8 * ((long long)mx * 8);
  unsigned char *plane = planes + d[D_PLANE] + (c == 0 ? 0 : pY + (c - 1) * pC);
  (void)ph;
#pragma unroll
  for (int r = 0; r < 8; ++r) {   // pass 2: rows
    XM_IDCT_1D(x[r * 8], x[r * 8 + 1], x[r * 8 + 2], x[r * 8 + 3], x[r * 8 + 4], x[r * 8 + 5], x[r * 8 + 6], x[r * 8 + 7], 18);
    uint2 o;
    o.x = idct_limit(x[r * 8]) | (idct_limit(x[r * 8 + 1]) << 8) | (idct_limit(x[r * 8 + 2]) << 16) | (idct_limit(x[r * 8 + 3]) << 24);
    o.y = idct_limit(x[r * 8 + 4]) | (idct_limit(x[r * 8 + 5]) << 8) | (idct_limit(x[r * 8 + 6]) << 16) | (idct_limit(x[r * 8 + 7]) << 24);
    *(uint2 *)(plane + ((long long)by * 8 + r) * pw + (long long)bx * 8) = o;
  }
}

// ---- jpeg_colour_kernel --------------------------------------------------------------------------------------------
// one upsampled chroma sample at (y, x) of the H x W image from a plane of dh x dw real samples (row pitch pw)
__device__ __forceinline__ int chroma_at(const unsigned char *__restrict__ p, long long pw, int dh, int dw, int hs, int vs,
                                         int y, int x) {
  if (hs == 1) return p[y * pw + x];
  if (dw <= 2) return p[(long long)(y / vs) * pw + (x >> 1)];     // jdsample.c: fancy only where downsampled_width > 2
  const int i = x >> 1, odd = x & 1;
  const int nb = odd ? min(i + 1, dw - 1) : max(i - 1, 0);
  if (vs == 1) return (3 * p[y * pw + i] + p[y * pw + nb] + (odd ? 2 : 1)) >> 2;
  const int near = y >> 1, far = (y & 1) ? min(near + 1, dh - 1) : max(near - 1, 0);
  const int cs = 3 * p[near * pw + i] + p[far * pw + i], cn = 3 * p[near * pw + nb] + p[far * pw + nb];
  return (3 * cs + cn + (odd ? 7 : 8)) >> 4;
}

__global__ void __launch_bounds__(256)
jpeg_colour_kernel(const unsigned char *__restrict__ planes, const long long *__restrict__ desc, int N,
                   long long npix_all, float *__restrict__ pixels) {
  const long long g = blockIdx.x * (long long)256 + threadIdx.x;
  if (g >= npix_all) return;
  const int img = find_image(desc, N, D_PIX, 3, g);
  const long long *d = desc + (long long)img * kJpegDesc;
  const int H = (int)d[D_H], W = (int)d[D_W], hs = (int)d[D_HS], vs = (int)d[D_VS], mx = (int)d[D_MX], my = (int)d[D_MY];
  const long long p = g - d[D_PIX] / 3;
  if (p >= (long long)H * W) return;
  const int x = (int)(p / H), y = (int)(p - (long long)x * H);
  const long long pwY = (long long)mx * hs * 8, pY = (long long)my * vs * 8 * pwY, pwC = (long long)mx * 8, pC = (long long)my * 8 * pwC;
  const unsigned char *base = planes + d[D_PLANE];
  const int Y = base[y * pwY + x];
  int r = Y, gg = Y, b = Y;
  if ((int)d[D_NCOMP] == 3) {
    const int dh = (H + vs - 1) / vs, dw = (W + hs - 1) / hs;
    const int cb = chroma_at(base + pY, pwC, dh, dw, hs, vs, y, x) - 128;
    const int cr = chroma_at(base + pY + pC, pwC, dh, dw, hs, vs, y, x) - 128;
    r = Y + ((91881 * cr + 32768) >> 16);
    gg = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
    b = Y + ((116130 * cb + 32768) >> 16);
  }
  float *o = pixels + d[D_PIX] + y + (long long)H * x;
  const long long HW = (long long)H * W;
  o[0] = (float)min(max(r, 0), 255);
  o[HW] = (float)min(max(gg, 0), 255);
  o[2 * HW] = (float)min(max(b, 0), 255);
}

// ---- host: parse ---------------------------------------------------------------------------------------------------
struct JpegImage {
  long long scan0 = 0, scan1 = 0;
  int H = 0, W = 0, ncomp = 0, hs = 1, vs = 1, ri = 0, mx = 0, my = 0;
  int tq[3] = {0, 0, 0}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
};

struct JpegTables {   // per file: what DQT / DHT defined
  bool hasq[4] = {false, false, false, false}, hash[2][4] = {{false, false, false, false}, {false, false, false, false}};
  unsigned short q[4][64];
  unsigned char h[2][4][kHtBytes];
};

static int parse_one(int idx, const unsigned char *d, long long n, JpegImage &im, JpegTables &tb,
                     std::vector<long long> &cuts) {
#define JBAD(...) return fail(XM_EINVAL, __VA_ARGS__)
#define JNOT(...) return fail(XM_ENOTSUP, __VA_ARGS__)
  if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) JBAD("jpeg_plan: file %d: no SOI marker", idx);
  long long pos = 2;
  bool have_frame = false;
  int adobe = -1, fid[3] = {0, 0, 0};
  for (;;) {
    if (pos + 2 > n) JBAD("jpeg_plan: file %d: cut inside its headers", idx);
    if (d[pos] != 0xFF) JBAD("jpeg_plan: file %d: marker expected at byte %lld", idx, pos);
    while (pos < n && d[pos] == 0xFF) ++pos;
    if (pos + 1 > n) JBAD("jpeg_plan: file %d: cut inside its headers", idx);
    const int m = d[pos++];
    if (m == 0xD9) JBAD("jpeg_plan: file %d: EOI before SOS", idx);
    if (pos + 2 > n) JBAD("jpeg_plan: file %d: cut inside its headers", idx);
    const long long L = (d[pos] << 8) | d[pos + 1];
    if (L < 2) JBAD("jpeg_plan: file %d: bad segment length", idx);
    if (pos + L > n) JBAD("jpeg_plan: file %d: cut inside its headers", idx);
    const unsigned char *s = d + pos + 2;
    const long long sl = L - 2;
    if (m == 0xDB) {
      long long q = 0;
      while (q < sl) {
        const int pq = s[q] >> 4, tq = s[q] & 15;
        if (pq) JNOT("jpeg_plan: file %d: 16-bit quantiser table", idx);
        if (tq > 3 || q + 65 > sl) JBAD("jpeg_plan: file %d: bad DQT segment", idx);
        for (int k = 0; k < 64; ++k) tb.q[tq][kNatural[k]] = s[q + 1 + k];
        tb.hasq[tq] = true;
        q += 65;
      }
    } else if (m == 0xC4) {
      long long q = 0;
      while (q < sl) {
        if (q + 17 > sl) JBAD("jpeg_plan: file %d: bad DHT segment", idx);
        const int tc = s[q] >> 4, th = s[q] & 15;
        int tot = 0;
        for (int k = 0; k < 16; ++k) tot += s[q + 1 + k];
        if (tc > 1 || th > 3 || tot > 256 || q + 17 + tot > sl) JBAD("jpeg_plan: file %d: bad DHT segment", idx);
        if (!derive_table(s + q + 1, s + q + 17, tot, tb.h[tc][th])) JBAD("jpeg_plan: file %d: invalid Huffman code lengths", idx);
        tb.hash[tc][th] = true;
        q += 17 + tot;
      }
    } else if (m == 0xC0) {
      if (sl < 6) JBAD("jpeg_plan: file %d: bad SOF segment", idx);
      if (s[0] != 8) JNOT("jpeg_plan: file %d: %d-bit samples", idx, (int)s[0]);
      im.H = (s[1] << 8) | s[2];
      im.W = (s[3] << 8) | s[4];
      const int nf = s[5];
      if (nf != 1 && nf != 3) JNOT("jpeg_plan: file %d: %d components (grey and YCbCr only)", idx, nf);
      if (sl < 6 + 3 * nf || im.H == 0 || im.W == 0) JBAD("jpeg_plan: file %d: bad SOF segment", idx);
      if (im.H > kJpegMaxSide || im.W > kJpegMaxSide)
        JNOT("jpeg_plan: file %d: %d x %d, supported up to %d x %d", idx, im.H, im.W, kJpegMaxSide, kJpegMaxSide);
      im.ncomp = nf;
      for (int i = 0; i < nf; ++i) {
        fid[i] = s[6 + 3 * i];
        const int h = s[7 + 3 * i] >> 4, v = s[7 + 3 * i] & 15;
        im.tq[i] = s[8 + 3 * i];
        if (i == 0) {
          im.hs = h;
          im.vs = v;
        } else if (h != 1 || v != 1) {
          JNOT("jpeg_plan: file %d: chroma sampling %d x %d (1 x 1 only)", idx, h, v);
        }
      }
      have_frame = true;
    } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8) {
      JNOT("jpeg_plan: file %d: SOF%d (progressive, arithmetic, lossless or 12-bit coding); baseline SOF0 only", idx, m - 0xC0);
    } else if (m == 0xDD) {
      if (sl < 2) JBAD("jpeg_plan: file %d: bad DRI segment", idx);
      im.ri = (s[0] << 8) | s[1];
    } else if (m == 0xEE && sl >= 12 && !memcmp(s, "Adobe", 5)) {
      adobe = s[11];
    } else if (m == 0xDA) {
      if (!have_frame) JBAD("jpeg_plan: file %d: SOS before SOF", idx);
      const int ns = sl ? s[0] : 0;
      if (sl < 1 + 2 * ns + 3) JBAD("jpeg_plan: file %d: bad SOS segment", idx);
      if (ns != im.ncomp) JNOT("jpeg_plan: file %d: multi-scan file (%d of %d components in the first scan)", idx, ns, im.ncomp);
      for (int i = 0; i < ns; ++i) {
        if (s[1 + 2 * i] != fid[i]) JNOT("jpeg_plan: file %d: scan components out of frame order", idx);
        im.td[i] = s[2 + 2 * i] >> 4;
        im.ta[i] = s[2 + 2 * i] & 15;
      }
      pos += L;
      break;
    }
    pos += L;
  }
  if (im.ncomp == 3) {
    if (adobe == 0) JNOT("jpeg_plan: file %d: Adobe transform 0 (RGB / CMYK data)", idx);
    if (!((im.hs == 1 && im.vs == 1) || (im.hs == 2 && im.vs == 1) || (im.hs == 2 && im.vs == 2)))
      JNOT("jpeg_plan: file %d: luma sampling %d x %d (1 x 1, 2 x 1, 2 x 2 only)", idx, im.hs, im.vs);
  } else {
    im.hs = im.vs = 1;   // a single component is never interleaved
  }
  for (int i = 0; i < im.ncomp; ++i)
    if (im.tq[i] > 3 || im.td[i] > 3 || im.ta[i] > 3 || !tb.hasq[im.tq[i]] || !tb.hash[0][im.td[i]] || !tb.hash[1][im.ta[i]])
      JBAD("jpeg_plan: file %d: component %d names a table the file does not define", idx, i);
  // the entropy data ends at the first marker that is neither a stuffed zero nor RSTn
  im.scan0 = pos;
  im.scan1 = n;
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
      im.scan1 = j;
      break;
    }
  }
  im.mx = (im.W + 8 * im.hs - 1) / (8 * im.hs);
  im.my = (im.H + 8 * im.vs - 1) / (8 * im.vs);
  return XM_OK;
#undef JBAD
#undef JNOT
}

}  // namespace xm

using namespace xm;

extern "C" {

int xm_jpeg_plan(const unsigned char *bytes, const long long *offsets, int N, long long *desc, long long *lanes,
                 long long lanes_cap, unsigned char *tables, long long tables_cap, long long *sizes) {
  if (N < 0 || lanes_cap < 0 || tables_cap < 0)
    return fail(XM_EINVAL, "jpeg_plan: need N >= 0, lanes_cap >= 0, tables_cap >= 0 (got N=%d lanes_cap=%lld tables_cap=%lld)", N,
                lanes_cap, tables_cap);
  if (!sizes) return fail(XM_EINVAL, "jpeg_plan: NULL sizes");
  for (int k = 0; k < XM_JPEG_SIZES; ++k) sizes[k] = 0;
  if (N == 0) return XM_OK;
  if (!bytes || !offsets || !desc || !lanes || !tables) return fail(XM_EINVAL, "jpeg_plan: NULL argument");
  std::vector<unsigned char> qpool, hpool;
  std::vector<long long> lane_rows, cuts;
  long long coef = 0, plane = 0, pix = 0;
  JpegTables *tb = new JpegTables;
  int rc = XM_OK;
  for (int i = 0; i < N && rc == XM_OK; ++i) {
    if (offsets[i] < 0 || offsets[i + 1] < offsets[i]) {
      rc = fail(XM_EINVAL, "jpeg_plan: file %d: offsets must ascend from 0", i);
      break;
    }
    JpegImage im;
    *tb = JpegTables();
    cuts.clear();
    rc = parse_one(i, bytes + offsets[i], offsets[i + 1] - offsets[i], im, *tb, cuts);
    if (rc) break;
    long long *d = desc + (long long)i * kJpegDesc;
    const long long base = offsets[i];
    d[D_SCAN0] = base + im.scan0;
    d[D_SCAN1] = base + im.scan1;
    d[D_H] = im.H;
    d[D_W] = im.W;
    d[D_NCOMP] = im.ncomp;
    d[D_HS] = im.hs;
    d[D_VS] = im.vs;
    d[D_RI] = im.ri;
    d[D_MX] = im.mx;
    d[D_MY] = im.my;
    for (int c = 0; c < 3; ++c) {
      const int s = c < im.ncomp ? c : 0;
      d[D_QT + c] = intern<kQtBytes>(qpool, (const unsigned char *)tb->q[im.tq[s]]);
      d[D_DC + c] = intern<kHtBytes>(hpool, tb->h[0][im.td[s]]);
      d[D_AC + c] = intern<kHtBytes>(hpool, tb->h[1][im.ta[s]]);
    }
    const long long total = (long long)im.mx * im.my;
    const long long nblocks = total * im.hs * im.vs + (im.ncomp == 3 ? 2 * total : 0);
    d[D_COEF] = coef;
    d[D_PLANE] = plane;
    d[D_PIX] = pix;
    coef += nblocks * 64;
    plane += nblocks * 64;
    pix += 3LL * im.H * im.W;
    d[D_LANE0] = (long long)(lane_rows.size() / kJpegLane);
    // one lane per restart interval; markers past the last interval of the image are ignored
    long long begin = im.scan0, k = 0;
    if (im.ri > 0) {
      for (size_t c = 0; c < cuts.size() && (k + 1) * im.ri < total; ++c, ++k) {
        const long long row[4] = {i, base + begin, base + cuts[c], k * im.ri};
        lane_rows.insert(lane_rows.end(), row, row + 4);
        begin = cuts[c] + 2;
      }
    }
    const long long row[4] = {i, base + begin, base + im.scan1, im.ri > 0 ? k * im.ri : 0};
    lane_rows.insert(lane_rows.end(), row, row + 4);
    d[D_NLANES] = (long long)(lane_rows.size() / kJpegLane) - d[D_LANE0];
    if (coef >= (1LL << 31) || pix >= (1LL << 31))
      rc = fail(XM_ETOOBIG, "jpeg_plan: the batch holds 2^31 or more coefficients or pixel values at file %d", i);
  }
  delete tb;
  if (rc) return rc;
  const long long nq = (long long)(qpool.size() / kQtBytes), nh = (long long)(hpool.size() / kHtBytes);
  const long long nl = (long long)(lane_rows.size() / kJpegLane);
  sizes[0] = (long long)(qpool.size() + hpool.size());
  sizes[1] = nq;
  sizes[2] = nh;
  sizes[3] = coef;
  sizes[4] = plane;
  sizes[5] = pix;
  sizes[6] = nl;
  sizes[7] = N;
  if (nl > lanes_cap) return fail(XM_ENOMEM, "jpeg_plan: %lld lanes, room for %lld", nl, lanes_cap);
  if (sizes[0] > tables_cap) return fail(XM_ENOMEM, "jpeg_plan: %lld table bytes, room for %lld", sizes[0], tables_cap);
  memcpy(lanes, lane_rows.data(), lane_rows.size() * sizeof(long long));
  memcpy(tables, qpool.data(), qpool.size());
  memcpy(tables + qpool.size(), hpool.data(), hpool.size());
  return XM_OK;
}

}  // extern "C"

// The launches of a decode around its entropy stage (jpeg_entropy.h): xm_jpeg_decode_batch, xm_jpeg_decode_batch_split and
// xm_jpeg_decode_batch_prog (csrc/jpeg_prog.hip) differ in that stage alone.
namespace xm {

int jpeg_decode_launch(const unsigned char *bytes, long long nbytes, const long long *desc, int N, const long long *lanes,
                       int nlanes, const unsigned char *tables, int nq, int nh, long long coef_elems, long long plane_bytes,
                       long long pixel_floats, float *pixels, float *faces, float crop, int Ho, int Wo, const float *avg3,
                       int *status, const JpegEntropyStage &stage, void *stream) {
  if (N < 0 || nbytes < 0 || nlanes < 0 || nq < 0 || nh < 0 || coef_elems < 0 || plane_bytes < 0 || pixel_floats < 0)
    return fail(XM_EINVAL, "jpeg_decode_batch: negative size");
  if (N == 0) return XM_OK;
  if (!bytes || !desc || !lanes || !tables || !status) return fail(XM_EINVAL, "jpeg_decode_batch: NULL argument");
  if (nlanes < N || nq < 1 || nh < stage.min_huff() || coef_elems < 64 || (coef_elems & 63) || plane_bytes != coef_elems || pixel_floats < 3)
    return fail(XM_EINVAL, "jpeg_decode_batch: sizes are not what xm_jpeg_plan reports");
  if (coef_elems >= (1LL << 31) || pixel_floats >= (1LL << 31)) return fail(XM_ETOOBIG, "jpeg_decode_batch: batch too large");
  if (((uintptr_t)bytes & 15) || ((uintptr_t)tables & 15) || ((uintptr_t)desc & 7) || ((uintptr_t)lanes & 7))
    return fail(XM_EINVAL, "jpeg_decode_batch: bytes and tables must be 16-byte aligned, desc and lanes 8-byte aligned");
  if (faces) {
    if (Ho <= 0 || Wo <= 0) return fail(XM_EINVAL, "jpeg_decode_batch: faces need Ho > 0, Wo > 0");
    if (!(crop > 0.f) || crop > 1.f) return fail(XM_EINVAL, "jpeg_decode_batch: crop must be in (0, 1]");
    if (too_big(Ho, Wo, 3, N)) return fail(XM_ETOOBIG, "jpeg_decode_batch: faces too large");
  }
  hipStream_t st = (hipStream_t)stream;
  WsCarver ws;
  const size_t need = WsCarver::need((size_t)coef_elems, 2) + WsCarver::need((size_t)plane_bytes, 1) +
                      (pixels ? 0 : WsCarver::need((size_t)pixel_floats, 4));
  int rc = ws.init(need, st);
  if (rc) return rc;
  short *coef = ws.take<short>((size_t)coef_elems);
  unsigned char *planes = ws.take<unsigned char>((size_t)plane_bytes);
  float *pix = pixels ? pixels : ws.take<float>((size_t)pixel_floats);
  const unsigned char *huff = tables + (size_t)nq * kQtBytes;
  {
    ProfScope ps(prof_key(kProfJpeg, 0), 0, st);
    const size_t n16 = (size_t)coef_elems / 8;
    hipLaunchKernelGGL(jpeg_clear_kernel, dim3((unsigned)std::min<size_t>((n16 + 255) / 256, 4096)), dim3(256), 0, st,
                       (uint4 *)coef, n16, status, N);
  }
  XM_LAUNCH_CHECK();
  rc = stage.launch(coef, huff, planes, st);
  if (rc) return rc;
  XM_LAUNCH_CHECK();
  {
    ProfScope ps(prof_key(kProfJpeg, 2), 0, st);
    const long long nb = coef_elems / 64;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, coef, nb, desc, N, tables, nq,
                       planes);
  }
  XM_LAUNCH_CHECK();
  {
    ProfScope ps(prof_key(kProfJpeg, 3), 0, st);
    const long long np = pixel_floats / 3;
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, planes, desc, N, np, pix);
  }
  XM_LAUNCH_CHECK();
  if (!faces) return XM_OK;
  ProfScope ps(prof_key(kProfJpeg, 4), 0, st);
  return face_ragged_launch(pix, desc, kJpegDesc, D_H, D_W, D_PIX, N, crop, Ho, Wo, avg3, faces, st);
}

namespace {

// seg_bytes == 0: one lane per restart interval; else the segment-parallel kernel, one block per lane
struct BaselineStage : JpegEntropyStage {
  const unsigned char *bytes;
  long long nbytes;
  const long long *desc, *lanes;
  int N, nlanes, nh, *status, seg_bytes, *rounds;
  int min_huff() const override { return 2; }   // a DC and an AC table
  int launch(short *coef, const unsigned char *huff, unsigned char *, hipStream_t st) const override {
    ProfScope ps(prof_key(kProfJpeg, seg_bytes ? 5 : 1), 0, st);
    if (seg_bytes)
      hipLaunchKernelGGL(jpeg_entropy_split_kernel, dim3((unsigned)nlanes), dim3(kJpegSplitThreads), 0, st,
                         (const uint4 *)bytes, nbytes, desc, N, lanes, nlanes, huff, nh, coef, status, seg_bytes, rounds);
    else
      hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)((nlanes + kJpegLanes - 1) / kJpegLanes)), dim3(64), 0, st,
                         (const uint4 *)bytes, nbytes, desc, N, lanes, nlanes, huff, nh, coef, status);
    return XM_OK;
  }
};

}  // namespace

static int jpeg_decode_baseline(const unsigned char *bytes, long long nbytes, const long long *desc, int N, const long long *lanes,
                                int nlanes, const unsigned char *tables, int nq, int nh, long long coef_elems,
                                long long plane_bytes, long long pixel_floats, float *pixels, float *faces, float crop, int Ho,
                                int Wo, const float *avg3, int *status, int seg_bytes, int *rounds, void *stream) {
  BaselineStage stage;
  stage.bytes = bytes;
  stage.nbytes = nbytes;
  stage.desc = desc;
  stage.lanes = lanes;
  stage.N = N;
  stage.nlanes = nlanes;
  stage.nh = nh;
  stage.status = status;
  stage.seg_bytes = seg_bytes;
  stage.rounds = rounds;
  return jpeg_decode_launch(bytes, nbytes, desc, N, lanes, nlanes, tables, nq, nh, coef_elems, plane_bytes, pixel_floats,
                            pixels, faces, crop, Ho, Wo, avg3, status, stage, stream);
}

}  // namespace xm

extern "C" {

int xm_jpeg_decode_batch(const unsigned char *bytes, long long nbytes, const long long *desc, int N, const long long *lanes,
                         int nlanes, const unsigned char *tables, int nq, int nh, long long coef_elems,
                         long long plane_bytes, long long pixel_floats, float *pixels, float *faces, float crop, int Ho,
                         int Wo, const float *avg3, int *status, void *stream) {
  return jpeg_decode_baseline(bytes, nbytes, desc, N, lanes, nlanes, tables, nq, nh, coef_elems, plane_bytes, pixel_floats,
                              pixels, faces, crop, Ho, Wo, avg3, status, 0, nullptr, stream);
}

int xm_jpeg_decode_batch_split(const unsigned char *bytes, long long nbytes, const long long *desc, int N,
                               const long long *lanes, int nlanes, const unsigned char *tables, int nq, int nh,
                               long long coef_elems, long long plane_bytes, long long pixel_floats, float *pixels,
                               float *faces, float crop, int Ho, int Wo, const float *avg3, int *status, int seg_bytes,
                               int *rounds, void *stream) {
  if (seg_bytes < 16 || seg_bytes > 65536 || (seg_bytes & 15))
    return fail(XM_EINVAL, "jpeg_decode_batch_split: seg_bytes must be a multiple of 16 in 16 .. 65536 (got %d)", seg_bytes);
  return jpeg_decode_baseline(bytes, nbytes, desc, N, lanes, nlanes, tables, nq, nh, coef_elems, plane_bytes, pixel_floats,
                              pixels, faces, crop, Ho, Wo, avg3, status, seg_bytes, rounds, stream);
}

int xm_jpeg_split_geometry(int *segments_per_pass, int *launches) {
  if (segments_per_pass) *segments_per_pass = kJpegSplitThreads;
  if (launches) *launches = 5;   // clear, entropy, IDCT, colour, faces
  return XM_OK;
}

}  // extern "C"

// The entropy reader that jpeg_entropy_kernel (csrc/jpeg.hip) and jpeg_entropy_prog_kernel (csrc/jpeg_prog.hip) share: the
// clamped byte reader with FF 00 unstuffing, the Huffman lookup on a table in LDS and the baseline block decode; and the
// launch sequence around an entropy stage, which jpeg.hip owns.
#pragma once
#include "jpeg_scan_plan.h"
#include "xm_common.h"

namespace xm {

constexpr int kJpegLanes = 4;        // lanes per 64-thread block of the entropy kernels

static __constant__ unsigned char kNaturalDev[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct BitReader {
  const uint4 *base;     // the batch's bytes, 16-byte pieces
  long long pos, end;    // next byte and the end of the lane's range (absolute offsets, inside the buffer)
  long long cidx;        // which piece `chunk` holds
  uint4 chunk;
  unsigned long long acc;   // next bit at the top
  int nbits, fake;          // bits in acc; zero bits appended past the end of the range (they sit at the tail)

  __device__ __forceinline__ unsigned byte_at(long long p) {
    if ((p >> 4) != cidx) {
      cidx = p >> 4;
      chunk = base[cidx];
    }
    const int w = (int)(p >> 2) & 3;
    const unsigned v = w == 0 ? chunk.x : (w == 1 ? chunk.y : (w == 2 ? chunk.z : chunk.w));
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
          } else {                 // a marker inside the range: the entropy data ends here
            end = pos - 1;
            pos = end;
            b = 0;
            fake = min(fake + 8, 1 << 30);
          }
        }
      } else {
        fake = min(fake + 8, 1 << 30);
      }
      acc |= (unsigned long long)b << (56 - nbits);
      nbits += 8;
    }
  }
  __device__ __forceinline__ void drop(int n) {
    acc <<= n;
    nbits -= n;
  }
  __device__ __forceinline__ int take(int n) {   // n in 0 .. 16
    refill();
    const int v = n ? (int)(acc >> (64 - n)) : 0;
    drop(n);
    return v;
  }
  __device__ __forceinline__ bool starved() const { return nbits < fake; }
};

// one Huffman table in LDS: lut[256] of (nbits << 8 | symbol), huffval[256], maxcode[17], valoff[17]
__device__ __forceinline__ int huff_decode(const unsigned char *t, BitReader &br) {
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

__device__ __forceinline__ int huff_extend(int v, int s) { return (s && v < (1 << (s - 1))) ? v - (1 << s) + 1 : v; }

// one block: 0 = fine, else XM_JPEG_BADCODE.  `out` holds 64 zeroed coefficients in row-major order.
__device__ __forceinline__ int decode_block(BitReader &br, const unsigned char *dc, const unsigned char *ac,
                                            const unsigned char *nat, int &pred, short *__restrict__ out) {
  int s = huff_decode(dc, br);
  if (s < 0 || s > 15) return XM_JPEG_BADCODE;
  pred += huff_extend(br.take(s), s);
  out[0] = (short)pred;
  int k = 1;
  while (k < 64) {
    const int rs = huff_decode(ac, br);
    if (rs < 0) return XM_JPEG_BADCODE;
    const int r = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (r != 15) break;
      k += 16;
      continue;
    }
    k += r;
    if (k > 63) return XM_JPEG_BADCODE;
    out[nat[k & 63]] = (short)huff_extend(br.take(s), s);
    ++k;
  }
  return 0;
}

// the image whose range [desc[i][col] / unit, desc[i + 1][col] / unit) holds g
__device__ __forceinline__ int find_image(const long long *__restrict__ desc, int N, int col, long long unit, long long g) {
  int lo = 0, hi = N - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (desc[(long long)mid * kJpegDesc + col] / unit <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// the entropy stage of a decode: enqueues its launches on `st`, writing the non-zero coefficients into the zeroed `coef`;
// `planes` (one byte per coefficient) is free for it to use until the IDCT, which follows, writes it
struct JpegEntropyStage {
  virtual int launch(short *coef, const unsigned char *huff, unsigned char *planes, hipStream_t st) const = 0;
  virtual int min_huff() const = 0;   // the fewest Huffman tables a plan for it can hold
  virtual ~JpegEntropyStage() {}
};

// checks the arguments, takes the workspace and enqueues clear, `stage`, IDCT, colour and (with faces) the face kernel
int jpeg_decode_launch(const unsigned char *bytes, long long nbytes, const long long *desc, int N, const long long *lanes,
                       int nlanes, const unsigned char *tables, int nq, int nh, long long coef_elems, long long plane_bytes,
                       long long pixel_floats, float *pixels, float *faces, float crop, int Ho, int Wo, const float *avg3,
                       int *status, const JpegEntropyStage &stage, void *stream);

}  // namespace xm

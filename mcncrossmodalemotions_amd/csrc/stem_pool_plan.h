// Integer planning of the fused stem chain (stem_pool_kernels.h, stem_pool.hip): work decomposition of stem_gram_kernel,
// conv_stem_bnpool_fwd_kernel and conv_stem_wgrad_pool_kernel, and the addresses of the pooled loads of the last.  Nothing
// from HIP (compiles with g++ -std=c++17; tests/stem_pool_plan_check.cpp checks it without a GPU): the host code AND the
// kernels call these functions, neither keeps a copy.
#pragma once
#include <cstddef>
#include <cstdint>

#include "fastdiv.h"

namespace xm {

XM_HD int sp_min(int a, int b) { return a < b ? a : b; }
XM_HD int sp_max(int a, int b) { return a > b ? a : b; }

// ---- units shared by the Gram and the backward kernel ------------------------------------------------------------------
// (sample, pair of output columns 2 jp, 2 jp + 1, 64 output rows [64 cp, 64 cp + 64)): what one wave multiplies at a time
struct SpUnit {
  int n, jp, cp;         // sample, column pair, 64-row chunk pair of this wave
  bool live;             // the unit exists and the wave's rows exist
  bool col1, chunk1;     // the second column / the second 32-row chunk exist
};
inline int sp_col_pairs(int Wo) { return (Wo + 1) / 2; }
inline int sp_row_groups(int Ho) { return (Ho + 255) / 256; }      // stem_gram_kernel: a block unit holds 256 output rows
inline int sp_chunk_pairs(int Ho) { return (Ho + 63) / 64; }       // conv_stem_wgrad_pool_kernel: a wave unit holds 64

// ---- stem_gram_kernel -------------------------------------------------------------------------------------------------
// BLOCK units (sample, column pair, group of 256 rows); block b walks the units tbase + q, q = b / 8, b / 8 + tstep, ...
// < tend of its eighth (b % 8) of the range; wave w of the block takes rows [64 (4 group + w), + 64) of the unit
inline int stem_pool_units(int N, int Ho, int Wo) { return N * sp_col_pairs(Wo) * sp_row_groups(Ho); }
inline int stem_pool_grid(int nunits, int occ) { return sp_min(256 * occ, (nunits + 7) / 8 * 8); }
constexpr int kSpGramOcc = 3;                                      // blocks per CU of stem_gram_kernel
inline size_t stem_gram_part_floats(int N, int Ho, int Wo) {       // scratch: one [64][64] partial per block
  return (size_t)stem_pool_grid(stem_pool_units(N, Ho, Wo), kSpGramOcc) * 64 * 64;
}
struct SpGramWalk {
  int tbase, tstep, tend, q0;
};
XM_HD SpGramWalk sp_gram_walk(int block, int grid, int nunits) {
  const int per = (nunits + 7) >> 3;
  SpGramWalk w;
  w.tbase = (block & 7) * per, w.tstep = grid >> 3;
  w.tend = sp_min(per, nunits - w.tbase);
  w.q0 = block >> 3;
  return w;
}
// divJG: (column pairs) * (256-row groups), divG: 256-row groups
XM_HD SpUnit sp_gram_unit(int unit, int wave, const FastDiv divJG, const FastDiv divG, int PI, int PJ) {
  SpUnit c;
  const uint32_t u = (uint32_t)unit;
  c.n = (int)fast_div(u, divJG);
  const uint32_t rem = u - (uint32_t)c.n * divJG.d;
  c.jp = (int)fast_div(rem, divG);
  c.cp = 4 * ((int)rem - c.jp * (int)divG.d) + wave;
  c.live = 64 * c.cp < PI;
  c.col1 = 2 * c.jp + 1 < PJ;
  c.chunk1 = 64 * c.cp + 32 < PI;
  return c;
}

// ---- conv_stem_bnpool_fwd_kernel --------------------------------------------------------------------------------------
// WAVE units (sample, strip of 63 window rows, segment of window columns, row tile of 32 filters), row tile fastest
constexpr int kSfStrip = 63;
struct SfPlan {
  int NS, SG, nunits, grid;
};
// segments of window columns per (sample, strip, row tile): the count that minimises (rounds of the resident waves) x
// (output columns of a unit, one of them computed twice per segment).  A partly filled last round costs a whole one:
// 11 segments at 32 spectrograms = 2112 units for 2048 waves ran 285 us, 10 segments 206 us; at 256 spectrograms one
// segment leaves a quarter of the waves idle and two make 1.5 rounds, four make exactly three.
inline SfPlan stem_fwd_plan(int N, int pHo, int pWo, int occ) {
  SfPlan p;
  p.NS = (pHo + kSfStrip - 1) / kSfStrip;
  const int slots = 256 * occ * 4;
  const long long base = (long long)N * p.NS * 3;
  long long best = -1;
  p.SG = 1;
  for (int sg = 1; sg <= sp_min(16, pWo); ++sg) {
    const long long rounds = (base * sg + slots - 1) / slots;
    const long long cost = rounds * (2 * ((pWo + sg - 1) / sg) + 1);
    if (best < 0 || cost < best) best = cost, p.SG = sg;
  }
  p.nunits = N * p.NS * p.SG * 3;
  p.grid = sp_min(256 * occ, (p.nunits + 3) / 4);
  return p;
}
struct SfUnit {
  int n, strip, seg, rt;
  int pw0, pw1;          // window columns [pw0, pw1) of the segment
};
XM_HD SfUnit sf_unit(int unit, const FastDiv div3, const FastDiv divSG, const FastDiv divNS, int pWo, int SG) {
  SfUnit c;
  const uint32_t uu = (uint32_t)unit;
  const uint32_t q3 = fast_div(uu, div3);
  c.rt = (int)(uu - q3 * 3u);
  const uint32_t qs = fast_div(q3, divSG);
  c.seg = (int)(q3 - qs * divSG.d);
  c.n = (int)fast_div(qs, divNS);
  c.strip = (int)(qs - (uint32_t)c.n * divNS.d);
  c.pw0 = c.seg * pWo / SG, c.pw1 = (c.seg + 1) * pWo / SG;
  return c;
}

// ---- conv_stem_wgrad_pool_kernel --------------------------------------------------------------------------------------
// WAVE units (sample, column pair, 64-row chunk pair), chunk pair fastest; a wave owns ONE row tile of 32 filters (rt) and
// walks the units wc, wc + nwc, ...  Grid: whole XCD rows of blocks whose waves split evenly over the three row tiles (a
// multiple of 24 blocks), two blocks per CU.
struct SpBwdPlan {
  int ncp, npair, nunits, grid, nwc;
};
inline SpBwdPlan stem_bwd_plan(int N, int Ho, int Wo) {
  SpBwdPlan p;
  p.ncp = sp_chunk_pairs(Ho), p.npair = sp_col_pairs(Wo);
  p.nunits = N * p.npair * p.ncp;
  p.grid = sp_min(504, ((p.nunits * 3 + 3) / 4 + 23) / 24 * 24);      // two blocks per CU, 63 per XCD
  p.nwc = p.grid * 4 / 3;
  return p;
}
// logical wave index: XCD x (blocks b % 8 == x) holds a contiguous range, so that the waves that work on neighbouring
// units at the same time -- and share pooled lines and source columns -- share an L2
struct SpWave {
  int wl, rt, wc;
};
XM_HD SpWave sp_bwd_wave(int block, int grid, int wv) {
  const int nb8 = grid >> 3;                                          // blocks per XCD (grid % 24 == 0)
  SpWave w;
  w.wl = ((block & 7) * nb8 + (block >> 3)) * 4 + wv;
  w.rt = w.wl % 3, w.wc = w.wl / 3;
  return w;
}
// divG: chunk pairs per column, divJG: column pairs per sample.  u >= nunits: the last unit's geometry, not live
XM_HD SpUnit sp_bwd_unit(int u, int nunits, const FastDiv divG, const FastDiv divJG, int PI, int PJ) {
  SpUnit c;
  const uint32_t uu = (uint32_t)sp_min(u, nunits - 1);
  const uint32_t q = fast_div(uu, divG);
  c.cp = (int)(uu - q * divG.d);
  c.n = (int)fast_div(q, divJG);
  c.jp = (int)(q - (uint32_t)c.n * divJG.d);
  c.live = u < nunits;
  c.col1 = 2 * c.jp + 1 < PJ;
  c.chunk1 = 64 * c.cp + 32 < PI;
  return c;
}

// ---- pooled loads of conv_stem_wgrad_pool_kernel ----------------------------------------------------------------------
// The pooled tensors are [pHo][pWo][M][N].  A buffer load's address is base + voffset + soffset: the lane part (voffset)
// is range-checked against the tensor's bytes, the scalar part (soffset, `so` below: sample, row tile, filter group,
// window column) is NOT -- so every load that is issued must lie inside the tensor by its arithmetic alone:
//   * a group of 16 filters 32 rt + 16 it .. + 15 that does not exist (>= M) is not loaded at all (wave-uniform);
//   * in a partly filled group a lane of a filter >= M hands the hardware an out-of-range voffset (kSpNoLoad): the load
//     returns zero without an access.  (Clamping the lane to the last existing plane instead needs a lane offset per GROUP:
//     six more address registers at the kernel's tightest point, measured as spills);
//   * a quad that reaches past its pooled column reads on in the columns behind it (ignored: vmask) -- except where that
//     would end behind the last plane of the tensor: there it is loaded early (shift) and re-aligned after the load.
// lane -> filter 32 rt + 16 it + lane / 4 of its wave's row tile: does it exist
XM_HD bool sp_filter_ok(int rt, int it, int lane, int M) { return 32 * rt + 16 * it + (lane >> 2) < M; }
struct SpCand {
  unsigned voff[2];      // per chunk h: element offset of the lane's quad inside a (sample, 16-filter group, window column 0) block
  unsigned vmask;        // bit 4 h + e: element e of the chunk-h quad is a window row of this column (< pHo)
  int shift[2];          // != 0 only at the end of the tensor's last plane: the quad was loaded `shift` rows early (> 3: none
                         // of its rows exists)
  bool anyshift;         // (wave-uniform) some lane of this unit has a shifted quad
  unsigned exoff;        // the window row 32 cp - 1 (lanes with qd < 2: window column p = qd): element offset inside a
                         // (sample, 16-filter group) block, or out of range (kSpNoLoad: no row in front or no such column)
  bool ok[2];            // window column p exists (wave-uniform)
  bool grp[2];           // filter group it exists (wave-uniform): its loads are issued
  int sbase;             // element offset of (sample, filter 32 rt, window column 0, window row 0)
  int jp;
};
constexpr unsigned kSpNoLoad = 0x3FFFFFFFu;   // element offset that is out of range as a 4-byte AND as a 1-byte offset
// pooledElems = pHo * pWo * M * N
XM_HD SpCand sp_cand_of(const SpUnit &c, int rt, int lane, int M, int pHo, int pWo, unsigned pooledElems) {
  const int pHW = pHo * pWo, cl = lane >> 2, qd = lane & 3;
  SpCand k;
  k.jp = c.jp;
  k.ok[1] = c.live && c.jp < pWo;
  k.ok[0] = c.live && c.jp >= 1 && c.jp - 1 < pWo;
  // (wave-uniform) the furthest quad of the unit -- last existing filter of the row tile, last window column, rows up to
  // 32 cp + 31 -- would end behind the tensor.  (With fewer than 32 window rows a quad reaches TWO columns or planes on:
  // pHo = 15 at the smallest admitted height, where more than the tensor's last column is shifted.)
  const int mlast = sp_min(32 * rt + 31, M - 1), cmax = sp_min(c.jp, pWo - 1);
  k.anyshift = (unsigned)(((c.n * M + mlast) * pWo + cmax) * pHo + 32 * c.cp + 32) > pooledElems;
  k.vmask = 0;
#ifdef __HIPCC__
#pragma unroll
#endif
  for (int h = 0; h < 2; ++h) {
    const int ph0 = 32 * c.cp + 16 * h + 4 * qd;        // first window row of the lane's quad
    const int phs = k.anyshift ? sp_min(ph0, pHo - 4) : ph0;
    k.shift[h] = ph0 - phs;
    k.voff[h] = (unsigned)(cl * pHW + phs);
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int e = 0; e < 4; ++e) k.vmask |= (ph0 + e < pHo ? 1u : 0u) << (4 * h + e);
  }
  const bool exok = c.cp > 0 && qd < 2 && (qd ? k.ok[1] : k.ok[0]);
  k.exoff = exok ? (unsigned)((cl * pWo + c.jp - 1 + qd) * pHo + 32 * c.cp - 1) : kSpNoLoad;
  k.grp[0] = 32 * rt < M, k.grp[1] = 32 * rt + 16 < M;
  k.sbase = (c.n * M + 32 * rt) * pHW;
  return k;
}
// scalar part (elements) of the quads of (group it, window column p = 0: jp - 1, 1: jp) and of the row in front
XM_HD bool sp_cand_issued(const SpCand &k, int it, int p) { return k.ok[p] && k.grp[it]; }
XM_HD int sp_cand_so(const SpCand &k, int it, int p, int pHo, int pWo) {
  return k.sbase + 16 * it * pHo * pWo + (k.jp - 1 + p) * pHo;
}
// lane part (elements) of a load of group it; `mine`: the lane's filter of that group exists (sp_filter_ok)
XM_HD unsigned sp_cand_voff(const SpCand &k, int h, bool mine) { return mine ? k.voff[h] : kSpNoLoad; }
XM_HD unsigned sp_cand_exoff(const SpCand &k, bool mine) { return mine ? k.exoff : kSpNoLoad; }
XM_HD int sp_cand_exso(const SpCand &k, int it, int pHo, int pWo) { return k.sbase + 16 * it * pHo * pWo; }

}  // namespace xm

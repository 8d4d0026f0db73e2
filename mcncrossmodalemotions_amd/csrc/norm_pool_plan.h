// Host-side planning of vl_nnbnorm, vl_nnpool and their fusion: integer arithmetic on the geometry, nothing from HIP
// (compiles with g++ -std=c++17; tests/norm_pool_plan_check.cpp holds it to the figures the GPU edge tests rely on).
// Sample splits, vector / scalar forks, block and grid geometry, the CAN half of every kernel's eligibility (addresses come
// in as uintptr_t) and each operator's scratch.  The WANT half -- path_on(kPathPool*) -- the validation, the template
// dispatch and the launches are norm_pool.hip's.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace xm {

// every address (pointer or uintptr_t; NULL counts as aligned) on a 16-byte boundary: the condition of the float4 arms
template <class... P>
inline bool aligned16(P... p) { return ((... | (uintptr_t)p) & 15) == 0; }

// grid of the grid-stride elementwise kernels: one block per 256 items, at most 2,048 blocks
inline unsigned ew_grid(size_t work_items) {
  size_t b = (work_items + 255) / 256;
  if (b > 256 * 8) b = 256 * 8;
  if (b < 1) b = 1;
  return (unsigned)b;
}

// ---- scratch: an operator describes its segments ONCE, as element counts; ws_bytes sums them for WsCarver::init and the
// operator takes them in the order of its struct (count == 0: the call does not take the segment) ----------------------
template <class T>
struct WsSeg { size_t count; };
template <class T>
inline size_t ws_bytes(WsSeg<T> s) { return (s.count * sizeof(T) + 255) & ~size_t(255); }   // WsCarver's rounding

// ============================== batch normalisation =========================================
// grid (C, S) of the reduction kernels: block (c, s) reduces samples s, s + S, ... of channel c
inline int bn_splits(int C, int N) {
  int s = 2048 / (C > 0 ? C : 1);
  if (s < 1) s = 1;
  if (s > N) s = N;
  return s;
}
// apply blocks per channel of the dxsum path: enough blocks to fill the chip, at most one per sample
inline int bn_dxsum_splits(int C, int N) { return std::max(1, std::min(N, 4096 / std::max(1, C))); }
// the float4 arms (bn_stats_partial_kernel, bn_apply_kernel<true>, bn_bwd_apply_kernel<true>, bn_bwd_apply_ch_kernel<true>)
// take whole pixel quads from 16-byte aligned tensors only (the caller of vl_nnconv with batch moments may hand in an
// output that is 4-byte aligned)
template <class... P>
inline bool bn_vec(int HW, P... p) { return (HW & 3) == 0 && aligned16(p...); }
// run length of one sample inside the flat (sample, position) index of the reduction kernels
inline int bn_run(int HW, bool vec) { return vec ? HW >> 2 : HW; }

// partial sums [C][S][2], sums [C][2], sum(dx) partials [C][S2], moments [C][2] (computed here and not handed back)
struct BnWs {
  WsSeg<double> part, sums, part2;
  WsSeg<float> mom;
  size_t bytes() const { return ws_bytes(part) + ws_bytes(sums) + ws_bytes(part2) + ws_bytes(mom); }
};
// npart partial sums per channel (0: none); backward: the sums; npart2 partials of sum(dx) (0: no dxsum)
inline BnWs bn_ws(int C, size_t npart, bool backward, size_t npart2, bool mom_scratch) {
  const size_t c = (size_t)C;
  return BnWs{{2 * c * npart}, {backward ? 2 * c : 0}, {c * npart2}, {mom_scratch ? 2 * c : 0}};
}

// ===================================== pooling ===============================================
struct PoolGeo {
  int H, W, Ho, Wo, ph, pw, sy, sx, pt, pl;
};
inline int pow2_ge(int v, int cap) {
  int p = 1;
  while (p < v && p < cap) p <<= 1;
  return p;
}

// 2-D indexing shared by the pooling kernels: threadIdx.x runs along the contiguous H axis,
// (blockIdx.x * blockDim.y + threadIdx.y) along W, blockIdx.y (+ grid-stride) over C*N planes --
// no per-element integer division.
struct PoolLaunch {
  int bx, by, bz, gx, gy, gz;
};
inline PoolLaunch pool_launch(int rows, int cols, long long planes) {
  // 256 threads = bx (rows, contiguous) x by (cols) x bz (planes): small planes pack several
  // planes into one block instead of idling lanes
  PoolLaunch l;
  l.bx = pow2_ge(rows, 256), l.by = pow2_ge(cols, 256 / l.bx), l.bz = 256 / (l.bx * l.by);
  // ~8k blocks in total: each block then strides over several planes (amortises block start-up)
  l.gx = (cols + l.by - 1) / l.by, l.gz = (rows + l.bx - 1) / l.bx;
  const long long pg = (planes + l.bz - 1) / l.bz, gy = std::max<long long>(1, 8192 / ((long long)l.gx * l.gz));
  l.gy = (int)std::min<long long>(std::min<long long>(gy, pg), 65535);
  return l;
}

// pool_global_kernel: the window is the whole unpadded plane; no routing table, no fused producer
inline bool pool_is_global(const PoolGeo &g, bool table, bool fused) {
  return !table && !fused && g.Ho == 1 && g.Wo == 1 && g.ph >= g.H && g.pw >= g.W && !(g.pt | g.pl);
}
// at most 2 x 2 windows cover an input element: pool_bwd_kernel<true>, and the only case the fused backward is written for
inline bool pool_cover_2x2(const PoolGeo &g) { return (g.ph + g.sy - 1) / g.sy <= 2 && (g.pw + g.sx - 1) / g.sx <= 2; }

// pool_fwd_lds_kernel<3, 3>: max pooling, 3 x 3 window, planes large enough to fill a block, 16-byte aligned tensor; a
// block owns `wob` output columns of a plane (`groups` blocks per plane) and stages the `ncols` input columns under them
struct PoolLds {
  bool run;
  int groups, wob, ncols;
  size_t lds_bytes;
};
inline PoolLds pool_lds_plan(const PoolGeo &g, bool max_pool, uintptr_t x) {
  PoolLds p{false, 0, 0, 0, 0};
  if (!max_pool || g.ph != 3 || g.pw != 3 || !aligned16(x) || g.Ho * g.Wo < 256) return p;
  const int maxcols = 16 * 256 / g.H;  // 16 KB of LDS per block: 10 blocks per CU, measured best of 8 / 16 / 32 / 64
  const int wob = std::min(maxcols >= g.pw ? (maxcols - g.pw) / g.sx + 1 : 0, g.Wo);
  if (wob < 1 || (wob < 4 && wob != g.Wo)) return p;
  p.run = true;
  p.groups = (g.Wo + wob - 1) / wob;
  p.wob = (g.Wo + p.groups - 1) / p.groups;   // even out the column groups (the last block would otherwise hold a sliver)
  p.ncols = (p.wob - 1) * g.sx + g.pw;
  p.lds_bytes = ((size_t)p.ncols * g.H + 8) * sizeof(float);
  return p;
}

// ---- fused backward of vl_nnpool('max') o vl_nnrelu o vl_nnbnorm ------------------------------
struct BnPoolBwd {
  int bx, by, gx, gz, S;                // element kernels: (bx, by) threads own (h, w); grid (gx, C, gz * S): N split S ways
  int KH, KW, pbx, pby, pgx, pgz, pS;   // patch kernel (apply): threads own the KH x KW stride cells; grid (pgx, C, pgz * pS)
  bool patch_can, vec2;                 // ... its instantiated strides; the two rows of a patch column as one 8-byte access
  int S2;                               // pooled-domain sums: grid (C, S2)
  bool pooled_can;                      // ... they read the pooled output
  // partial sums per channel that bn_bwd_finalize_kernel / sum_partials_kernel add up
  size_t npart(bool pooled) const { return pooled ? (size_t)S2 : (size_t)gx * gz * S; }
  size_t npart2(bool patch) const { return patch ? (size_t)pgx * pgz * pS : (size_t)gx * gz * S; }
};
inline BnPoolBwd bnpool_bwd_plan(const PoolGeo &g, int C, int N, uintptr_t x, uintptr_t dx, bool y_pool) {
  BnPoolBwd p;
  p.bx = pow2_ge(g.H, 256), p.by = pow2_ge(g.W, 256 / p.bx);
  p.gx = (g.W + p.by - 1) / p.by, p.gz = (g.H + p.bx - 1) / p.bx;
  p.S = std::max(1, std::min(N, 4096 / std::max(1, C * p.gx * p.gz)));
  p.KH = (g.H + g.pt + g.sy - 1) / g.sy, p.KW = (g.W + g.pl + g.sx - 1) / g.sx;
  p.pbx = pow2_ge(p.KH, 256), p.pby = pow2_ge(p.KW, 256 / p.pbx);
  p.pgx = (p.KW + p.pby - 1) / p.pby, p.pgz = (p.KH + p.pbx - 1) / p.pbx;
  p.pS = std::max(1, std::min(N, 16384 / std::max(1, C * p.pgx * p.pgz)));   // >= 16 k blocks (4 k and 64 k measured worse)
  p.patch_can = dx != 0 && ((g.sy == 2 && g.sx == 2) || (g.sy == 3 && g.sx == 2));
  p.vec2 = g.sy == 2 && (g.H & 1) == 0 && (g.pt & 1) == 0 && ((x | dx) & 7) == 0;
  p.S2 = bn_splits(C, N);
  p.pooled_can = y_pool;
  return p;
}

}  // namespace xm

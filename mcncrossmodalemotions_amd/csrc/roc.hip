// vl_roc / vl_tpfp of vlfeat (emoVoxCeleb/student_stats.m:109-125) and histcounts of the dominant emotion
// (student_stats.m:65-68,97-100, teacher_stats.m:28-29,57) on gfx950.
//
// xm_roc: G x E ranking problems per call.  Problem (g, c) owns the contiguous slice [c nnz + off[g], c nnz + off[g+1])
// of four nnz x E scratch arrays (key, position; double-buffered).  The slice is cut into tiles of kTile entries, one
// workgroup per tile, so a 118,485-row problem spreads over 58 workgroups and a call of 3 x 8 problems over ~600.
//   keys      key = order-reversing transform of the score, payload = position in `rows`; p, n, retrieved by integer atomics
//   4 passes  stable LSD radix sort, 8 bits each: per-tile digit histogram -> per-problem exclusive scan over
//             (digit, tile) -> stable scatter (rank inside the tile by wave-level digit matching)
//   curve     per-tile positives -> per-problem scan over tiles -> cumulative tp per rank, perm / tp outputs, and
//             S = sum over retrieved negatives of tp, added up with 64-bit integer atomics
//   finish    auc = S / (p n)
// 18 launches whatever G and E are.  Only integers are accumulated, so every output bit is a function of the problem's
// own rows: independent of G, of the order of the sets and of how the tiles are scheduled.  The sort is stable because
// an LSD pass keeps the order of equal digits and the initial order is the order of `rows`.
//
// xm_group_rows (fetch_emovoxceleb_imdb.m:140-148) sorts the frames by the group their wav id belongs to with the same
// passes, as one problem: id -> group through a slot table, (group, position) through the four passes, offsets as lower
// bounds in the sorted keys.  16 launches; no float atomics, integer LDS atomics only (the tile histograms).
#include "xm_common.h"

namespace xm {

constexpr int kRocThreads = 256;
constexpr int kRocWaves = kRocThreads / 64;
constexpr int kRocItems = 8;                              // entries per thread
constexpr int kRocWaveSpan = 64 * kRocItems;              // consecutive entries owned by one wave
constexpr int kTile = kRocThreads * kRocItems;            // 2048
constexpr unsigned kNegInfKey = 0xFF800000u;              // the key of -Inf: larger than the key of every score > -Inf
constexpr int kRocNanBit = 1, kRocBadBit = 2;             // raw per-problem flags, turned into XM_ROC_* by the last kernel
constexpr int kHistClassesMax = 4096;                     // xm_label_hist: one LDS counter per class, 16 KiB at the limit

// descending order of the scores = ascending order of the keys; -0.0 and +0.0 share a key
__device__ __forceinline__ unsigned roc_key(float s) {
  unsigned u = s == 0.f ? 0u : __float_as_uint(s);
  u = (u >> 31) ? ~u : (u | 0x80000000u);
  return ~u;
}

struct RocTile {
  int g, seg0, begin, end;   // problem, first entry of its set, entries [begin, end) of this tile (positions in rows)
};

// tile t of a column: tile_start[g] <= t < tile_start[g + 1]; false for the unused tail of the grid
__device__ __forceinline__ bool roc_locate(int t, const int *__restrict__ tile_start, const int *__restrict__ offsets,
                                           int G, RocTile &o) {
  if (t >= tile_start[G]) return false;
  int lo = 0, hi = G;   // invariant: tile_start[lo] <= t < tile_start[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tile_start[mid] <= t) lo = mid;
    else hi = mid;
  }
  o.g = lo;
  o.seg0 = offsets[lo];
  o.begin = o.seg0 + (t - tile_start[lo]) * kTile;
  o.end = min(o.begin + kTile, offsets[lo + 1]);
  return true;
}

__device__ __forceinline__ int roc_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one workgroup: checks the offsets, numbers the tiles of every set (tile_start[0 .. G], [G + 1] = bad-offsets flag)
// and clears the accumulators
__global__ void __launch_bounds__(kRocThreads)
roc_setup_kernel(const int *__restrict__ offsets, int G, int E, int nnz, int *__restrict__ tile_start,
                 long long *__restrict__ area, int *__restrict__ counts, int *__restrict__ status) {
  __shared__ int part[kRocThreads];
  __shared__ int bad;
  const int tid = threadIdx.x;
  if (tid == 0) bad = 0;
  __syncthreads();
  for (int g = tid; g < G; g += kRocThreads) {
    const int a = offsets[g], b = offsets[g + 1];
    if (a < 0 || b < a || b > nnz) atomicOr(&bad, 1);
  }
  __syncthreads();
  const bool isbad = bad != 0;
  const int chunk = (G + kRocThreads - 1) / kRocThreads;
  const int g0 = min(tid * chunk, G), g1 = min(g0 + chunk, G);
  int sum = 0;
  if (!isbad)
    for (int g = g0; g < g1; ++g) sum += (offsets[g + 1] - offsets[g] + kTile - 1) / kTile;
  part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int i = 0; i < kRocThreads; ++i) {
      const int v = part[i];
      part[i] = run;
      run += v;
    }
    tile_start[G] = run;
    tile_start[G + 1] = isbad ? 1 : 0;
  }
  __syncthreads();
  int run = part[tid];
  for (int g = g0; g < g1; ++g) {
    tile_start[g] = run;
    if (!isbad) run += (offsets[g + 1] - offsets[g] + kTile - 1) / kTile;
  }
  for (int i = tid; i < E * G; i += kRocThreads) {
    area[i] = 0;
    status[i] = isbad ? kRocBadBit : 0;
    counts[3 * i] = counts[3 * i + 1] = counts[3 * i + 2] = 0;
  }
}

__global__ void __launch_bounds__(kRocThreads)
roc_keys_kernel(const float *__restrict__ scores, int n, int E, const int *__restrict__ cls,
                const int *__restrict__ offsets, const int *__restrict__ rows, int nnz, int G,
                const int *__restrict__ tile_start, unsigned *__restrict__ keys, unsigned *__restrict__ pos,
                int *__restrict__ counts, int *__restrict__ status) {
  RocTile t;
  if (!roc_locate(blockIdx.x, tile_start, offsets, G, t)) return;
  const int c = blockIdx.y;
  const size_t col = (size_t)c * nnz;
  int np = 0, nn = 0, nr = 0, flags = 0;
  for (int i = t.begin + threadIdx.x; i < t.end; i += kRocThreads) {
    const int row = rows[i];
    unsigned key = kNegInfKey;
    if (row < 1 || row > n) {
      flags |= kRocBadBit;
    } else {
      const float s = scores[(size_t)(row - 1) + (size_t)n * c];
      if (cls[row - 1] == c + 1) ++np;
      else ++nn;
      if (s != s) {
        flags |= kRocNanBit;
      } else {
        key = roc_key(s);
        if (key != kNegInfKey) ++nr;
      }
    }
    keys[col + i] = key;
    pos[col + i] = (unsigned)i;
  }
  np = roc_wave_sum(np);
  nn = roc_wave_sum(nn);
  nr = roc_wave_sum(nr);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) flags |= __shfl_xor(flags, o, 64);
  if ((threadIdx.x & 63) == 0) {
    int *cnt = counts + 3 * ((size_t)c + (size_t)E * t.g);
    if (np) atomicAdd(cnt, np);
    if (nn) atomicAdd(cnt + 1, nn);
    if (nr) atomicAdd(cnt + 2, nr);
    if (flags) atomicOr(status + c + (size_t)E * t.g, flags);
  }
}

__global__ void __launch_bounds__(kRocThreads)
roc_hist_kernel(const unsigned *__restrict__ keys, const int *__restrict__ offsets, int nnz, int G,
                const int *__restrict__ tile_start, int Tc, int shift, unsigned *__restrict__ hist) {
  __shared__ unsigned h[256];
  RocTile t;
  if (!roc_locate(blockIdx.x, tile_start, offsets, G, t)) return;
  const int c = blockIdx.y;
  h[threadIdx.x] = 0;
  __syncthreads();
  const unsigned *k = keys + (size_t)c * nnz;
  for (int i = t.begin + threadIdx.x; i < t.end; i += kRocThreads) atomicAdd(&h[(k[i] >> shift) & 255u], 1u);
  __syncthreads();
  hist[((size_t)c * Tc + blockIdx.x) * 256 + threadIdx.x] = h[threadIdx.x];
}

// per problem: counts[tile][digit] -> the number of entries of the problem that precede (digit, tile) in the order
// (digit ascending, then tile ascending); thread d owns digit d
__global__ void __launch_bounds__(kRocThreads)
roc_scan_kernel(const int *__restrict__ tile_start, int Tc, unsigned *__restrict__ hist) {
  __shared__ unsigned tot[256];
  const int g = blockIdx.x, c = blockIdx.y, d = threadIdx.x;
  const int t0 = tile_start[g], t1 = tile_start[g + 1];
  unsigned *h = hist + ((size_t)c * Tc + t0) * 256 + d;
  unsigned sum = 0;
  for (int t = 0; t < t1 - t0; ++t) sum += h[(size_t)t * 256];
  tot[d] = sum;
  __syncthreads();
  if (d == 0) {
    unsigned run = 0;
    for (int i = 0; i < 256; ++i) {
      const unsigned v = tot[i];
      tot[i] = run;
      run += v;
    }
  }
  __syncthreads();
  unsigned run = tot[d];
  for (int t = 0; t < t1 - t0; ++t) {
    const unsigned v = h[(size_t)t * 256];
    h[(size_t)t * 256] = run;
    run += v;
  }
}

// Stable scatter of one tile.  Wave w owns entries [w kRocWaveSpan, (w + 1) kRocWaveSpan) of the tile and walks them 64
// at a time; the lanes holding the same digit find each other with eight ballots, an entry's rank among the wave's
// earlier entries of its digit is the running per-wave count plus the number of lower lanes in its group.
__global__ void __launch_bounds__(kRocThreads)
roc_scatter_kernel(const unsigned *__restrict__ keys_in, const unsigned *__restrict__ pos_in,
                   unsigned *__restrict__ keys_out, unsigned *__restrict__ pos_out, const int *__restrict__ offsets,
                   int nnz, int G, const int *__restrict__ tile_start, int Tc, int shift,
                   const unsigned *__restrict__ hist) {
  __shared__ unsigned cnt[kRocWaves][256];
  RocTile t;
  if (!roc_locate(blockIdx.x, tile_start, offsets, G, t)) return;
  const int c = blockIdx.y, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const size_t col = (size_t)c * nnz;
  for (int i = tid; i < kRocWaves * 256; i += kRocThreads) (&cnt[0][0])[i] = 0;
  __syncthreads();
  unsigned key[kRocItems], id[kRocItems], rk[kRocItems];
  const unsigned long long lower = (1ull << lane) - 1ull;
#pragma unroll
  for (int r = 0; r < kRocItems; ++r) {
    const int i = t.begin + w * kRocWaveSpan + r * 64 + lane;
    const bool valid = i < t.end;
    key[r] = valid ? keys_in[col + i] : 0u;
    id[r] = valid ? pos_in[col + i] : 0u;
    const unsigned d = (key[r] >> shift) & 255u;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bal = __ballot(bit);
      peers &= bit ? bal : ~bal;
    }
    const unsigned prior = valid ? cnt[w][d] : 0u;
    rk[r] = prior + (unsigned)__popcll(peers & lower);
    __syncthreads();   // every lane of the group has read the count before its last lane moves it
    if (valid && lane == 63 - __clzll(peers)) cnt[w][d] = prior + (unsigned)__popcll(peers);
    __syncthreads();
  }
  {   // per-wave totals -> entries of the earlier waves of this tile, per digit (thread d owns digit d)
    unsigned run = 0;
#pragma unroll
    for (int q = 0; q < kRocWaves; ++q) {
      const unsigned v = cnt[q][tid];
      cnt[q][tid] = run;
      run += v;
    }
  }
  __syncthreads();
  const unsigned *h = hist + ((size_t)c * Tc + blockIdx.x) * 256;
  const size_t base = col + (size_t)t.seg0;
#pragma unroll
  for (int r = 0; r < kRocItems; ++r) {
    const int i = t.begin + w * kRocWaveSpan + r * 64 + lane;
    if (i < t.end) {
      const unsigned d = (key[r] >> shift) & 255u;
      const size_t dst = base + h[d] + cnt[w][d] + rk[r];
      keys_out[dst] = key[r];
      pos_out[dst] = id[r];
    }
  }
}

__device__ __forceinline__ bool roc_positive(const int *__restrict__ rows, const int *__restrict__ cls, int n, unsigned id,
                                             int c, int &row) {
  row = rows[id];
  return row >= 1 && row <= n && cls[row - 1] == c + 1;
}

__global__ void __launch_bounds__(kRocThreads)
roc_tilepos_kernel(const unsigned *__restrict__ pos, const int *__restrict__ rows, const int *__restrict__ cls, int n,
                   const int *__restrict__ offsets, int nnz, int G, const int *__restrict__ tile_start, int Tc,
                   unsigned *__restrict__ tile_pos) {
  __shared__ int wsum[kRocWaves];
  RocTile t;
  if (!roc_locate(blockIdx.x, tile_start, offsets, G, t)) return;
  const int c = blockIdx.y;
  const unsigned *p = pos + (size_t)c * nnz;
  int np = 0, row;
  for (int i = t.begin + threadIdx.x; i < t.end; i += kRocThreads) np += roc_positive(rows, cls, n, p[i], c, row) ? 1 : 0;
  np = roc_wave_sum(np);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = np;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int q = 0; q < kRocWaves; ++q) s += wsum[q];
    tile_pos[(size_t)c * Tc + blockIdx.x] = (unsigned)s;
  }
}

// per problem: positives per tile -> positives in the earlier tiles of the problem
__global__ void __launch_bounds__(kRocThreads)
roc_scanpos_kernel(const int *__restrict__ tile_start, int Tc, unsigned *__restrict__ tile_pos) {
  __shared__ unsigned part[kRocThreads];
  const int g = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
  const int t0 = tile_start[g], nt = tile_start[g + 1] - t0;
  unsigned *v = tile_pos + (size_t)c * Tc + t0;
  const int chunk = (nt + kRocThreads - 1) / kRocThreads;
  const int a = min(tid * chunk, nt), b = min(a + chunk, nt);
  unsigned sum = 0;
  for (int t = a; t < b; ++t) sum += v[t];
  part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    unsigned run = 0;
    for (int i = 0; i < kRocThreads; ++i) {
      const unsigned x = part[i];
      part[i] = run;
      run += x;
    }
  }
  __syncthreads();
  unsigned run = part[tid];
  for (int t = a; t < b; ++t) {
    const unsigned x = v[t];
    v[t] = run;
    run += x;
  }
}

// tp at every rank of the tile (same entry order as the scatter), the curve outputs, and the tile's share of
// S = sum over retrieved negatives of the positives ranked before them
__global__ void __launch_bounds__(kRocThreads)
roc_curve_kernel(const unsigned *__restrict__ keys, const unsigned *__restrict__ pos, const int *__restrict__ rows,
                 const int *__restrict__ cls, int n, int E, const int *__restrict__ offsets, int nnz, int G,
                 const int *__restrict__ tile_start, int Tc, const unsigned *__restrict__ tile_pos,
                 long long *__restrict__ area, int *__restrict__ perm_out, int *__restrict__ tp_out) {
  __shared__ unsigned wtot[kRocWaves];
  RocTile t;
  if (!roc_locate(blockIdx.x, tile_start, offsets, G, t)) return;
  const int c = blockIdx.y, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const size_t col = (size_t)c * nnz;
  unsigned long long bal[kRocItems];
  int row[kRocItems];
  bool retrieved[kRocItems];
  unsigned total = 0;
#pragma unroll
  for (int r = 0; r < kRocItems; ++r) {
    const int i = t.begin + w * kRocWaveSpan + r * 64 + lane;
    bool p = false;
    row[r] = 0;
    retrieved[r] = false;
    if (i < t.end) {
      p = roc_positive(rows, cls, n, pos[col + i], c, row[r]);
      retrieved[r] = keys[col + i] != kNegInfKey;
    }
    bal[r] = __ballot(p);
    total += (unsigned)__popcll(bal[r]);
  }
  if (lane == 0) wtot[w] = total;
  __syncthreads();
  unsigned run = tile_pos[(size_t)c * Tc + blockIdx.x];
  for (int q = 0; q < w; ++q) run += wtot[q];
  const unsigned long long upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;
  unsigned long long S = 0;
#pragma unroll
  for (int r = 0; r < kRocItems; ++r) {
    const int i = t.begin + w * kRocWaveSpan + r * 64 + lane;
    const unsigned tp = run + (unsigned)__popcll(bal[r] & upto);
    run += (unsigned)__popcll(bal[r]);
    if (i < t.end) {
      if (perm_out) {
        perm_out[col + i] = row[r];
        tp_out[col + i] = (int)tp;
      }
      if (retrieved[r] && !((bal[r] >> lane) & 1ull)) S += tp;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) S += __shfl_xor(S, o, 64);
  if (lane == 0 && S) atomicAdd((unsigned long long *)(area + c + (size_t)E * t.g), S);
}

__global__ void roc_finish_kernel(int EG, const int *__restrict__ tile_start, int G, const long long *__restrict__ area,
                                  const int *__restrict__ counts, double *__restrict__ auc, int *__restrict__ status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= EG) return;
  const int st = status[i] | (tile_start[G + 1] ? kRocBadBit : 0);
  const double p = (double)counts[3 * i], n = (double)counts[3 * i + 1];
  if (st) {
    auc[i] = __longlong_as_double(0x7ff8000000000000ll);
    status[i] = (st & kRocBadBit) ? XM_ROC_BADINPUT : XM_ROC_NAN;
  } else {
    auc[i] = (p == 0.0 || n == 0.0) ? 0.0 : (double)area[i] / (p * n);
  }
}

// first maximum per sample (as max_label_kernel: NaN never wins, all -Inf is class 1), counted per workgroup in LDS and
// added to the 64-bit bins once per workgroup
__global__ void __launch_bounds__(256)
label_hist_kernel(const float *__restrict__ x, int N, int E, int sample_major, unsigned long long *__restrict__ bins) {
  extern __shared__ unsigned hbins[];
  for (int c = threadIdx.x; c < E; c += 256) hbins[c] = 0;
  __syncthreads();
  for (size_t s = blockIdx.x * (size_t)256 + threadIdx.x; s < (size_t)N; s += (size_t)gridDim.x * 256) {
    float best = -INFINITY;
    int arg = 0;
    for (int c = 0; c < E; ++c) {
      const float v = sample_major ? x[s + (size_t)N * c] : x[(size_t)E * s + c];
      if (v > best) {
        best = v;
        arg = c;
      }
    }
    atomicAdd(&hbins[arg], 1u);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < E; c += 256)
    if (hbins[c]) atomicAdd(&bins[c], (unsigned long long)hbins[c]);
}

// ---- xm_group_rows: rows grouped by wav id (fetch_emovoxceleb_imdb.m:140-148) with the radix passes above ----------
constexpr unsigned kGroupDropped = 0xFFFFFFFFu;           // the key of a row no group claims: sorts after every group

// slot[id] = 0 for every id, and the one-problem tile table the radix kernels read: set 0 = entries [0, n)
__global__ void __launch_bounds__(kRocThreads)
group_clear_kernel(int *__restrict__ slot, int slots, int n, int Tc, int *__restrict__ tile_start,
                   int *__restrict__ offsets1) {
  const size_t i = blockIdx.x * (size_t)kRocThreads + threadIdx.x;
  if (i < (size_t)slots) slot[i] = 0;
  if (i == 0) {
    tile_start[0] = 0;
    tile_start[1] = Tc;
    tile_start[2] = 0;
    offsets1[0] = 0;
    offsets1[1] = n;
  }
}

// slot[key] = group + 1
__global__ void __launch_bounds__(kRocThreads)
group_slots_kernel(const int *__restrict__ keys, int T, int key_max, int *__restrict__ slot) {
  const size_t t = blockIdx.x * (size_t)kRocThreads + threadIdx.x;
  if (t >= (size_t)T) return;
  const int k = keys[t];
  if (k > 0 && k <= key_max) slot[k] = (int)t + 1;
}

__global__ void __launch_bounds__(kRocThreads)
group_keys_kernel(const int *__restrict__ ids, int n, int key_max, const int *__restrict__ slot,
                  unsigned *__restrict__ key, unsigned *__restrict__ pos) {
  const size_t i = blockIdx.x * (size_t)kRocThreads + threadIdx.x;
  if (i >= (size_t)n) return;
  const int id = ids[i];
  const int g = (id > 0 && id <= key_max) ? slot[id] : 0;
  key[i] = g ? (unsigned)(g - 1) : kGroupDropped;
  pos[i] = (unsigned)i;
}

// offsets[t] = the number of sorted keys below t (t = 0 .. T; keys are group numbers, dropped rows sort last), rows_out =
// the sorted positions + 1 up to nnz = offsets[T] and 0 behind; key == NULL: nothing is claimed
__global__ void __launch_bounds__(kRocThreads)
group_finish_kernel(const unsigned *__restrict__ key, const unsigned *__restrict__ pos, int n, int T,
                    int *__restrict__ offsets_out, int *__restrict__ rows_out, int *__restrict__ nnz_out) {
  const size_t i = blockIdx.x * (size_t)kRocThreads + threadIdx.x;
  if (i < (size_t)n) rows_out[i] = (key && key[i] != kGroupDropped) ? (int)pos[i] + 1 : 0;
  if (i <= (size_t)T) {
    int lo = 0, hi = key ? n : 0;   // first entry with key >= i
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (key[mid] < (unsigned)i) lo = mid + 1;
      else hi = mid;
    }
    offsets_out[i] = lo;
    if (i == (size_t)T) *nnz_out = lo;
  }
}

}  // namespace xm

using namespace xm;

extern "C" {

int xm_roc_launches(void) { return 18; }

int xm_roc_geometry(int *tile, int *wave_span, int *threads, int *hist_classes_max) {
  if (tile) *tile = kTile;
  if (wave_span) *wave_span = kRocWaveSpan;
  if (threads) *threads = kRocThreads;
  if (hist_classes_max) *hist_classes_max = kHistClassesMax;
  return XM_OK;
}

int xm_roc(const float *scores, int n, int E, const int *cls, const int *offsets, const int *rows, int nnz, int G,
           double *auc, long long *area, int *counts, int *status, int *perm_out, int *tp_out, void *stream) {
  if (E < 1 || G < 0 || n < 1 || nnz < 0)
    return fail(XM_EINVAL, "roc: need n >= 1, E >= 1, G >= 0, nnz >= 0 (got n=%d E=%d G=%d nnz=%d)", n, E, G, nnz);
  if ((perm_out == nullptr) != (tp_out == nullptr))
    return fail(XM_EINVAL, "roc: perm_out and tp_out come together (both or neither)");
  if (G == 0) return XM_OK;
  if (!scores || !cls || !offsets || (nnz > 0 && !rows) || !auc || !area || !counts || !status)
    return fail(XM_EINVAL, "roc: NULL tensor");
  const long long Tc = (long long)nnz / kTile + G;   // >= the tiles of one column: sum of ceil(len_g / kTile)
  if (too_big(nnz, E) || too_big(Tc, E, 256) || too_big(3LL * E, G) || E > 65535)
    return fail(XM_ENOTSUP, "roc: supported up to nnz * E < 2^31, E <= 65535 and 3 * E * G < 2^31 (got nnz=%d E=%d G=%d)",
                nnz, E, G);
  hipStream_t st = (hipStream_t)stream;
  const size_t M = (size_t)nnz * E;
  const size_t bytes = WsCarver::need(G + 2, 4) + 4 * WsCarver::need(M, 4) + WsCarver::need((size_t)E * Tc * 256, 4) +
                       WsCarver::need((size_t)E * Tc, 4);
  WsCarver ws;
  int rc = ws.init(bytes, st);
  if (rc) return rc;
  int *tile_start = ws.take<int>(G + 2);
  unsigned *key[2] = {ws.take<unsigned>(M), ws.take<unsigned>(M)};
  unsigned *pos[2] = {ws.take<unsigned>(M), ws.take<unsigned>(M)};
  unsigned *hist = ws.take<unsigned>((size_t)E * Tc * 256);
  unsigned *tile_pos = ws.take<unsigned>((size_t)E * Tc);
  const dim3 tiles((unsigned)Tc, (unsigned)E), probs((unsigned)G, (unsigned)E), blk(kRocThreads);
  hipLaunchKernelGGL(roc_setup_kernel, dim3(1), blk, 0, st, offsets, G, E, nnz, tile_start, area, counts, status);
  hipLaunchKernelGGL(roc_keys_kernel, tiles, blk, 0, st, scores, n, E, cls, offsets, rows, nnz, G, tile_start, key[0],
                     pos[0], counts, status);
  int cur = 0;
  for (int shift = 0; shift < 32; shift += 8, cur ^= 1) {
    hipLaunchKernelGGL(roc_hist_kernel, tiles, blk, 0, st, key[cur], offsets, nnz, G, tile_start, (int)Tc, shift, hist);
    hipLaunchKernelGGL(roc_scan_kernel, probs, blk, 0, st, tile_start, (int)Tc, hist);
    hipLaunchKernelGGL(roc_scatter_kernel, tiles, blk, 0, st, key[cur], pos[cur], key[cur ^ 1], pos[cur ^ 1], offsets,
                       nnz, G, tile_start, (int)Tc, shift, hist);
  }
  hipLaunchKernelGGL(roc_tilepos_kernel, tiles, blk, 0, st, pos[cur], rows, cls, n, offsets, nnz, G, tile_start, (int)Tc,
                     tile_pos);
  hipLaunchKernelGGL(roc_scanpos_kernel, probs, blk, 0, st, tile_start, (int)Tc, tile_pos);
  hipLaunchKernelGGL(roc_curve_kernel, tiles, blk, 0, st, key[cur], pos[cur], rows, cls, n, E, offsets, nnz, G,
                     tile_start, (int)Tc, tile_pos, area, perm_out, tp_out);
  hipLaunchKernelGGL(roc_finish_kernel, dim3((E * G + 255) / 256), dim3(256), 0, st, E * G, tile_start, G, area, counts,
                     auc, status);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_label_hist(const float *x, int N, int E, int sample_major, long long *bins, void *stream) {
  if (N < 0 || E < 1) return fail(XM_EINVAL, "label_hist: need N >= 0 and E >= 1 (got N=%d E=%d)", N, E);
  if (E > kHistClassesMax) return fail(XM_ENOTSUP, "label_hist: more than %d classes", kHistClassesMax);
  if (N == 0) return XM_OK;
  if (!x || !bins) return fail(XM_EINVAL, "label_hist: NULL tensor");
  const int blocks = (int)(((size_t)N + 255) / 256 < 2048 ? ((size_t)N + 255) / 256 : 2048);
  hipLaunchKernelGGL(label_hist_kernel, dim3(blocks), dim3(256), sizeof(unsigned) * E, (hipStream_t)stream, x, N, E,
                     sample_major ? 1 : 0, (unsigned long long *)bins);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

int xm_group_rows(const int *ids, int n, const int *keys, int T, int key_max, int *offsets_out, int *rows_out,
                  int *nnz_out, void *stream) {
  if (n < 0 || T < 0 || key_max < 0)
    return fail(XM_EINVAL, "group_rows: need n >= 0, T >= 0, key_max >= 0 (got n=%d T=%d key_max=%d)", n, T, key_max);
  if ((n > 0 && (!ids || !rows_out)) || (T > 0 && !keys) || !offsets_out || !nnz_out)
    return fail(XM_EINVAL, "group_rows: NULL tensor");
  const long long Tc = ((long long)n + kTile - 1) / kTile;
  if (key_max >= (1 << 28) || too_big(Tc, 256))
    return fail(XM_ENOTSUP, "group_rows: supported up to key_max < 2^28 and n < 2^31 (got n=%d key_max=%d)", n, key_max);
  hipStream_t st = (hipStream_t)stream;
  const dim3 blk(kRocThreads);
  const size_t fin = ((size_t)(n > T + 1 ? n : T + 1) + kRocThreads - 1) / kRocThreads;
  if (n == 0 || T == 0) {
    hipLaunchKernelGGL(group_finish_kernel, dim3((unsigned)fin), blk, 0, st, (const unsigned *)nullptr,
                       (const unsigned *)nullptr, n, T, offsets_out, rows_out, nnz_out);
    XM_LAUNCH_CHECK();
    return XM_OK;
  }
  const size_t slots = (size_t)key_max + 1;
  const size_t bytes = WsCarver::need(slots, 4) + 2 * WsCarver::need(4, 4) + 4 * WsCarver::need((size_t)n, 4) +
                       WsCarver::need((size_t)Tc * 256, 4);
  WsCarver ws;
  int rc = ws.init(bytes, st);
  if (rc) return rc;
  int *slot = ws.take<int>(slots);
  int *tile_start = ws.take<int>(4);
  int *offsets1 = ws.take<int>(4);
  unsigned *key[2] = {ws.take<unsigned>(n), ws.take<unsigned>(n)};
  unsigned *pos[2] = {ws.take<unsigned>(n), ws.take<unsigned>(n)};
  unsigned *hist = ws.take<unsigned>((size_t)Tc * 256);
  const dim3 tiles((unsigned)Tc, 1), one(1, 1);
  hipLaunchKernelGGL(group_clear_kernel, dim3((unsigned)((slots + kRocThreads - 1) / kRocThreads)), blk, 0, st, slot,
                     (int)slots, n, (int)Tc, tile_start, offsets1);
  hipLaunchKernelGGL(group_slots_kernel, dim3((unsigned)(((size_t)T + kRocThreads - 1) / kRocThreads)), blk, 0, st, keys,
                     T, key_max, slot);
  hipLaunchKernelGGL(group_keys_kernel, dim3((unsigned)(((size_t)n + kRocThreads - 1) / kRocThreads)), blk, 0, st, ids, n,
                     key_max, slot, key[0], pos[0]);
  int cur = 0;
  for (int shift = 0; shift < 32; shift += 8, cur ^= 1) {
    hipLaunchKernelGGL(roc_hist_kernel, tiles, blk, 0, st, key[cur], offsets1, n, 1, tile_start, (int)Tc, shift, hist);
    hipLaunchKernelGGL(roc_scan_kernel, one, blk, 0, st, tile_start, (int)Tc, hist);
    hipLaunchKernelGGL(roc_scatter_kernel, tiles, blk, 0, st, key[cur], pos[cur], key[cur ^ 1], pos[cur ^ 1], offsets1, n,
                       1, tile_start, (int)Tc, shift, hist);
  }
  hipLaunchKernelGGL(group_finish_kernel, dim3((unsigned)fin), blk, 0, st, key[cur], pos[cur], n, T, offsets_out,
                     rows_out, nnz_out);
  XM_LAUNCH_CHECK();
  return XM_OK;
}

}  // extern "C"

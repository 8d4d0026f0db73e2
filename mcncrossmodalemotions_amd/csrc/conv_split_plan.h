// Host-side planning of the bf16x3 arm of vl_nnconv (conv_split.hip, xm_nnconv_forward_split): integer arithmetic on the
// geometry, nothing from HIP (compiles with g++ -std=c++17; tests/test_conv_split_plan_cpu.py checks it through
// xm_nnconv_split_geometry without a GPU).
//   * CAN: which calls conv_split_kernel runs at all;
//   * the launch geometry: ONE fixed tile configuration, no tuning-table entry (as xm_spec_bucket_batch);
//   * WANT: which layers of a forward-only test-mode plan are sent to it -- a pure function of the shape.
#pragma once
#include <cstddef>
#include <cstdint>

namespace xm {

// the one tile configuration of conv_split_kernel
constexpr int kSplitBP = 128;     // output pixels of a block tile (pixels are numbered across samples: a tile may cross one)
constexpr int kSplitBK = 64;      // output channels of a block tile
constexpr int kSplitBC = 32;      // reduction depth per LDS stage = two MFMA steps of 16
constexpr int kSplitStep = 16;    // reduction depth of v_mfma_f32_32x32x16_bf16
constexpr int kSplitThreads = 256;

struct SplitShape {
  int H, W, C, N, FH, FW, FC, K, sy, sx, pt, pb, pl, pr, dy, dx, flags;
};

inline int split_out_extent(int in, int stride) { return (in - 1) / stride + 1; }   // 1 x 1 filter, no padding

// Index arithmetic of the kernel: element offsets into x, y and the residual are 32-bit, so each tensor holds fewer than
// 2^31 elements (8 GiB); the block count ceil(Ho Wo N / 128) * ceil(K / 64) is one grid dimension, below 2^31 as well.
inline bool split_fits(long long elements) { return elements < (1LL << 31); }

// dilation is accepted and ignored: a 1 x 1 filter has no second tap to move
inline bool split_can(const SplitShape &s, int sigmoid_flag) {
  if (s.H < 1 || s.W < 1 || s.C < 1 || s.N < 1 || s.K < 1 || s.sy < 1 || s.sx < 1) return false;
  if (s.FH != 1 || s.FW != 1 || s.FC != s.C) return false;          // 1 x 1, no filter groups
  if (s.pt != 0 || s.pb != 0 || s.pl != 0 || s.pr != 0) return false;
  if (s.flags & sigmoid_flag) return false;
  const long long Ho = split_out_extent(s.H, s.sy), Wo = split_out_extent(s.W, s.sx);
  if (!split_fits((long long)s.H * s.W * s.C * s.N) || !split_fits(Ho * Wo * s.K * s.N)) return false;
  if (!split_fits((long long)s.C * s.K)) return false;
  const long long blocks = (Ho * Wo * s.N + kSplitBP - 1) / kSplitBP * ((s.K + kSplitBK - 1) / kSplitBK);
  return split_fits(blocks);
}

struct SplitLaunch {
  int pixel_tiles, k_tiles, blocks, launches;
};
inline SplitLaunch split_launch(const SplitShape &s) {
  const long long NP = (long long)split_out_extent(s.H, s.sy) * split_out_extent(s.W, s.sx) * s.N;
  SplitLaunch l;
  l.pixel_tiles = (int)((NP + kSplitBP - 1) / kSplitBP);
  l.k_tiles = (s.K + kSplitBK - 1) / kSplitBK;
  l.blocks = l.pixel_tiles * l.k_tiles;
  l.launches = 1;
  return l;
}

// WANT: the layers a forward-only plan sends to the split kernel.  The rule is the outcome of ONE measurement
// (tools/conv_split_bench.py): a shape is listed only where the split kernel was more than 4 % faster
// than the fp32 selection in the same call.  kSplitWantMinC == 0 means "no layer": the operator and the option ship, the
// plan keeps every layer on fp32.  That is the state today: the kernel measured 0.10 - 0.95 x the speed of the fp32 selection
// on every 1 x 1 layer of both teachers at 32 and 128 faces.  A second limit holds whatever the speed: on the real graphs only
// the last stage (7 x 7 maps, C >= 512) keeps the network inside its 1e-4 forward tolerance, so a later rule may admit those
// shapes and nothing earlier (tests/test_gpu_teacher_precision.py holds the rule to that tolerance).
constexpr int kSplitWantMinC = 0;        // reduction depth from which the split kernel was measured faster (0: nowhere)
constexpr int kSplitWantMinPixels = 0;   // ... and the least Ho Wo N
inline bool split_want(const SplitShape &s) {
  if (kSplitWantMinC <= 0) return false;
  const long long NP = (long long)split_out_extent(s.H, s.sy) * split_out_extent(s.W, s.sx) * s.N;
  return s.C >= kSplitWantMinC && NP >= kSplitWantMinPixels;
}

}  // namespace xm

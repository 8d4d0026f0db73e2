// The tile configurations of the implicit-GEMM convolution and the table of measured choices between them: host only,
// no HIP, like conv_plan.h (plain g++; tests/conv_tune_check.cpp checks the table and its file format without a GPU).
// Who measures, when, and where the default file lies is conv.hip's business; nothing here reads the environment.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "conv_plan.h"

namespace xm {

// ---- tile configuration ---------------------------------------------------------------------
struct Cfg {
  int tm, tn, wgm, wgn;
  int bm() const { return 32 * tm * wgm; }
  int bn() const { return 32 * tn * wgn; }
};
static const Cfg kCfgs[] = {
    {2, 2, 2, 2},  // 128 x 128
    {2, 2, 1, 4},  //  64 x 256
    {3, 1, 1, 4},  //  96 x 128
    {1, 2, 2, 2},  //  64 x 128
    {1, 1, 2, 2},  //  64 x  64
    {1, 1, 4, 1},  // 128 x  32
    {1, 1, 1, 4},  //  32 x 128
    // EIGHT waves per block: the 128 x 128 tile by waves of 32 x 64 -- 128 VGPRs, so two blocks per CU are four waves per
    // SIMD instead of two: +3 ... 4 % on the long-reduction forward / dgrad layers (the filter derivative is
    // 2 % slower with it, 64 x 256 by eight waves is no faster than 64 x 128 by four, 96 x 256 by waves of 96 x 32 spills,
    // 96 x 128 by six waves stages 512 gather units with 384 threads: 75 against 117 TFLOP/s)
    {1, 2, 4, 2},  //  7
    // LDS-DMA variants (conv_gemm_dma_kernel): forward / dgrad GEMMs of 1x1 unit-stride layers only; LDS stages: kDmaStages
    {2, 2, 2, 2},  //  8: 128 x 128
    {2, 2, 1, 4},  //  9:  64 x 256
    {1, 2, 2, 2},  // 10:  64 x 128
    {1, 1, 2, 2},  // 11:  64 x  64
};
constexpr int kNumCfg = sizeof(kCfgs) / sizeof(kCfgs[0]);
constexpr int kNumBaseCfg = 8;                       // configurations every forward / dgrad geometry can run
constexpr int kCfgW8 = 7;                            // the eight-wave configuration (XM_NO_W8 runs configuration 0 in its place)
constexpr int kNumWgradCfg = 7;                      // ... and the filter derivative (four-wave configurations only)
static const int kDmaBase[] = {0, 1, 3, 4};          // the register-staged configuration of the same tile shape
inline bool is_dma_cfg(int ci) { return ci >= kNumBaseCfg; }
inline int base_cfg(int ci) { return is_dma_cfg(ci) ? kDmaBase[ci - kNumBaseCfg] : ci; }
inline int wgrad_cfg(int ci) { ci = base_cfg(ci); return ci >= kNumWgradCfg ? 0 : ci; }

// ---- table keys -----------------------------------------------------------------------------
struct TuneKey {
  int kind, M, NP, Rp, mode, a, b, c, d;
  bool operator<(const TuneKey &o) const { return memcmp(this, &o, sizeof(TuneKey)) < 0; }
};
// one builder per key family (the kinds: DESIGN.md 2.0); the fields are what the shipped table was written with
inline TuneKey tune_key_forward(int kind, const Geo &g, int M, int NP, int Rp, int tmode) {
  return TuneKey{kind, M, NP, Rp, tmode, g.sy * 16 + g.sx, g.FH * 64 + g.FW, g.H, g.W};
}
inline TuneKey tune_key_class_dgrad(int kind, const Geo &g, const DgradClass &c, int M, int NP, int PI) {
  return TuneKey{kind, M, NP, c.Rp, c.nU * 64 + c.nV, g.sy * 16 + g.sx, PI, c.PJ, g.Ho};
}
inline TuneKey tune_key_merged_dgrad(int kind, const Geo &g, int M, long long npSum, int rpMax, int classes) {
  return TuneKey{kind, M, (int)std::min<long long>(npSum, 1 << 30), rpMax, classes, g.sy * 16 + g.sx, g.FH * 64 + g.FW, g.H, g.W};
}
inline TuneKey tune_key_wgrad(int kind, const Geo &g) {
  return TuneKey{kind, g.Kg, g.Ho * g.Wo * g.N, g.R, g.G, g.sy * 16 + g.sx, g.FH * 64 + g.FW, g.H, g.W};
}

// ---- persistent tuning table ------------------------------------------------------------------
// The measured choices are kept in a text file next to the library (tune_gfx950.txt, or $XM_TUNE_FILE) and
// loaded before the first lookup: tile choices -- and therefore the summation order of every convolution --
// are then the same in every process, and shapes already in the table pay no timed launches on the caller's
// stream.  Shapes that are not in the table are still measured once per process (and written back by
// xm_tune_save).  The header carries XM_TUNE_REV, bumped whenever the kernels or the configuration list change.
constexpr int XM_TUNE_REV = 7;   // 7: configuration 7 = 128 x 128 by eight waves (the LDS-DMA ones moved to 8 ... 11); 6: fused-statistics launches are their own entries (mode + 4)

struct TuneTable {
  std::map<TuneKey, int> entries;   // key -> configuration (tune_cfg) or arm (tune_challengers)
  int unsaved = 0;                  // entries recorded since the last save
  bool loaded = false;              // a file has been read, or the owner has decided that none will be

  int size() const { return (int)entries.size(); }
  const int *find(const TuneKey &k) const {
    auto it = entries.find(k);
    return it == entries.end() ? nullptr : &it->second;
  }
  void record(const TuneKey &k, int cfg) {
    entries[k] = cfg;
    ++unsaved;
  }
  // Returns the number of entries ADDED: nothing from a file whose header is not this build's, no line whose
  // configuration this build does not have, and an entry already in the table wins over the file's.
  int load(const char *path) {
    loaded = true;
    FILE *fp = fopen(path, "r");
    if (!fp) return 0;
    int ver = 0, rev = 0, ncfg = 0, n = 0;
    if (fscanf(fp, "xmodal-tune %d rev=%d cfgs=%d\n", &ver, &rev, &ncfg) == 3 && ver == 1 && rev == XM_TUNE_REV &&
        ncfg == kNumCfg) {
      TuneKey k;
      int cfg;
      while (fscanf(fp, "%d %d %d %d %d %d %d %d %d %d\n", &k.kind, &k.M, &k.NP, &k.Rp, &k.mode, &k.a, &k.b, &k.c, &k.d,
                    &cfg) == 10)
        if (cfg >= 0 && cfg < kNumCfg && !entries.count(k)) {
          entries[k] = cfg;
          ++n;
        }
    }
    fclose(fp);
    return n;
  }
  // Writes <path>.tmp and renames it over path, entries in key order.  0: done; 1: <path>.tmp cannot be written;
  // 2: the rename failed.
  int save(const char *path) {
    const std::string tmp = std::string(path) + ".tmp";
    FILE *fp = fopen(tmp.c_str(), "w");
    if (!fp) return 1;
    fprintf(fp, "xmodal-tune 1 rev=%d cfgs=%d\n", XM_TUNE_REV, kNumCfg);
    for (auto &kv : entries) {
      const TuneKey &k = kv.first;
      fprintf(fp, "%d %d %d %d %d %d %d %d %d %d\n", k.kind, k.M, k.NP, k.Rp, k.mode, k.a, k.b, k.c, k.d, kv.second);
    }
    fclose(fp);
    if (rename(tmp.c_str(), path) != 0) return 2;
    unsaved = 0;
    return 0;
  }
};

}  // namespace xm

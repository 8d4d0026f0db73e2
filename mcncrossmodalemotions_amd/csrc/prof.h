// Per-kernel timing with HIP events on the launch stream: the xm_prof_* hooks of include/xmodal_prof.h (bench.py's
// roofline leg, the route assertions of the tests).  Every translation unit wraps a launch in a ProfScope.
#pragma once
#include <hip/hip_runtime.h>

namespace xm {

// one value per launch site family; a key is prof_key(kind, sub), the sub-keys and names of every kind are the rows of
// kProfRows (prof.cpp)
enum ProfKind {
  kProfGemm = 0,            // conv.hip, sub = ci * 2 + mode
  kProfWgrad = 1,           //           sub = ci * 4 + log2(vector width)
  kProfGemmMulti = 2,       //           sub = ci * 2
  kProfHalo = 3,            //           sub = halo variant
  kProfHaloMulti = 4,
  kProfStem = 5,
  kProfStemWgrad = 6,       //           sub = 1: from the bnorm + relu + pool tensors
  kProfWgradPatch = 9,
  kProfWgradPatchS2 = 10,
  kProfDgradS2 = 11,
  kProfStem3 = 12,          //           sub = 1: 256-pixel block tiles
  kProfStemGram = 13,       // stem_pool.hip
  kProfStemWgradPool = 14,  //           sub = 1: with the pooled output
  kProfStemBnpoolFwd = 15,
  kProfSpec = 20,           // spec.hip, sub = launch of xm_spec_bucket_batch
  kProfJpeg = 21,           // jpeg.hip, sub = stage of the decode
  kProfWav = 22,            // wav.hip
  kProfPixcsv = 23,         // pixcsv.hip
  kProfLrn = 25,            // lrn.hip, sub = 2 * backward + 16-byte arm; 4 / 5: the general arm, forward / backward
  kProfJpegProg = 26,       // jpeg_prog.hip: the entropy launch of a level, the two smoothing launches
  kProfWavRate = 27,        // wav.hip, decode + resample: sub = 0 the gains, 1 the data
  kProfConvSplit = 28,      // conv_split.hip: the bf16x3 arm of 1 x 1 layers
  kProfImread = 29,         // imread_xform.hip: sub = 0 the tap tables, 1 / 2 resampling without / with Contrast, 3 its colour pass, 4 uint8 rounding
};
constexpr int prof_key(ProfKind kind, int sub = 0) { return kind * 100 + sub; }

struct ProfRec {
  hipEvent_t start, stop;
  int key;  // prof_key(kind, sub)
  double flops;
  double bytes;  // algorithmic HBM bytes of the launch: every operand once (x + f + y [+ residual])
};
extern bool g_prof_on;
void prof_begin(ProfRec &r, hipStream_t st);      // takes two events from the pool, records r.start
void prof_end(const ProfRec &r, hipStream_t st);  // records r.stop, keeps the record

// one record around the launch(es) in its scope; while the profiler is off it reads g_prof_on and does nothing else
struct ProfScope {
  const bool on;
  ProfRec r;
  hipStream_t st;
  ProfScope(int key, double flops, hipStream_t s, double bytes = 0) : on(g_prof_on), st(s) {
    if (!on) return;
    r.key = key;
    r.flops = flops;
    r.bytes = bytes;
    prof_begin(r, st);
  }
  ~ProfScope() { if (on) prof_end(r, st); }
};

// conv.hip, next to the launch switches over kCfgs (conv_tune.h): name of the instantiation behind a kProfGemm / kProfWgrad /
// kProfGemmMulti sub-key; false when no launch site produces `sub`
bool conv_cfg_kernel_name(ProfKind kind, int sub, char *buf, int len);

}  // namespace xm

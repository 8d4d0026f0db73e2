// The kernel profiler: records, event pool, key table and the C entry points of include/xmodal_prof.h.
#include "prof.h"

#include <algorithm>
#include <vector>

#include "xm_common.h"

namespace xm {

bool g_prof_on = false;
static std::vector<ProfRec> g_prof;
static std::vector<hipEvent_t> g_event_pool;

static hipEvent_t prof_event() {
  if (!g_event_pool.empty()) {
    hipEvent_t e = g_event_pool.back();
    g_event_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  (void)hipEventCreate(&e);
  return e;
}
void prof_begin(ProfRec &r, hipStream_t st) {
  r.start = prof_event();
  r.stop = prof_event();
  (void)hipEventRecord(r.start, st);
}
void prof_end(const ProfRec &r, hipStream_t st) {
  (void)hipEventRecord(r.stop, st);
  g_prof.push_back(r);
}

// ---- the key table: one row per kind, the names as rocprofv3 --kernel-trace prints them (sans namespace) ------------
struct ProfRow {
  ProfKind kind;
  int nsub;              // sub-keys are 0 .. nsub - 1
  const char *names[6];  // names[sub]; none: conv_cfg_kernel_name (conv.hip), which also refuses the holes of its numbering
};
static const ProfRow kProfRows[] = {
    {kProfGemm, 2 * 12, {}},
    {kProfWgrad, 4 * 7, {}},
    {kProfGemmMulti, 2 * 8, {}},
    {kProfHalo, 3, {"conv_halo_kernel<2, 2, 2, 2, 512>", "conv_halo_kernel<3, 1, 1, 4, 512>", "conv_halo_kernel<3, 1, 1, 4, 1024>"}},
    {kProfHaloMulti, 3, {"conv_halo_multi_kernel<2, 2, 2, 2, 512>", "conv_halo_multi_kernel<3, 1, 1, 4, 512>",
                         "conv_halo_multi_kernel<3, 1, 1, 4, 1024>"}},
    // inexact (tests assert on these strings): the stem rows name the stride-2 instantiation for stride-1 launches too
    {kProfStem, 1, {"conv_stem_kernel<2>"}},
    {kProfStemWgrad, 2, {"conv_stem_wgrad_kernel<2>", "conv_stem_wgrad_bnp_kernel<2, 2>"}},
    {kProfWgradPatch, 1, {"conv_wgrad_patch_kernel<30>"}},
    {kProfWgradPatchS2, 1, {"conv_wgrad_patch_s2_kernel<5, 2>"}},
    {kProfDgradS2, 1, {"conv_dgrad_s2_kernel<1>"}},
    {kProfStem3, 2, {"conv_stem3_kernel<1>", "conv_stem3_kernel<2>"}},
    {kProfStemGram, 1, {"stem_gram_kernel<2>"}},                                                            // inexact, as above
    {kProfStemWgradPool, 2, {"conv_stem_wgrad_pool_kernel<2, false>", "conv_stem_wgrad_pool_kernel<2, true>"}},  // inexact, as above
    {kProfStemBnpoolFwd, 1, {"conv_stem_bnpool_fwd_kernel"}},
    {kProfSpec, 4, {"spec_bank_kernel", "spec_plan_kernel", "spec_gemm_kernel", "spec_finish_kernel"}},
    // inexact (tests assert on this string): sub-key 4 is the family name, misc.hip picks the <false> / <true> instantiation
    {kProfJpeg, 6, {"jpeg_clear_kernel", "jpeg_entropy_kernel", "jpeg_idct_kernel", "jpeg_colour_kernel",
                    "crop_resize_face_ragged_kernel", "jpeg_entropy_split_kernel"}},
    {kProfJpegProg, 3, {"jpeg_entropy_prog_kernel", "jpeg_smooth_kernel", "jpeg_smooth_dc_kernel"}},
    {kProfWav, 1, {"wav_decode_kernel"}},
    {kProfWavRate, 2, {"wav_rate_gain_kernel", "wav_resample_kernel"}},
    {kProfPixcsv, 1, {"pixcsv_decode_kernel"}},
    {kProfConvSplit, 1, {"conv_split_kernel"}},
    {kProfImread, 5, {"imread_table_kernel", "imread_resample_kernel<false>", "imread_resample_kernel<true>", "imread_colour_kernel",
                     "imread_round_kernel"}},
    // inexact: the register-window rows name the N = 5 instantiation (the VGG-M family's) for every window width
    {kProfLrn, 6, {"lrn_forward_kernel<5, false>", "lrn_forward_kernel<5, true>", "lrn_backward_kernel<5, false>",
                   "lrn_backward_kernel<5, true>", "lrn_general_kernel<false>", "lrn_general_kernel<true>"}},
};

// index of `key` in the keys seen so far (appended when new): first-launch order
static size_t prof_slot(std::vector<int> &ks, int key) {
  const size_t i = std::find(ks.begin(), ks.end(), key) - ks.begin();
  if (i == ks.size()) ks.push_back(key);
  return i;
}

}  // namespace xm

using namespace xm;

extern "C" {

int xm_prof_enable(int on) {
  if (on) {
    for (auto &r : g_prof) {
      g_event_pool.push_back(r.start);
      g_event_pool.push_back(r.stop);
    }
    g_prof.clear();
  }
  g_prof_on = on != 0;
  return XM_OK;
}

// Aggregates the recorded launches by kernel instantiation.  Caller must have synchronised the
// stream(s).  Returns the number of distinct kernels; fills up to `cap` entries.
int xm_prof_collect(int cap, int *keys, double *total_ms, double *total_flops, long long *launches) {
  std::vector<int> ks;
  std::vector<double> ms, fl;
  std::vector<long long> cnt;
  for (auto &r : g_prof) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, r.start, r.stop) != hipSuccess) continue;
    const size_t i = prof_slot(ks, r.key);
    if (i == ms.size()) ms.push_back(0), fl.push_back(0), cnt.push_back(0);
    ms[i] += t;
    fl[i] += r.flops;
    cnt[i] += 1;
  }
  for (size_t i = 0; i < ks.size() && (int)i < cap; ++i) {
    keys[i] = ks[i];
    total_ms[i] = ms[i];
    total_flops[i] = fl[i];
    launches[i] = cnt[i];
  }
  return (int)ks.size();
}

// algorithmic bytes (every operand once) summed per kernel instantiation, same order / keys as xm_prof_collect
int xm_prof_collect_bytes(int cap, int *keys, double *total_bytes) {
  std::vector<int> ks;
  std::vector<double> by;
  for (auto &r : g_prof) {
    const size_t i = prof_slot(ks, r.key);
    if (i == by.size()) by.push_back(0);
    by[i] += r.bytes;
  }
  for (size_t i = 0; i < ks.size() && (int)i < cap; ++i) {
    keys[i] = ks[i];
    total_bytes[i] = by[i];
  }
  return (int)ks.size();
}

// kernel name of a key that a launch site can record; any other key is XM_EINVAL with an empty buffer
int xm_prof_kernel_name(int key, char *buf, int len) {
  if (!buf || len <= 0) return fail(XM_EINVAL, "xm_prof_kernel_name: no buffer");
  buf[0] = 0;
  const int kind = key / 100, sub = key % 100;
  for (const ProfRow &row : kProfRows) {
    if (key < 0 || kind != row.kind || sub >= row.nsub) continue;
    if (row.names[0]) {
      snprintf(buf, len, "%s", row.names[sub]);
      return XM_OK;
    }
    if (conv_cfg_kernel_name(row.kind, sub, buf, len)) return XM_OK;
  }
  return fail(XM_EINVAL, "xm_prof_kernel_name: no launch site records key %d", key);
}

}  // extern "C"

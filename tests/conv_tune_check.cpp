// Stand-alone check of csrc/conv_tune.h (no HIP, no GPU): tests/test_conv_tune_cpu.py builds and runs it.
//   conv_tune_check <shipped tune_gfx950.txt> <scratch directory>
//   1. the shipped table loads whole, once, and saves back byte for byte;
//   2. files of another format version / revision / configuration count, missing and empty files load nothing;
//   3. lines naming a configuration this build does not have are skipped, entries already in the table win;
//   4. the key builders give the keys recorded in tests/golden/conv_dispatch_digest.json.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../mcncrossmodalemotions_amd/csrc/conv_tune.h"

using namespace xm;

static long g_checked = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    ++g_checked;                                                         \
    if (!(cond)) {                                                       \
      std::printf("FAILED %s (line %d)\n", #cond, __LINE__);             \
      std::exit(1);                                                      \
    }                                                                    \
  } while (0)

static bool read_file(const std::string &path, std::string *out) {
  FILE *fp = fopen(path.c_str(), "rb");
  if (!fp) return false;
  out->clear();
  char buf[4096];
  for (size_t n; (n = fread(buf, 1, sizeof buf, fp)) > 0;) out->append(buf, n);
  fclose(fp);
  return true;
}
static void write_file(const std::string &path, const std::string &text) {
  FILE *fp = fopen(path.c_str(), "wb");
  CHECK(fp != nullptr);
  CHECK(fwrite(text.data(), 1, text.size(), fp) == text.size());
  fclose(fp);
}
static bool exists(const std::string &path) {
  FILE *fp = fopen(path.c_str(), "rb");
  if (fp) fclose(fp);
  return fp != nullptr;
}
static std::string header(int ver, int rev, int cfgs) {
  return "xmodal-tune " + std::to_string(ver) + " rev=" + std::to_string(rev) + " cfgs=" + std::to_string(cfgs) + "\n";
}
static std::string line(const TuneKey &k, int cfg) {
  char buf[256];
  snprintf(buf, sizeof buf, "%d %d %d %d %d %d %d %d %d %d\n", k.kind, k.M, k.NP, k.Rp, k.mode, k.a, k.b, k.c, k.d, cfg);
  return buf;
}
static bool same(const TuneKey &k, int kind, int M, int NP, int Rp, int mode, int a, int b, int c, int d) {
  const TuneKey o{kind, M, NP, Rp, mode, a, b, c, d};
  return memcmp(&k, &o, sizeof k) == 0;
}

// the geometry as the library's make_geo derives it
static Geo geo(int H, int W, int C, int N, int FH, int FW, int FC, int K, int sy, int sx, int pt, int pb, int pl, int pr) {
  const int th = H + pt + pb - FH, tw = W + pl + pr - FW;
  return Geo{H, W, C, N, FH, FW, FC, K, C / FC, K / (C / FC), th / sy + 1, tw / sx + 1, FH * FW * FC, sy, sx, pt, pb, pl, pr, 1, 1};
}

int main(int argc, char **argv) {
  if (argc != 3) {
    std::printf("usage: conv_tune_check <tune_gfx950.txt> <scratch directory>\n");
    return 2;
  }
  const std::string shipped = argv[1], dir = std::string(argv[2]) + "/";

  // ---- 1. the shipped table ------------------------------------------------------------------------------------------
  std::string text;
  CHECK(read_file(shipped, &text));
  CHECK(!text.empty() && text.back() == '\n');
  int lines = 0;
  for (char ch : text) lines += ch == '\n';
  TuneTable t;
  CHECK(t.size() == 0 && t.unsaved == 0 && !t.loaded);
  const int added = t.load(shipped.c_str());
  CHECK(added == lines - 1);
  CHECK(t.size() == added && t.unsaved == 0 && t.loaded);
  CHECK(t.load(shipped.c_str()) == 0);
  CHECK(t.size() == added);
  for (auto &kv : t.entries) {
    CHECK(kv.second >= 0 && kv.second < kNumCfg);
    const int *hit = t.find(kv.first);
    CHECK(hit && *hit == kv.second);
  }
  const std::string copy = dir + "copy.txt";
  CHECK(t.save(copy.c_str()) == 0);
  std::string back;
  CHECK(read_file(copy, &back));
  CHECK(back == text);                       // byte for byte: header, key order, line format
  CHECK(t.unsaved == 0 && !exists(copy + ".tmp"));

  // record counts what a save has not seen yet; a save into a directory that does not exist reports it and keeps the count
  const TuneKey fresh{99, 1, 2, 3, 4, 5, 6, 7, 8};
  CHECK(t.find(fresh) == nullptr);
  t.record(fresh, 3);
  CHECK(t.unsaved == 1 && t.size() == added + 1 && *t.find(fresh) == 3);
  CHECK(t.save((dir + "no_such_directory/x.txt").c_str()) == 1);
  CHECK(t.unsaved == 1);
  CHECK(t.save(copy.c_str()) == 0);
  CHECK(t.unsaved == 0 && !exists(copy + ".tmp"));
  TuneTable t2;
  CHECK(t2.load(copy.c_str()) == added + 1 && *t2.find(fresh) == 3);

  // ---- 2. files that load nothing --------------------------------------------------------------------------------------
  const TuneKey ka{0, 32, 360, 144, 1, 17, 195, 12, 10}, kb{1, 16, 360, 288, 195, 17, 12, 10, 12};
  const TuneKey kc{2, 32, 360, 144, 1, 17, 195, 12, 10}, kd{3, 8, 131072, 80, 4, 34, 325, 64, 64};
  const std::string f = dir + "case.txt";
  const std::string bad[] = {header(2, XM_TUNE_REV, kNumCfg), header(1, XM_TUNE_REV + 1, kNumCfg),
                             header(1, XM_TUNE_REV - 1, kNumCfg), header(1, XM_TUNE_REV, kNumCfg + 1),
                             header(1, XM_TUNE_REV, kNumCfg - 1), std::string()};
  for (const std::string &h : bad) {
    write_file(f, h.empty() ? h : h + line(ka, 1) + line(kb, 2));
    TuneTable e;
    CHECK(e.load(f.c_str()) == 0);
    CHECK(e.size() == 0 && e.unsaved == 0 && e.loaded);
  }
  {
    TuneTable e;
    CHECK(!exists(dir + "missing.txt"));
    CHECK(e.load((dir + "missing.txt").c_str()) == 0);
    CHECK(e.size() == 0 && e.loaded);
  }

  // ---- 3. line handling --------------------------------------------------------------------------------------------------
  write_file(f, header(1, XM_TUNE_REV, kNumCfg) + line(ka, 3) + line(kb, -1) + line(kc, kNumCfg) + line(kd, kNumCfg - 1));
  {
    TuneTable e;
    CHECK(e.load(f.c_str()) == 2);
    CHECK(e.size() == 2 && e.unsaved == 0);
    CHECK(e.find(ka) && *e.find(ka) == 3);
    CHECK(e.find(kb) == nullptr && e.find(kc) == nullptr);
    CHECK(e.find(kd) && *e.find(kd) == kNumCfg - 1);
  }
  {
    TuneTable e;
    e.record(ka, 5);
    CHECK(e.load(f.c_str()) == 1);           // kd alone is new
    CHECK(*e.find(ka) == 5 && *e.find(kd) == kNumCfg - 1);
    CHECK(e.size() == 2 && e.unsaved == 1);
    CHECK(e.save(f.c_str()) == 0);           // key order: kind first
    CHECK(read_file(f, &back));
    CHECK(back == header(1, XM_TUNE_REV, kNumCfg) + line(ka, 5) + line(kd, kNumCfg - 1));
  }

  // ---- 4. key builders (geometries and keys of tests/golden/conv_dispatch_digest.json) -----------------------------------
  {
    const Geo g = geo(12, 10, 16, 3, 3, 3, 16, 32, 1, 1, 1, 1, 1, 1);            // 3 x 3, pad 1
    const int NP = g.Ho * g.Wo * g.N, Rp = (g.R + kBK - 1) / kBK * kBK;
    CHECK(same(tune_key_forward(0, g, g.Kg, NP, Rp, 1), 0, 32, 360, 144, 1, 17, 195, 12, 10));
    CHECK(same(tune_key_forward(4, g, g.Kg, NP, Rp, 1), 4, 32, 360, 144, 1, 17, 195, 12, 10));
    CHECK(same(tune_key_wgrad(2, g), 2, 32, 360, 144, 1, 17, 195, 12, 10));
    bool all;
    const std::vector<DgradClass> cls = dgrad_classes(g, dgrad_fold_h(g), &all);
    CHECK(cls.size() == 1 && all);
    const DgradClass &c = cls[0];
    CHECK(same(tune_key_class_dgrad(1, g, c, g.FC, c.PI * c.PJ * g.N, c.PI), 1, 16, 360, 288, 195, 17, 12, 10, 12));
  }
  {
    const Geo g = geo(512, 60, 1, 10, 7, 7, 1, 96, 2, 2, 1, 1, 1, 1);            // the single-channel stem, stride 2
    const int NP = g.Ho * g.Wo * g.N, Rp = (g.R + kBK - 1) / kBK * kBK;
    CHECK(same(tune_key_forward(0, g, g.Kg, NP, Rp, 1), 0, 96, 71120, 64, 1, 34, 455, 512, 60));
    CHECK(same(tune_key_wgrad(2, g), 2, 96, 71120, 49, 1, 34, 455, 512, 60));
    CHECK(same(tune_key_wgrad(8, g), 8, 96, 71120, 49, 1, 34, 455, 512, 60));
  }
  {
    const Geo g = geo(64, 64, 8, 32, 5, 5, 8, 8, 2, 2, 2, 2, 2, 2);              // 5 x 5 / stride 2: four classes, one launch
    bool all;
    const std::vector<DgradClass> cls = dgrad_classes(g, dgrad_fold_h(g), &all);
    long long npSum = 0;
    int rpMax = 0;
    for (const DgradClass &c : cls) npSum += (long long)c.PI * c.PJ * g.N, rpMax = std::max(rpMax, c.Rp);
    CHECK(same(tune_key_merged_dgrad(3, g, g.FC, npSum, rpMax, (int)cls.size()), 3, 8, 131072, 80, 4, 34, 325, 64, 64));
    CHECK(same(tune_key_merged_dgrad(3, g, g.FC, 1LL << 40, rpMax, 4), 3, 8, 1 << 30, 80, 4, 34, 325, 64, 64));   // clamped
  }
  // the order of a saved file is memcmp's on the nine integers
  CHECK(ka < kb && kb < kc && kc < kd && !(kd < ka) && !(ka < ka));

  std::printf("%ld checks, %d entries in the shipped table\n", g_checked, added);
  return 0;
}

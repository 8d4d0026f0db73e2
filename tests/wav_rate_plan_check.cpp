// Stand-alone check of the rate-aware plan in csrc/wav_plan.h (wav_plan_batch_fs; no HIP, no GPU):
// tests/test_wav_rate_cpu.py builds it with the address and undefined-behaviour sanitizers and runs it.  For a file of
// every format at each of several rates it plans, towards several target rates,
//   1. every truncation of the file,
//   2. every third value of every one of its first 48 bytes (the whole header, the rate field in it),
// alone and as the middle file of a batch of three, in exactly sized heap blocks so that a read past a file is caught.
// The code must be a documented one; on success p / q is fs / SampleRate in lowest terms and inside the plan's bounds,
// the offsets advance by ceil(frames p / q) per channel written and `sizes` is consistent.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../mcncrossmodalemotions_amd/csrc/wav_plan.h"

using namespace xm;
typedef std::vector<unsigned char> Bytes;

static long g_checked = 0, g_ok = 0, g_notsup = 0;
static char g_what[160];
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) {                                                               \
      std::printf("FAILED %s (line %d): %s\n", #cond, __LINE__, g_what);         \
      std::exit(1);                                                              \
    }                                                                            \
  } while (0)

static void put16(Bytes &b, unsigned v) { b.push_back(v & 255); b.push_back((v >> 8) & 255); }
static void put32(Bytes &b, unsigned v) { put16(b, v & 0xFFFF); put16(b, v >> 16); }
static void puts4(Bytes &b, const char *t) { b.insert(b.end(), t, t + 4); }

static Bytes make_file(int tag, int nch, int bits, int frames, unsigned rate) {
  Bytes b;
  puts4(b, "RIFF");
  put32(b, 0);
  puts4(b, "WAVE");
  puts4(b, "fmt ");
  const int align = nch * bits / 8;
  put32(b, 16);
  put16(b, tag);
  put16(b, nch);
  put32(b, rate);
  put32(b, rate * align);
  put16(b, align);
  put16(b, bits);
  puts4(b, "data");
  put32(b, frames * align);
  for (int k = 0; k < frames * align; ++k) b.push_back((unsigned char)(k * 37 + 11));
  const unsigned riff = (unsigned)b.size() - 8;
  for (int k = 0; k < 4; ++k) b[4 + k] = (riff >> (8 * k)) & 255;
  return b;
}

static long long gcd(long long a, long long b) {
  while (b) {
    const long long t = a % b;
    a = b;
    b = t;
  }
  return a;
}

static int plan_and_check(const std::vector<Bytes> &files, const long long *ranges, int channel, long long fs, long long out_base) {
  const int N = (int)files.size();
  size_t total = 0;
  for (const Bytes &f : files) total += f.size();
  unsigned char *blob = (unsigned char *)std::malloc(total ? total : 1);
  long long *offsets = (long long *)std::malloc(sizeof(long long) * (N + 1));
  long long *desc = (long long *)std::malloc(sizeof(long long) * XM_WAV_DESC * (N ? N : 1));
  long long *plain = (long long *)std::malloc(sizeof(long long) * XM_WAV_DESC * (N ? N : 1));
  long long sizes[XM_WAV_SIZES] = {-1, -1}, psizes[XM_WAV_SIZES] = {-1, -1};
  size_t o = 0;
  for (int i = 0; i < N; ++i) {
    offsets[i] = (long long)o;
    if (!files[i].empty()) std::memcpy(blob + o, files[i].data(), files[i].size());
    o += files[i].size();
  }
  offsets[N] = (long long)o;
  char err[256], perr[256];
  err[0] = perr[0] = 0;
  const int rc = wav_plan_batch_fs(blob, offsets, N, ranges, channel, fs, out_base, desc, sizes, err, (int)sizeof err);
  const int prc = wav_plan_batch(blob, offsets, N, ranges, channel, out_base, plain, psizes, perr, (int)sizeof perr);
  ++g_checked;
  CHECK(rc == XM_OK || rc == XM_EINVAL || rc == XM_ENOTSUP);
  if (fs < 1) {
    CHECK(rc == XM_EINVAL && std::strstr(err, "fs") != nullptr);
  } else if (prc != XM_OK) {
    CHECK(rc == prc && std::strcmp(err, perr) == 0);                   // the same refusals, word for word
  }
  if (fs < 1) {
  } else if (rc != XM_OK) {
    CHECK(std::strstr(err, "file ") != nullptr);
    if (prc == XM_OK) {   // only the ratio can refuse a file the plain plan takes
      CHECK(rc == XM_ENOTSUP && std::strstr(err, " Hz to ") != nullptr);
      ++g_notsup;
    }
  } else {
    ++g_ok;
    long long out = out_base;
    for (int i = 0; i < N; ++i) {
      const long long *d = desc + (long long)i * XM_WAV_DESC, *e = plain + (long long)i * XM_WAV_DESC;
      for (int k = 0; k < XM_WAV_DESC; ++k)
        if (k != WD_OUT && k != WD_P && k != WD_Q) CHECK(d[k] == e[k]);
      CHECK(e[WD_P] == 0 && e[WD_Q] == 0);
      const long long p = d[WD_P], q = d[WD_Q];
      CHECK(p >= 1 && q >= 1 && gcd(p, q) == 1 && p * d[WD_RATE] == q * fs);
      CHECK(p <= kWavPlanMaxRatio && q <= kWavPlanMaxRatio && q <= kWavPlanMaxStep * p && p <= kWavPlanMaxStep * q);
      CHECK(d[WD_FIRST] >= 0 && d[WD_FRAMES] >= 0 && d[WD_FIRST] + d[WD_FRAMES] <= d[WD_TOTAL]);
      CHECK(d[WD_OUT] == out);
      const long long rows = (d[WD_FRAMES] * p + q - 1) / q;
      CHECK(rows * q >= d[WD_FRAMES] * p && (rows - 1) * q < d[WD_FRAMES] * p + (d[WD_FRAMES] == 0 ? q : 0));
      if (d[WD_RATE] == fs) CHECK(p == 1 && q == 1 && rows == d[WD_FRAMES]);
      out += rows * d[WD_CW];
    }
    CHECK(sizes[0] == out - out_base && sizes[1] == N);
  }
  std::free(blob);
  std::free(offsets);
  std::free(desc);
  std::free(plain);
  return rc;
}

int main() {
  static const int kinds[6][2] = {{1, 8}, {1, 16}, {1, 24}, {1, 32}, {3, 32}, {3, 64}};
  static const unsigned rates[5] = {48000, 44100, 11025, 16000, 192000};
  static const long long targets[3] = {16000, 22050, 8000};
  for (int k = 0; k < 6; ++k)
    for (int ri = 0; ri < 5; ++ri)
      for (int nch = 1; nch <= 3; nch += 2) {
        const Bytes good = make_file(kinds[k][0], nch, kinds[k][1], 7, rates[ri]);
        const Bytes other = make_file(1, 1, 16, 3, 32000);
        for (int ti = 0; ti < 3; ++ti) {
          const long long fs = targets[ti];
          std::snprintf(g_what, sizeof g_what, "tag %d, %d bits, %d channels, %u Hz to %lld Hz", kinds[k][0], kinds[k][1], nch, rates[ri], fs);
          const bool steep = rates[ri] > 16 * fs;   // 192000 -> 8000 is 1 / 24
          CHECK(plan_and_check({good}, nullptr, -1, fs, 0) == (steep ? XM_ENOTSUP : XM_OK));
          CHECK(plan_and_check({other, good, other}, nullptr, 0, fs, 9) == (steep ? XM_ENOTSUP : XM_OK));
          const long long whole[2] = {1, -1}, inner[2] = {2, 6}, past[2] = {2, 8};
          CHECK(plan_and_check({good}, whole, -1, fs, 0) == (steep ? XM_ENOTSUP : XM_OK));
          CHECK(plan_and_check({good}, inner, nch - 1, fs, 3) == (steep ? XM_ENOTSUP : XM_OK));
          CHECK(plan_and_check({good}, past, -1, fs, 0) == XM_EINVAL && plan_and_check({good}, nullptr, nch, fs, 0) == XM_EINVAL);
          CHECK(plan_and_check({good}, nullptr, -1, 0, 0) == XM_EINVAL && plan_and_check({good}, nullptr, -1, -16000, 0) == XM_EINVAL);
          if (ti && k != 1) continue;                                               // the sweeps: every format to 16 kHz, PCM16 to all
          for (size_t cut = 0; cut < good.size(); ++cut) {                          // 1. truncations
            std::snprintf(g_what, sizeof g_what, "tag %d, %d bits, %d channels, %u Hz to %lld Hz, cut at %zu", kinds[k][0], kinds[k][1],
                          nch, rates[ri], fs, cut);
            const Bytes f(good.begin(), good.begin() + (long)cut);
            plan_and_check({f}, nullptr, -1, fs, 0);
            plan_and_check({other, f, other}, nullptr, 0, fs, 5);
          }
          for (size_t at = 0; at < 48 && at < good.size(); ++at)                    // 2. mutations
            for (int v = 0; v < 256; v += (nch > 1 || ti) ? 7 : 3) {
              if (v == good[at]) continue;
              std::snprintf(g_what, sizeof g_what, "tag %d, %d bits, %d channels, %u Hz to %lld Hz, byte %zu = %d", kinds[k][0],
                            kinds[k][1], nch, rates[ri], fs, at, v);
              Bytes f = good;
              f[at] = (unsigned char)v;
              plan_and_check({f}, nullptr, -1, fs, 0);
              if (v % 16 == 0) plan_and_check({other, f, other}, nullptr, 0, fs, 5);
            }
        }
      }
  // the edges of the ratio's bounds
  std::snprintf(g_what, sizeof g_what, "ratio bounds");
  CHECK(plan_and_check({make_file(1, 1, 16, 5, 256000)}, nullptr, -1, 16000, 0) == XM_OK);        // 1 / 16
  CHECK(plan_and_check({make_file(1, 1, 16, 5, 272000)}, nullptr, -1, 16000, 0) == XM_ENOTSUP);   // 1 / 17
  CHECK(plan_and_check({make_file(1, 1, 16, 5, 1000)}, nullptr, -1, 16000, 0) == XM_OK);          // 16 / 1
  CHECK(plan_and_check({make_file(1, 1, 16, 5, 1000)}, nullptr, -1, 17000, 0) == XM_ENOTSUP);     // 17 / 1
  CHECK(plan_and_check({make_file(1, 1, 16, 5, 1048577)}, nullptr, -1, 1048576, 0) == XM_ENOTSUP);   // q = 2^20 + 1
  CHECK(plan_and_check({make_file(1, 1, 16, 5, 1048575)}, nullptr, -1, 1048576, 0) == XM_OK);        // 2^20 / (2^20 - 1)
  CHECK(plan_and_check({make_file(1, 1, 16, 5, 4294967295u)}, nullptr, -1, 4611686018427387904LL, 0) == XM_ENOTSUP);
  std::printf("%ld plans checked, %ld of them accepted, %ld refused for their ratio alone\n", g_checked, g_ok, g_notsup);
  return 0;
}

// Stand-alone check of csrc/wav_plan.h (no HIP, no GPU): tests/test_wav_read_cpu.py builds it with the address and
// undefined-behaviour sanitizers and runs it.  For every format it writes a valid file (plain and extensible, with a
// LIST chunk in front of the data), then plans
//   1. every truncation of the file,
//   2. every value of every one of its first 128 bytes,
// alone and as the middle file of a batch of three, in exactly sized heap blocks so that a read past a file is caught.
// The code must be a documented one; on success the byte range lies inside the file, frames x block align fits the
// range, offsets are monotone and `sizes` is consistent.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../mcncrossmodalemotions_amd/csrc/wav_plan.h"

using namespace xm;
typedef std::vector<unsigned char> Bytes;

static long g_checked = 0, g_ok = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) {                                                               \
      std::printf("FAILED %s (line %d): %s\n", #cond, __LINE__, g_what);         \
      std::exit(1);                                                              \
    }                                                                            \
  } while (0)
static char g_what[128];

static void put16(Bytes &b, unsigned v) { b.push_back(v & 255); b.push_back((v >> 8) & 255); }
static void put32(Bytes &b, unsigned v) { put16(b, v & 0xFFFF); put16(b, v >> 16); }
static void puts4(Bytes &b, const char *t) { b.insert(b.end(), t, t + 4); }

static Bytes make_file(int tag, int nch, int bits, int frames, bool extensible) {
  Bytes b;
  puts4(b, "RIFF");
  put32(b, 0);
  puts4(b, "WAVE");
  puts4(b, "fmt ");
  const int align = nch * bits / 8;
  put32(b, extensible ? 40 : 16);
  put16(b, extensible ? 0xFFFE : tag);
  put16(b, nch);
  put32(b, 16000);
  put32(b, 16000 * align);
  put16(b, align);
  put16(b, bits);
  if (extensible) {
    put16(b, 22);
    put16(b, bits);
    put32(b, 0);
    put16(b, tag);
    static const unsigned char tail[14] = {0, 0, 0, 0, 0x10, 0, 0x80, 0, 0, 0xAA, 0, 0x38, 0x9B, 0x71};
    b.insert(b.end(), tail, tail + 14);
  }
  puts4(b, "LIST");
  put32(b, 5);
  for (int k = 0; k < 6; ++k) b.push_back('a' + k);   // five bytes and the pad byte
  puts4(b, "data");
  put32(b, frames * align);
  for (int k = 0; k < frames * align; ++k) b.push_back((unsigned char)(k * 37 + 11));
  const unsigned riff = (unsigned)b.size() - 8;
  for (int k = 0; k < 4; ++k) b[4 + k] = (riff >> (8 * k)) & 255;
  return b;
}

// plans `files` from heap blocks of exactly the needed sizes and checks what comes back
static int plan_and_check(const std::vector<Bytes> &files, const long long *ranges, int channel, long long out_base) {
  const int N = (int)files.size();
  size_t total = 0;
  for (const Bytes &f : files) total += f.size();
  unsigned char *blob = (unsigned char *)std::malloc(total ? total : 1);
  long long *offsets = (long long *)std::malloc(sizeof(long long) * (N + 1));
  long long *desc = (long long *)std::malloc(sizeof(long long) * XM_WAV_DESC * (N ? N : 1));
  long long sizes[XM_WAV_SIZES] = {-1, -1};
  size_t o = 0;
  for (int i = 0; i < N; ++i) {
    offsets[i] = (long long)o;
    if (!files[i].empty()) std::memcpy(blob + o, files[i].data(), files[i].size());
    o += files[i].size();
  }
  offsets[N] = (long long)o;
  char err[256];
  err[0] = 0;
  const int rc = wav_plan_batch(blob, offsets, N, ranges, channel, out_base, desc, sizes, err, (int)sizeof err);
  ++g_checked;
  CHECK(rc == XM_OK || rc == XM_EINVAL || rc == XM_ENOTSUP);
  if (rc != XM_OK) {
    CHECK(std::strstr(err, "file ") != nullptr);
  } else {
    ++g_ok;
    long long out = out_base;
    for (int i = 0; i < N; ++i) {
      const long long *d = desc + (long long)i * XM_WAV_DESC;
      CHECK(d[WD_BEGIN] >= offsets[i] && d[WD_BEGIN] <= d[WD_END] && d[WD_END] <= offsets[i + 1]);
      CHECK(d[WD_NCH] >= 1 && d[WD_NCH] <= 64 && d[WD_RATE] >= 1);
      CHECK(d[WD_FMT] >= XM_WAV_U8 && d[WD_FMT] <= XM_WAV_F64);
      CHECK(d[WD_ALIGN] == d[WD_NCH] * d[WD_BITS] / 8 && d[WD_ALIGN] >= 1);
      CHECK(d[WD_TOTAL] >= 0 && d[WD_TOTAL] * d[WD_ALIGN] <= d[WD_END] - d[WD_BEGIN]);
      CHECK(d[WD_END] - d[WD_BEGIN] - d[WD_TOTAL] * d[WD_ALIGN] < d[WD_ALIGN]);
      CHECK(d[WD_FIRST] >= 0 && d[WD_FRAMES] >= 0 && d[WD_FIRST] + d[WD_FRAMES] <= d[WD_TOTAL]);
      CHECK(d[WD_SEL] == channel && d[WD_SEL] < d[WD_NCH] && d[WD_CW] == (channel >= 0 ? 1 : d[WD_NCH]));
      CHECK(d[WD_OUT] == out);
      CHECK(d[WD_STATUS] == XM_WAV_OK || d[WD_STATUS] == XM_WAV_TRUNCATED);
      out += d[WD_FRAMES] * d[WD_CW];
    }
    CHECK(sizes[0] == out - out_base && sizes[1] == N);
  }
  std::free(blob);
  std::free(offsets);
  std::free(desc);
  return rc;
}

int main() {
  static const int kinds[6][2] = {{1, 8}, {1, 16}, {1, 24}, {1, 32}, {3, 32}, {3, 64}};
  for (int k = 0; k < 6; ++k)
    for (int ext = 0; ext < 2; ++ext)
      for (int nch = 1; nch <= 3; nch += 2) {
        const Bytes good = make_file(kinds[k][0], nch, kinds[k][1], 7, ext != 0);
        const Bytes other = make_file(1, 1, 16, 3, false);
        std::snprintf(g_what, sizeof g_what, "tag %d, %d bits, %d channels, extensible %d", kinds[k][0], kinds[k][1], nch, ext);
        CHECK(plan_and_check({good}, nullptr, -1, 0) == XM_OK);
        CHECK(plan_and_check({other, good, other}, nullptr, 0, 9) == XM_OK && plan_and_check({good}, nullptr, nch - 1, 9) == XM_OK);
        const long long whole[2] = {1, -1}, inner[2] = {2, 6}, past[2] = {2, 8}, back[2] = {5, 4};
        CHECK(plan_and_check({good}, whole, -1, 0) == XM_OK && plan_and_check({good}, inner, 0, 3) == XM_OK);
        CHECK(plan_and_check({good}, past, -1, 0) == XM_EINVAL && plan_and_check({good}, back, -1, 0) == XM_EINVAL);
        CHECK(plan_and_check({good}, nullptr, nch, 0) == XM_EINVAL);
        for (size_t cut = 0; cut < good.size(); ++cut) {                          // 1. truncations
          std::snprintf(g_what, sizeof g_what, "tag %d, %d bits, %d channels, extensible %d, cut at %zu", kinds[k][0],
                        kinds[k][1], nch, ext, cut);
          const Bytes f(good.begin(), good.begin() + (long)cut);
          plan_and_check({f}, nullptr, -1, 0);
          plan_and_check({other, f, other}, nullptr, 0, 5);
        }
        for (size_t at = 0; at < 128 && at < good.size(); ++at)                   // 2. mutations
          for (int v = 0; v < 256; v += (ext || nch > 1) ? 5 : 1) {
            if (v == good[at]) continue;
            std::snprintf(g_what, sizeof g_what, "tag %d, %d bits, %d channels, extensible %d, byte %zu = %d", kinds[k][0],
                          kinds[k][1], nch, ext, at, v);
            Bytes f = good;
            f[at] = (unsigned char)v;
            plan_and_check({f}, nullptr, -1, 0);
            if (v % 16 == 0) plan_and_check({other, f, other}, nullptr, 0, 5);
          }
      }
  std::printf("%ld plans checked, %ld of them accepted\n", g_checked, g_ok);
  return 0;
}

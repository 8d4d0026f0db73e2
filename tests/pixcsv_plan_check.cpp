// Stand-alone check of csrc/pixcsv_plan.h (no HIP, no GPU): tests/test_pixcsv_cpu.py builds it with the address and
// undefined-behaviour sanitizers and runs it.  It writes small valid files (with and without a header, quoted fields,
// CRLF, a byte order mark, blank lines, no final newline, reordered columns), then plans
//   1. every truncation of each file,
//   2. every value of every one of its bytes,
// from heap blocks of exactly the file's size, so that a read past the end is caught; once counting only, once into a
// descriptor block of exactly the counted size, once into a block one row short.  The code must be a documented one and
// an error must name its line; on success every pixel range lies inside the file and holds no line end, line numbers
// ascend, the indices are the ordinals and `sizes` agrees with the rows.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../mcncrossmodalemotions_amd/csrc/pixcsv_plan.h"

using namespace xm;

static long g_checked = 0, g_ok = 0;
static char g_what[160];
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) {                                                               \
      std::printf("FAILED %s (line %d): %s\n", #cond, __LINE__, g_what);         \
      std::exit(1);                                                              \
    }                                                                            \
  } while (0)

static int plan_and_check(const std::string &file) {
  const long long n = (long long)file.size();
  unsigned char *blob = (unsigned char *)std::malloc(file.size() ? file.size() : 1);
  if (n) std::memcpy(blob, file.data(), file.size());
  char err[256];
  err[0] = 0;
  long long sizes[XM_PIX_SIZES] = {-1, -1};
  const int rc = pixcsv_plan(n ? blob : nullptr, n, nullptr, 0, sizes, err, (int)sizeof err);
  ++g_checked;
  CHECK(rc == XM_OK || rc == XM_EINVAL);
  if (rc != XM_OK) {
    CHECK(std::strstr(err, "line ") != nullptr);
    CHECK(sizes[0] == 0 && sizes[1] == 0);
  } else {
    ++g_ok;
    const long long N = sizes[0];
    CHECK(N >= 0 && sizes[1] >= 0 && sizes[1] <= n);
    long long *desc = (long long *)std::malloc(sizeof(long long) * XM_PIX_DESC * (N ? N : 1));
    long long again[XM_PIX_SIZES] = {-1, -1};
    CHECK(pixcsv_plan(blob, n, desc, N, again, err, (int)sizeof err) == XM_OK);
    CHECK(again[0] == N && again[1] == sizes[1]);
    long long longest = 0, line = 0;
    for (long long i = 0; i < N; ++i) {
      const long long *d = desc + i * XM_PIX_DESC;
      CHECK(d[PD_BEGIN] >= 0 && d[PD_BEGIN] <= d[PD_END] && d[PD_END] <= n);
      for (long long p = d[PD_BEGIN]; p < d[PD_END]; ++p) CHECK(blob[p] != '\n');
      CHECK(d[PD_EMOTION] >= -1 && d[PD_EMOTION] <= 999999999);
      CHECK(d[PD_USAGE] >= -1 && d[PD_USAGE] <= 2);
      CHECK(d[PD_LINE] > line);
      line = d[PD_LINE];
      CHECK(d[PD_OUT] == i && d[6] == 0 && d[7] == 0);
      if (d[PD_END] - d[PD_BEGIN] > longest) longest = d[PD_END] - d[PD_BEGIN];
    }
    CHECK(longest == sizes[1]);
    if (N > 0) {   // one row short: refused with the line of the row that does not fit, nothing written past the block
      long long *small = (long long *)std::malloc(sizeof(long long) * XM_PIX_DESC * (N > 1 ? N - 1 : 1));
      CHECK(pixcsv_plan(blob, n, small, N - 1, again, err, (int)sizeof err) == XM_EINVAL);
      CHECK(std::strstr(err, "max_rows") != nullptr && std::strstr(err, "line ") != nullptr);
      std::free(small);
    }
    std::free(desc);
  }
  std::free(blob);
  return rc;
}

int main() {
  const std::vector<std::string> files = {
      "emotion,pixels,Usage\n0,70 80 82,Training\n3,\"1 22 133\",PublicTest\n6,5,PrivateTest\n",
      "\xEF\xBB\xBF" "Usage, pixels ,emotion\r\nTraining,\"0 1\",2\r\n\r\nOther,255 254 253 252,\r\n",
      "1,10 20 30,Training\n\n2,\"40 50\",PublicTest\n7,60,PrivateTest",
      "pixels\n1 2 3\n\"4 5 6\"\n",
      "\"emotion\",\"pixels\",\"Usage\",extra\n4,9 9,Training,\"a,b\"\n",
  };
  for (size_t k = 0; k < files.size(); ++k) {
    const std::string &good = files[k];
    std::snprintf(g_what, sizeof g_what, "file %zu", k);
    CHECK(plan_and_check(good) == XM_OK);
    for (size_t cut = 0; cut < good.size(); ++cut) {                               // 1. truncations
      std::snprintf(g_what, sizeof g_what, "file %zu cut at %zu", k, cut);
      plan_and_check(good.substr(0, cut));
    }
    for (size_t at = 0; at < good.size(); ++at)                                    // 2. mutations
      for (int v = 0; v < 256; ++v) {
        if ((unsigned char)good[at] == v) continue;
        std::snprintf(g_what, sizeof g_what, "file %zu byte %zu = %d", k, at, v);
        std::string f = good;
        f[at] = (char)v;
        plan_and_check(f);
      }
  }
  // the documented rejections
  std::snprintf(g_what, sizeof g_what, "rejections");
  CHECK(plan_and_check("emotion,pixels\n1,\"2 3\n") == XM_EINVAL);
  CHECK(plan_and_check("emotion,Usage\n1,Training\n") == XM_EINVAL);
  CHECK(plan_and_check("emotion,pixels,Usage\n1,2 3\n") == XM_EINVAL);
  CHECK(plan_and_check("1,2 3\n") == XM_EINVAL);
  std::printf("%ld plans checked, %ld of them accepted\n", g_checked, g_ok);
  return 0;
}

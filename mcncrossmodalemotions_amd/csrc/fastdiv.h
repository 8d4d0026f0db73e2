// Magic division of a 31-bit numerator by a runtime divisor: q = (n * m) >> s.  Nothing from HIP: the planning headers
// (stem_pool_plan.h) and their CPU checks use it as the kernels do.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define XM_HD __host__ __device__ __forceinline__
#else
#define XM_HD inline
#endif

namespace xm {

struct FastDiv {
  uint32_t m;
  uint32_t s;
  uint32_t d;
};
static inline FastDiv make_fastdiv(uint32_t d) {
  FastDiv f;
  f.d = d;
  uint32_t l = 0;
  while ((1ull << l) < d) ++l;
  f.s = 31 + l;
  f.m = (uint32_t)(((1ull << f.s) + d - 1) / d);
  return f;
}
XM_HD uint32_t fast_div(uint32_t n, const FastDiv f) { return (uint32_t)(((uint64_t)n * f.m) >> f.s); }

}  // namespace xm

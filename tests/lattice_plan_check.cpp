// csrc/conv_plan.h, the lattice helpers of xm_nnconv_forward_lattice, against their definition: the lattice pixels
// (ly i, lx j) enumerated in the order of the full-extent pixels, and the number of them below a cut of the full-extent
// pixel range.  Plain g++, no HIP.  Prints the number of (geometry, cut) pairs checked.
#include <cstdio>

#include "../mcncrossmodalemotions_amd/csrc/conv_plan.h"

int main() {
  long long checked = 0;
  for (int Ho = 1; Ho <= 9; ++Ho)
    for (int Wo = 1; Wo <= 7; ++Wo)
      for (int N = 1; N <= 3; ++N)
        for (int ly = 1; ly <= 3; ++ly)
          for (int lx = 1; lx <= 3; ++lx) {
            const int PI = xm::lattice_extent(Ho, ly), PJ = xm::lattice_extent(Wo, lx);
            if (PI != (Ho + ly - 1) / ly || PJ != (Wo + lx - 1) / lx) {
              printf("extent %d/%d %d/%d\n", Ho, ly, Wo, lx);
              return 1;
            }
            long long below = 0;      // lattice pixels met so far while walking the full-extent pixels in order
            for (long long p = 0; p <= (long long)Ho * Wo * N; ++p) {
              const long long got = xm::lattice_pixels_below(p, Ho, Wo, ly, lx);
              if (got != below) {
                printf("Ho %d Wo %d N %d lattice [%d %d] cut %lld: %lld, expected %lld\n", Ho, Wo, N, ly, lx, p, got, below);
                return 1;
              }
              ++checked;
              if (p == (long long)Ho * Wo * N) break;
              const int i = (int)(p % Ho), j = (int)(p / Ho % Wo), n = (int)(p / ((long long)Ho * Wo));
              if (i % ly == 0 && j % lx == 0) {
                // the lattice index of this pixel is its rank: monotone in p
                if (below != (i / ly) + (long long)PI * ((j / lx) + (long long)PJ * n)) {
                  printf("rank Ho %d Wo %d [%d %d] p %lld\n", Ho, Wo, ly, lx, p);
                  return 1;
                }
                ++below;
              }
            }
            if (below != (long long)PI * PJ * N) return 1;
          }
  printf("%lld\n", checked);
  return 0;
}

/* GRID = VL_NNAFFINEGRID(A, SZ);  DA = VL_NNAFFINEGRID(A, SZ, DY)
 * MatConvNet M-file operator: A is 1 x 1 x 6 x N, SZ = [Ho Wo], GRID 2 x Ho x Wo x N (include/xmodal.h).  Reference use:
 * getBatchFerPlus, teacher/ferplus_baselines.m:209.  Gateway over xm_nnaffinegrid / xm_nnaffinegrid_backward. */
#include "xm_mex.h"

void mexFunction(int nout, mxArray *out[], int nin, mxArray const *in[]) {
  (void)nout;
  XmCall call;
  if (nin < 2) call.fail("XM:invalidArgument", "Not enough arguments.");
  if (mxGetNumberOfElements(in[1]) < 2) call.fail("XM:invalidArgument", "SZ must be [Ho Wo].");
  const double *sz = mxGetPr(in[1]);
  const int Ho = (int)sz[0], Wo = (int)sz[1];
  XmTensor a = call.input(in[0], "A");
  if (a.empty || a.numel() % 6) call.fail("XM:invalidArgument", "A must be 1 x 1 x 6 x N.");
  const int N = (int)(a.numel() / 6);
  if (nin > 2 && !mxIsEmpty(in[2])) {
    XmTensor dy = call.input(in[2], "DY");
    if (dy.numel() != (size_t)2 * Ho * Wo * N) call.fail("XM:invalidArgument", "DY must be 2 x Ho x Wo x N.");
    XmCall::Out da = call.output(1, 1, 6, N);
    call.check(xm_nnaffinegrid_backward(dy.ptr, N, Ho, Wo, da.ptr, nullptr));
    out[0] = call.deliver(da);
    return;
  }
  XmCall::Out grid = call.output(2, Ho, Wo, N);
  call.check(xm_nnaffinegrid(a.ptr, N, Ho, Wo, grid.ptr, nullptr));
  out[0] = call.deliver(grid);
}

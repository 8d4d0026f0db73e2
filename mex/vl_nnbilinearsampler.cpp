/* Y = VL_NNBILINEARSAMPLER(X, GRID);  [DX, DGRID] = VL_NNBILINEARSAMPLER(X, GRID, DY)
 * MatConvNet's compiled operator: X is H x W x C x N, GRID 2 x Ho x Wo x No (No a multiple of N), zero padding
 * (include/xmodal.h).  Reference use: getBatchFerPlus, teacher/ferplus_baselines.m:213.  Gateway over
 * xm_nnbilinearsampler / xm_nnbilinearsampler_backward; DGRID is only computed when it is asked for (nout > 1). */
#include "xm_mex.h"

void mexFunction(int nout, mxArray *out[], int nin, mxArray const *in[]) {
  XmCall call;
  if (nin < 2) call.fail("XM:invalidArgument", "Not enough arguments.");
  XmTensor x = call.input(in[0], "X");
  XmTensor g = call.input(in[1], "GRID");
  if (x.empty || g.empty || g.d[0] != 2) call.fail("XM:invalidArgument", "GRID must be 2 x Ho x Wo x No.");
  const int Ho = g.d[1], Wo = g.d[2], No = g.d[3];
  if (nin > 2 && !mxIsEmpty(in[2])) {
    XmTensor dy = call.input(in[2], "DY");
    if (dy.d[0] != Ho || dy.d[1] != Wo || dy.d[2] != x.d[2] || dy.d[3] != No)
      call.fail("XM:invalidArgument", "DY must be Ho x Wo x C x No.");
    XmCall::Out dx = call.output(x.d[0], x.d[1], x.d[2], x.d[3]);
    XmCall::Out dg;
    if (nout > 1) dg = call.output(2, Ho, Wo, No);
    call.check(xm_nnbilinearsampler_backward(x.ptr, x.d[0], x.d[1], x.d[2], x.d[3], g.ptr, Ho, Wo, No, dy.ptr, dx.ptr,
                                             dg.ptr, nullptr));
    out[0] = call.deliver(dx);
    if (nout > 1) out[1] = call.deliver(dg);
    return;
  }
  XmCall::Out y = call.output(Ho, Wo, x.d[2], No);
  call.check(xm_nnbilinearsampler(x.ptr, x.d[0], x.d[1], x.d[2], x.d[3], g.ptr, Ho, Wo, No, y.ptr, nullptr));
  out[0] = call.deliver(y);
}

/* Y = VL_NNNORMALIZE(X, PARAM);  DZDX = VL_NNNORMALIZE(X, PARAM, DZDY),  PARAM = [N KAPPA ALPHA BETA]
 * MatConvNet ships this operator as a MEX file next to vl_nnconv / vl_nnpool / vl_nnbnorm [EXT: matlab/vl_nnnormalize.m];
 * this is the gateway over xm_nnnormalize_forward / _backward.  Call sites: every dagnn.LRN of a model file
 * (teacher/ferPlusZoo.m:98-100 loads them: the norm1 / norm2 layers of the VGG-M / VGG-F / AlexNet family). */
#include "xm_mex.h"

void mexFunction(int nout, mxArray *out[], int nin, mxArray const *in[]) {
  (void)nout;
  XmCall call;
  if (nin < 2) call.fail("XM:invalidArgument", "Not enough arguments.");
  if ((!mxIsClass(in[1], "double") && !mxIsSingle(in[1])) || mxGetNumberOfElements(in[1]) != 4)
    call.fail("XM:invalidArgument", "PARAM must have four DOUBLE or SINGLE elements [N KAPPA ALPHA BETA].");
  double p[4];
  for (int i = 0; i < 4; ++i)
    p[i] = mxIsClass(in[1], "double") ? mxGetPr(in[1])[i] : (double)((const float *)mxGetData(in[1]))[i];
  if (p[0] < 1 || p[0] != (double)(long long)p[0]) call.fail("XM:invalidArgument", "PARAM(1) = N must be a positive integer.");
  const bool backward = nin > 2 && !mxIsChar(in[2]) && !mxIsEmpty(in[2]);
  for (int next = (nin > 2 && !mxIsChar(in[2])) ? 3 : 2; next < nin; ++next)
    if (!xm_ignored_option(in[next])) call.fail("XM:invalidArgument", "Unknown option.");
  XmTensor x = call.input(in[0], "X");
  XmTensor dz;
  if (backward) dz = call.input(in[2], "DZDY");
  if (backward && (dz.d[0] != x.d[0] || dz.d[1] != x.d[1] || dz.d[2] != x.d[2] || dz.d[3] != x.d[3]))
    call.fail("XM:invalidArgument", "DZDY and X do not have the same size.");
  const int N = p[0] > 2147483647.0 ? 2147483647 : (int)p[0];
  XmCall::Out y = call.output(x.d[0], x.d[1], x.d[2], x.d[3]);
  if (backward)
    call.check(xm_nnnormalize_backward(x.ptr, dz.ptr, x.d[0], x.d[1], x.d[2], x.d[3], N, (float)p[1], (float)p[2],
                                       (float)p[3], y.ptr, nullptr));
  else
    call.check(xm_nnnormalize_forward(x.ptr, x.d[0], x.d[1], x.d[2], x.d[3], N, (float)p[1], (float)p[2], (float)p[3],
                                      y.ptr, nullptr));
  out[0] = call.deliver(y);
}

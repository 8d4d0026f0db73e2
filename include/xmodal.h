/*
 * xmodal.h -- C ABI of libxmodal_hip.so, the MI355X (gfx950) replacement for the
 * MatConvNet / mcnExtraLayers operator MEX files that albanie/mcnCrossModalEmotions
 * drives on its distillation hot path.
 *
 * One entry point per MATLAB operator direction.  A MEX gateway (the mex/ sources,
 * INTEGRATION.md) or the ctypes mirror (mcncrossmodalemotions_amd/vl.py) maps the
 * MATLAB call 1:1 onto these.  The reference reaches them through dagnn.DagNN.eval:
 *     emoVoxCeleb/fetch_emovoxceleb_imdb.m:129   (teacher forward, test mode)
 *     external/compute_audio_feats.m:126         (student forward)
 *     emoVoxCeleb/run_distillation.m:170-182     (cnn_train_dag: fwd + bwd + update)
 *
 * Conventions
 *   - every tensor is MATLAB `single`, H x W x C x N, column-major (H fastest),
 *     densely packed, resident in device (HBM) memory; the caller owns all buffers,
 *     inputs are never written (MATLAB copy-on-write safe), outputs never alias inputs;
 *   - filters are FH x FW x FC x K (groups = C / FC), biases K x 1 (NULL = none);
 *   - pad = [top bottom left right], stride = [sy sx], dilate = [dy dx];
 *   - `stream` is a hipStream_t (NULL = the null stream, MatConvNet's behaviour);
 *     calls are asynchronous with respect to the host, ordered on that stream;
 *   - return value 0 = ok, otherwise an XM_E* code; xm_last_error() gives the text.
 *     Nothing throws, aborts or leaks across this boundary (a MEX gateway turns a
 *     non-zero code into mexErrMsgIdAndTxt).
 *   - re-entrant per device, not thread-safe (MATLAB calls MEX from one thread).
 *   - FINITE INPUTS.  Several kernels multiply a padded operand position by a zero weight instead of masking it
 *     (conv_stem3_kernel's eighth filter row, the zero-filled rows of the patch kernels, the ones / zero columns of the
 *     Gram route): an Inf or NaN just OUTSIDE an output's receptive field can turn that output into NaN there, where
 *     MatConvNet -- and this library's generic implicit-GEMM arm -- would stay finite.  Results are specified for finite
 *     X, F, DZDY; which arm runs is a function of (shape, tuning table, exec hint), see xm_set_exec_hint.
 *     The bf16x3 arm (xm_nnconv_forward_split) narrows this further: its derived error bound holds for operands whose
 *     magnitude is 0 or within [2^-100, 2^100].  Outside that range the hi half can overflow to Inf or the lo half
 *     underflow to 0 (the result is then NaN / Inf, or carries a plain bf16 rounding of that operand); the kernel faults on
 *     no finite input.
 */
#ifndef XMODAL_H
#define XMODAL_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

enum {
  XM_OK = 0,
  XM_EINVAL = 1,   /* bad shape / option combination (MATLAB side: "XM:invalidArgument") */
  XM_ENOMEM = 2,   /* workspace allocation failed */
  XM_EHIP = 3,     /* HIP runtime error (text has hipGetErrorString) */
  XM_ETOOBIG = 4,  /* a tensor has >= 2^31 elements */
  XM_ENOTSUP = 5   /* valid MatConvNet call that this build does not cover */
};

enum { XM_POOL_MAX = 0, XM_POOL_AVG = 1 };
enum { XM_LOSS_SOFTMAXLOG = 0, XM_LOSS_CLASSERROR = 1 };
enum { XM_AGG_MAX = 0, XM_AGG_MEAN = 1, XM_AGG_PEAK = 2 };
/* xm_mnrfit status per problem */
enum { XM_MNR_CONVERGED = 0, XM_MNR_ITERLIMIT = 1, XM_MNR_NOTPD = 2, XM_MNR_BADINPUT = 3 };
/* xm_roc status per problem */
enum { XM_ROC_OK = 0, XM_ROC_NAN = 1, XM_ROC_BADINPUT = 2 };

/* fused-epilogue flags for xm_nnconv_forward_fused / xm_nnbnorm_forward_fused */
enum { XM_FUSE_RELU = 1, XM_BN_BATCH_MOMENTS = 2, XM_FUSE_SIGMOID = 4 };

/* ABI revision: 100 = round 1; 101 = xm_nnbnorm_relu_pool_backward gained `y_pool`, exchange entry points return
 * XM_EINVAL without a communicator; 102 = + xm_nnconv_forward_moments, xm_nnbnorm_backward_dxsum, xm_nnconv_forward_gated;
 * 103 = + xm_nnpool_global_avg_backward_accum; 104 = + xm_nnconv_backward_filter_bnrelupool, xm_nndropout_forward / _apply, xm_resample, xm_se_tail_backward_reduce / _apply, xm_se_squeeze_bn, xm_scale_axpy_bn; 105 = + xm_set_exec_hint / xm_get_exec_hint; 106 = + xm_nnconv_bnorm_relu_pool_forward, xm_stem_gram, xm_stem_gram_moments, xm_nnconv_backward_filter_bnrelupool_gram; 107 = + xm_nnaffinegrid / _backward, xm_nnbilinearsampler / _backward, xm_ferplus_batch; 108 = + XM_AGG_PEAK, xm_mnrfit, xm_mnrval; 109 = + xm_roc, xm_roc_launches, xm_label_hist; 110 = + xm_group_rows, xm_gather_rows, xm_scatter_rows, xm_track_peaks; 111 = + xm_wav_batch; 112 = + xm_spec_bucket_batch; 113 = + xm_jpeg_plan, xm_jpeg_decode_batch; 114 = + xm_wav_plan, xm_wav_decode_batch; 115 = + xm_jpeg_decode_batch_split, xm_jpeg_split_geometry; 116 = + xm_pixcsv_plan, xm_pixcsv_decode_batch, xm_pixcsv_geometry; 117 = + xm_nnconv_forward_strided_residual; 118 = + xm_solver_update; 119 = + xm_nnnormalize_forward / _backward, xm_nnnormalize_geometry; 120 = + xm_jpeg_plan_prog, xm_jpeg_decode_batch_prog; 121 = + xm_window_targets; 122 = + xm_wav_plan_fs, xm_wav_decode_resample_batch, xm_wav_resample_geometry; 123 = + xm_nnconv_forward_lattice; 124 = + xm_nnconv_forward_split, xm_nnconv_split_geometry, XM_CONV_F32 / XM_CONV_BF16X3; 125 = + xm_imread_plan, xm_imread_transform_batch, xm_imread_geometry, xm_imread_round_u8; 126 = + xm_roc_geometry (additions never change the revision's meaning for older bindings).  A binding checks xm_version() >= the revision it was written against. */
int xm_version(void);
const char *xm_last_error(void);
/* Device memory for hosts that have no device-array type of their own (MATLAB's gpuArray is CUDA-only: on an
 * MI355X host the MEX layer keeps tensors in buffers obtained here and hands MATLAB an opaque handle -- mex/xm_mex.h,
 * mex/matlab/xmArray.m).  Plain hipMalloc / hipFree / hipMemcpy underneath; upload / download are synchronous with
 * respect to the host and ordered after everything enqueued on the null stream. */
int xm_device_alloc(void **ptr, size_t bytes);
int xm_device_free(void *ptr);
int xm_device_upload(void *dst_device, const void *src_host, size_t bytes);
int xm_device_download(void *dst_host, const void *src_device, size_t bytes);
int xm_device_synchronize(void);
/* Tile-configuration table of vl_nnconv ("find mode": the first time a (direction, geometry) is seen every tile
 * configuration is timed on the caller's stream and the winner kept; the device is drained first -- hipDeviceSynchronize --
 * so that the candidates run alone: do not meet a new shape while ANY stream of the process is being captured into a graph;
 * a stream that is itself being captured gets the analytic choice instead).  The table persists in a text file next to the
 * library (tune_gfx950.txt; $XM_TUNE_FILE overrides, XM_TUNE_FILE="" disables): loaded before the first lookup,
 * written by xm_tune_save.  With the shipped table the kernel and tile choice -- hence the summation order and the bits of
 * every result -- is a function of (shape, table, execution hint below) and of NOTHING else: the same in every process,
 * whatever it called before, on whatever streams; known shapes cost no timed launches on first use
 * (external/compute_audio_feats.m:116-136 walks ten width buckets).  XM_AUTOTUNE=0 uses the analytic model instead.
 * One exception to "the same bits": the dX of xm_nnbilinearsampler_backward is scattered with float atomics (overlapping
 * grids add into the same pixels), so its last bits depend on the order the adds arrive in; every other output of the
 * library, the sampler's dGrid included, is a function of the inputs alone. */
/* Execution hint, an explicit statement of the host about HOW it calls (process-wide; default 0):
 *   XM_EXEC_SINGLE_STREAM  every operator call of this process arrives on ONE stream (MatConvNet's own sequence:
 *                          cnn_train_dag -> net.eval -> vl_nn* one after the other, run_distillation.m:170-182; what the
 *                          MEX binding does), so a kernel never shares the chip with another stream's kernel.  Kernels
 *                          that are faster alone but poor neighbours (conv_wgrad_patch_kernel: 48 KB of LDS x 3 blocks per
 *                          CU) become candidates.  A host that overlaps streams (dagnn.DagNN.wgradStream, bench.py's
 *                          default) leaves it 0.
 * Same results within the operator tolerance either way; another kernel is another summation order, so set the hint once,
 * before the first operator call, and identically on every worker.  Unknown bits: XM_EINVAL. */
enum { XM_EXEC_SINGLE_STREAM = 1 };
int xm_set_exec_hint(unsigned flags);
unsigned xm_get_exec_hint(void);
int xm_tune_load(const char *path);   /* NULL / "" = the default file; returns the number of entries ADDED: an entry the
                                         table already holds keeps its value and is not counted */
int xm_tune_save(const char *path);   /* NULL / "" = the default file; the table written is the process's merged with the
                                         DEFAULT file (loaded first if it was not yet), not with `path`; atomic (rename) */
int xm_tune_entries(int *total, int *unsaved);
/* optional: pre-size the internal scratch (split-K partials, filter transposes, tap tables). */
int xm_workspace_reserve(size_t bytes);
size_t xm_workspace_bytes(void);
/* Scratch is one grow-only buffer per stream; growing it frees the old buffer.  A HIP graph captured earlier still
 * holds the old address: reserve the largest need of a stream BEFORE capturing on it, and re-capture when the
 * generation counter (incremented by every growth, any stream) has moved since the capture. */
int xm_workspace_reserve_stream(size_t bytes, void *stream);
unsigned long long xm_workspace_generation(void);
/* output extent of conv / pool along one axis: floor((in + pa + pb - ((f-1)*d+1)) / s) + 1 */
int xm_out_size(int in, int pad_a, int pad_b, int f, int dilate, int stride);

/* ---- vl_nnconv  (MatConvNet matlab/vl_nnconv.m; dagnn.Conv at emoVoxZoo.m:118) -------------
 * Y = vl_nnconv(X, F, B, 'stride', [sy sx], 'pad', [t b l r], 'dilate', [dy dx])
 * Every pointer of the xm_nnconv_* entry points need only be 4-byte aligned (a float boundary): the alignment of an
 * operand selects between kernels (16- / 8-byte accesses where every operand they touch allows them, 4-byte ones
 * otherwise) and never changes what is computed. */
int xm_nnconv_forward(const float *x, int H, int W, int C, int N, const float *f, int FH, int FW,
                      int FC, int K, const float *b, float *y, int sy, int sx, int pt, int pb,
                      int pl, int pr, int dy, int dx, void *stream);
/* Extension (not a MatConvNet signature): same convolution with a fused epilogue
 *   y = act( (conv + b) .* scale_k + shift_k + residual ),  scale/shift/residual may be NULL;
 *   act = vl_nnrelu (XM_FUSE_RELU) or vl_nnsigmoid (XM_FUSE_SIGMOID: the SE gate fc2 -> sigmoid).
 * Used to fold test-mode vl_nnbnorm, dagnn.Sum and vl_nnrelu of the frozen teacher into the
 * producing convolution (fetch_emovoxceleb_imdb.m:107 sets dag.mode = 'test'). */
int xm_nnconv_forward_fused(const float *x, int H, int W, int C, int N, const float *f, int FH,
                            int FW, int FC, int K, const float *b, float *y, int sy, int sx,
                            int pt, int pb, int pl, int pr, int dy, int dx, const float *scale,
                            const float *shift, const float *residual, int flags, void *stream);
/* Extension: xm_nnconv_forward_fused with a per-(channel, sample) multiplier between the scale / shift and the residual:
 *   y = act( ((conv + b) .* scale_k + shift_k) .* gate(k, n) + residual ),   gate = 1 x 1 x K x N.
 * The SE block of senet50-ferplus (mcnExtraLayers dagnn.Axpy: out = a .* x + shortcut, teacher/ferPlusZoo.m:86-112;
 * fetch_emovoxceleb_imdb.m:98-136 runs it in test mode): x is the output of a bias-free 1 x 1 projection + test-mode
 * bnorm, i.e. affine in its input u, so the squeeze mean(x) = scale .* (F * mean(u)) + shift can be taken from the 4 x
 * narrower u BEFORE the projection runs; the gate a is then known when the projection's epilogue writes, and
 * relu(a .* x + shortcut) leaves the kernel directly -- x is never written, re-read for the squeeze, re-read and
 * re-written for the excite (three passes over the widest tensors of the network per block). */
int xm_nnconv_forward_gated(const float *x, int H, int W, int C, int N, const float *f, int FH, int FW,
                            int FC, int K, const float *b, float *y, int sy, int sx, int pt, int pb,
                            int pl, int pr, int dy, int dx, const float *scale, const float *shift,
                            const float *gate, const float *residual, int flags, void *stream);
/* Extension (ABI 117): xm_nnconv_forward_gated whose residual has an extent of its own, res_H x res_W x K x N, and is
 * SAMPLED with a stride: output pixel (oy, ox) adds residual(oy * res_sy, ox * res_sx, k, n).  gate == NULL is the plain
 * fused epilogue of xm_nnconv_forward_fused; both older entry points are this one with the residual at output extent and
 * unit stride.  XM_EINVAL unless Ho == floor((res_H - 1) / res_sy) + 1 and Wo == floor((res_W - 1) / res_sx) + 1.
 * What it is for: the last 1 x 1 expansion of a ResNet stage whose only readers are the 1 x 1 / stride-s convolutions that
 * open the next stage (Caffe-style: stride on the first 1 x 1).  Run with stride s over its own input it computes exactly the
 * pixels those readers look at; its shortcut operand still has the full extent and is read at every s-th row and column.
 * Restriction: a call whose residual is really strided (not at output extent with unit stride) runs the register-staged
 * implicit-GEMM kernel only and NEVER splits its reduction (no split-K, no hybrid remainder), so that, with a tile configuration
 * of the same chain structure, its outputs are the bits the full-extent layer gives the same pixels.  The price: a problem
 * with few output tiles and a deep reduction underfills the chip (the pruned res4f expansion at 32 faces: 208 blocks on 256
 * CUs).  Only the "conv_splits" test switch (xmodal_prof.h) makes such a call split. */
int xm_nnconv_forward_strided_residual(const float *x, int H, int W, int C, int N, const float *f, int FH, int FW,
                                       int FC, int K, const float *b, float *y, int sy, int sx, int pt, int pb,
                                       int pl, int pr, int dy, int dx, const float *scale, const float *shift,
                                       const float *gate, const float *residual, int res_H, int res_W, int res_sy,
                                       int res_sx, int flags, void *stream);
/* Extension (ABI 123): xm_nnconv_forward_fused on an OUTPUT LATTICE, written in place.  The layer is computed only at the
 * output pixels (lat_y * i, lat_x * j), i < floor((Ho - 1) / lat_y) + 1, j likewise, and stored at those positions of the
 * full-extent Ho x Wo x K x N tensor y; every other element of y is left untouched (its content is whatever the caller had
 * there).  What it is for: a 3 x 3 layer whose only reader is a stage-end 1 x 1 expansion that runs with stride s (above):
 * the reader looks at one pixel in s * s, the others need not be computed, and y keeps the extent the reader expects.
 * The same bits: every lattice pixel gets the bits a full-extent call (xm_nnconv_forward_fused, same operands) gives it.  The
 * launch takes the tile configuration of the FULL-EXTENT layer (table entry or modelled choice under the full-extent key), its
 * split-K cut points (an LDS-DMA selection runs as a register-staged configuration with ONE accumulator chain, which is how
 * the LDS-DMA kernels sum), and, where that launch runs a hybrid remainder, computes the lattice pixels below the hybrid cut
 * unsplit and the others as a split launch with the hybrid's cut points.  Where that is not possible -- the full-extent
 * selection is not known without a measurement (find mode on, shape not in the table: the call measures it like any first
 * call), or it is not an implicit-GEMM launch (skinny, stem or halo-patch kernels), or the layer has filter groups -- the call runs the layer at FULL
 * EXTENT and writes all of y: bits come before FLOPs.  lat_y == lat_x == 1 is xm_nnconv_forward_fused.
 * XM_ENOTSUP: a residual operand, XM_FUSE_SIGMOID. */
int xm_nnconv_forward_lattice(const float *x, int H, int W, int C, int N, const float *f, int FH, int FW, int FC, int K,
                              const float *b, float *y, int sy, int sx, int pt, int pb, int pl, int pr, int dy, int dx,
                              const float *scale, const float *shift, const float *residual, int flags, int lat_y,
                              int lat_x, void *stream);
/* Extension (ABI 124): the bf16x3 arm of 1 x 1 layers -- an opt-in fast mode with a stated error, for forward-only
 * (frozen teacher) use.  Operands, optional NULLs, extent checks and XM_FUSE_RELU are those of
 * xm_nnconv_forward_strided_residual:
 *   y(oy, ox, k, n) = act( ((sum_c x(oy sy, ox sx, c, n) f(c, k) + b_k) scale_k + shift_k) gate(k, n)
 *                          + residual(oy res_sy, ox res_sx, k, n) )
 * with the epilogue in fp32, in the order of operations of the fp32 kernels; only the dot product differs.  Each fp32
 * operand is written v = hi + lo + r, hi = bf16(v) (round to nearest even), lo = bf16(v - hi) (v - hi is exact), so
 * |v - hi| <= 2^-8 |v| and |r| <= 2^-16 |v|.  Per 16 reduction steps three v_mfma_f32_32x32x16_bf16 add into ONE fp32
 * accumulator in this fixed order, small terms first:  x_lo f_hi,  x_hi f_lo,  x_hi f_hi  (each bf16 x bf16 product is exact
 * in fp32); c ascends, the C tail is zero-filled.  Dropped per product: x_lo f_lo + r_x f + x r_f, so
 *   | dot - exact | <= 3 * 2^-16 * sum_c |x| |f|  (+ second-order terms, + the fp32 accumulation of C products)
 * -- a DERIVED bound, for operands of magnitude 0 or within [2^-100, 2^100] (FINITE INPUTS above).
 * DETERMINISM: one accumulation chain per output, never split-K, no atomics, one fixed tile configuration and no tuning-table
 * entry: the bits of an output element depend on its own operands only -- not on N, not on which other pixels the call
 * computes (a strided call gives the bits of the unit-stride call on the pre-sampled input), not on what the process ran
 * before.
 * precision: XM_CONV_BF16X3.  XM_CONV_F32 names the other entry points' arithmetic and is XM_EINVAL here, like an unknown
 * value, a NULL tensor with work to do, and residual extents that do not match.  XM_ENOTSUP, with a message, for what the
 * kernel is not built for: a filter larger than 1 x 1, padding, filter groups (FC != C), XM_FUSE_SIGMOID, a tensor of 2^31
 * elements or more.  Dilation is accepted and ignored (a 1 x 1 filter has one tap).  Both kinds are raised before anything
 * touches the device.
 * xm_nnconv_split_geometry: host only, no device call, usable without a GPU.  can: the call above would run; want: a
 * forward-only plan should send this layer to it (a pure function of the shape: the measured rule of conv_split_plan.h;
 * can == 0 implies want == 0); blocks / launches: the launch geometry (128 pixels x 64 output channels per block, pixels
 * numbered across samples; one launch), 0 when can == 0.  Always XM_OK; NULL outputs are skipped. */
enum { XM_CONV_F32 = 0, XM_CONV_BF16X3 = 1 };
int xm_nnconv_forward_split(const float *x, int H, int W, int C, int N, const float *f, int FH, int FW, int FC, int K,
                            const float *b, float *y, int sy, int sx, int pt, int pb, int pl, int pr, int dy, int dx,
                            const float *scale, const float *shift, const float *gate, const float *residual, int res_H,
                            int res_W, int res_sy, int res_sx, int flags, int precision, void *stream);
int xm_nnconv_split_geometry(int H, int W, int C, int N, int FH, int FW, int FC, int K, int sy, int sx, int pt, int pb,
                             int pl, int pr, int dy, int dx, int flags, int *can, int *want, int *blocks, int *launches);
/* Extension: Y = vl_nnconv(X, F, B, ...) AND the batch moments of Y that a train-mode vl_nnbnorm(Y, G, B) would
 * compute first -- moments_out (K x 2, column-major) = [mean_k, sqrt(var_k + epsilon)] over H x W x N, biased
 * variance (emoVoxZoo.m:118-123: every dagnn.Conv of the student is followed by dagnn.BatchNorm).  Hand them to
 * xm_nnbnorm_forward_fused / xm_nnbnorm_relu_pool_forward as `moments_in` and to the backward calls with
 * XM_BN_BATCH_MOMENTS / train = 1: same results as letting vl_nnbnorm compute them, minus one pass over Y (462 MB
 * for the student's first layer at 32 spectrograms) -- the per-channel sums ride in the GEMM epilogue. */
int xm_nnconv_forward_moments(const float *x, int H, int W, int C, int N, const float *f, int FH, int FW,
                              int FC, int K, const float *b, float *y, int sy, int sx, int pt, int pb,
                              int pl, int pr, int dy, int dx, float epsilon, float *moments_out, void *stream);
/* [DX, DF, DB] = vl_nnconv(X, F, B, DZDY, ...); dx_out / df_out / db_out may be NULL
 * (= 'NoDerData' / 'NoDerFilters' / 'NoDerBiases'). */
int xm_nnconv_backward(const float *x, int H, int W, int C, int N, const float *f, int FH, int FW,
                       int FC, int K, const float *dzdy, float *dx_out, float *df_out,
                       float *db_out, int sy, int sx, int pt, int pb, int pl, int pr, int dy,
                       int dx, void *stream);
/* Extension: the DZDX GEMM reads the filter bank transposed (and split by stride parity); building that copy is
 * ~20 us per layer on the critical path of the backward pass.  xm_nnconv_prepare_backward builds it ahead of time
 * into a persistent buffer -- e.g. on a side stream while the forward pass of the same step runs -- and a later
 * xm_nnconv_backward with the same F pointer and geometry uses it (waiting on the device for it if it was built on
 * another stream).  Valid until the parameters change: xm_sgd_update / xm_solver_update (every kind) / xm_average_update
 * invalidate every prepared operand; a host that updates parameters by other means -- or frees a filter tensor, whose
 * address the next allocation may reuse: the operands are keyed by F's address, the filter's size, the number of filter
 * groups, stride, dilation, top / left padding and H, W (not N, nor bottom / right padding) -- calls xm_params_changed().
 * From Python that is vl.params_changed(); dagnn calls it wherever DagNN.paramGeneration moves (pack_params, checkpoint
 * loads, the training update) and when DagNN.move uploads parameters. */
int xm_nnconv_prepare_backward(int H, int W, int C, int N, const float *f, int FH, int FW, int FC, int K,
                               int sy, int sx, int pt, int pb, int pl, int pr, int dy, int dx, void *stream);
int xm_params_changed(void);
/* Extension: DX = dgrad + dx_accum.  dagnn sums the derivatives that reach a variable from several
 * consumers (a ResNet block input: shortcut + branch2a); the sum rides in the dgrad epilogue instead of a
 * separate pass.  dx_accum has the size of X, must not alias dx_out, NULL = plain backward. */
int xm_nnconv_backward_accum(const float *x, int H, int W, int C, int N, const float *f, int FH, int FW,
                             int FC, int K, const float *dzdy, float *dx_out, float *df_out,
                             float *db_out, int sy, int sx, int pt, int pb, int pl, int pr, int dy,
                             int dx, const float *dx_accum, void *stream);
/* Extension: [DZDF, DZDB] of a FIRST-layer convolution together with [DG, DB] of the vl_nnbnorm behind it, when the
 * convolution's output Y feeds vl_nnbnorm -> vl_nnrelu -> vl_nnpool('max') and nothing else (the student's
 * conv1 -> bn1 -> relu1 -> pool1, emoVoxCeleb/emoVoxZoo.m:50-62) and the convolution's own input
 * needs no derivative.  Equivalent to
 *     xm_nnbnorm_relu_pool_backward(Y, ..., argmax, y_pool, dzdy_pool, DX, DG, DB, NULL)   then
 *     xm_nnconv_backward(X, ..., DZDY = DX, NULL, DZDF, DZDB)
 * but DX -- the widest tensor of the student's backward pass, 462 MB at 32 spectrograms -- is never written: the
 * filter-derivative kernel rebuilds it per element from the pooled derivative and the routing table.  Same decisions
 * (ReLU gates, routing) and the same per-element formula; the normalisation's constants are applied in fp32 with a
 * two-float mean instead of fp64 (1 ulp of DX).  Arguments: X / geometry of the convolution as for xm_nnconv_backward
 * (F itself is not needed), Y = its output, then the arguments of xm_nnbnorm_relu_pool_backward.  dzdb_out, dg_out,
 * db_out may be NULL.  Returns XM_ENOTSUP when the shapes are outside what the fused kernel covers (single input
 * channel, <= 96 filters, <= 8 x 7 taps, 3 x 3 / stride-2 unpadded pooling, y_pool given): make the two calls then. */
int xm_nnconv_backward_filter_bnrelupool(const float *x, int H, int W, int C, int N, int FH, int FW, int FC, int K,
                                         int sy, int sx, int pt, int pb, int pl, int pr, int dy, int dx,
                                         const float *y, const float *bn_g, const float *bn_b, const float *moments,
                                         int train, int ph, int pw, int psy, int psx, int ppt, int ppb, int ppl,
                                         int ppr, const unsigned char *argmax, const float *y_pool,
                                         const float *dzdy_pool, float *dzdf_out, float *dzdb_out, float *dg_out,
                                         float *db_out, void *stream);
/* Extension (ABI revision 106): the same derivatives WITHOUT a pass over the convolution's output.  A single-channel
 * first layer is Y[m][p] = sum_t F~[m][t] P~[p][t] over the im2col patches P~ of X (+ a column of ones for the bias), so
 * everything vl_nnbnorm's train-mode derivative needs from Y is a contraction with the (FH FW + 1)^2 Gram matrix
 * G = P~' P~ of the INPUT (xm_stem_gram, fp64 [64][64], row-major; row / column t = u + FH v, t = FH FW: the ones):
 *     A = DZ P~ (DZ: the pooled derivative routed through `argmax`, masked by y_pool > 0; built on chip),
 *     DG = (F~.A - mu A[:, ones]) / sigma, DB = A[:, ones],
 *     [DZDF, DZDB] = g/sigma (A - DB/P G[ones, :] - DG/(sigma P) ((F~ G) - mu G[ones, :]))          (train)
 * with [mu, sigma] = `moments` (the forward call's).  F and B (may be NULL) take Y's place in the argument list; `gram`
 * NULL = computed here; y_pool NULL = the table marks closed windows itself (code 255).  Same routing / ReLU decisions as the composition; the sums are another summation order
 * (fp32 MFMA chains per wave, fp64 across waves and in the closed form).  xm_stem_gram_moments gives the batch moments
 * of Y from G (mean = F~ G[:, ones] / P, E[y^2] = F~ G F~' / P; fp64), i.e. vl_nnbnorm's MOMENTS output for Y without Y.
 * XM_ENOTSUP outside: one input channel, <= 96 filters, 16 ... 63 taps in <= 8 x 7, stride 1 / 2, size(X,1) % 4 == 0,
 * 3 x 3 / stride-2 unpadded max pooling with >= 4 window rows. */
/* Extension (106): Y_POOL, ARGMAX, MOMENTS of
 *     vl_nnpool(vl_nnrelu(vl_nnbnorm(vl_nnconv(X, F, B), G, BB, 'epsilon', e)), [3 3], 'stride', 2, 'method', 'max')
 * for a single-channel first layer (7 x 7 / stride 2, K % 8 == 0) in ONE kernel: the convolution's output -- 3.7 GB at 256
 * spectrograms -- is never written.  Train mode (moments_in NULL): `gram` (caller-owned fp64 [64][64]) receives
 * xm_stem_gram(X), the batch moments come from it (xm_stem_gram_moments) before the kernel starts, and MOMENTS_OUT is
 * vl_nnbnorm's third output; test mode: moments_in as given.  The normalisation is folded into the MFMA operand
 * (g/sigma F, constant term on a spare reduction index), i.e. another rounding order than bnorm(conv(x)): 1e-6 relative.
 * ARGMAX: code = dh + 3 dw of the FIRST maximum in column-major scan order, or 255 where the window's maximum did not
 * pass the ReLU (y_pool == 0; the derivative of such a window is zero wherever it is routed) -- the form
 * xm_nnconv_backward_filter_bnrelupool_gram(..., y_pool = NULL, ...) takes. */
int xm_nnconv_bnorm_relu_pool_forward(const float *x, int H, int W, int C, int N, const float *f, int FH, int FW, int FC,
                                      int K, const float *bias, int sy, int sx, int pt, int pb, int pl, int pr, int dy, int dx,
                                      const float *bn_g, const float *bn_b, float epsilon, const float *moments_in, int ph,
                                      int pw, int psy, int psx, int ppt, int ppb, int ppl, int ppr, double *gram,
                                      float *y_pool, unsigned char *argmax, float *moments_out, void *stream);
int xm_stem_gram(const float *x, int H, int W, int N, int FH, int FW, int sy, int sx, int pt, int pb, int pl, int pr,
                 double *gram, void *stream);
int xm_stem_gram_moments(const double *gram, const float *f, const float *b, int FH, int FW, int K, float epsilon,
                         float *moments_out, void *stream);
int xm_nnconv_backward_filter_bnrelupool_gram(const float *x, int H, int W, int C, int N, const float *f, int FH, int FW,
                                              int FC, int K, const float *bias, int sy, int sx, int pt, int pb, int pl,
                                              int pr, int dy, int dx, const float *bn_g, const float *moments, int train,
                                              int ph, int pw, int psy, int psx, int ppt, int ppb, int ppl, int ppr,
                                              const unsigned char *argmax, const float *y_pool, const float *dzdy_pool,
                                              const double *gram, float *df_out, float *dbias_out, float *dg_out,
                                              float *db_out, void *stream);

/* ---- vl_nnpool  (matlab/vl_nnpool.m; pool6 resized at emoVoxZoo.m:256-269) ------------------
 * Y = vl_nnpool(X, [ph pw], 'stride', .., 'pad', .., 'method', 'max'|'avg') */
int xm_nnpool_forward(const float *x, int H, int W, int C, int N, int ph, int pw, int sy, int sx,
                      int pt, int pb, int pl, int pr, int method, float *y, void *stream);
/* DX = vl_nnpool(X, [ph pw], DZDY, ...) */
int xm_nnpool_backward(const float *x, int H, int W, int C, int N, int ph, int pw, int sy, int sx,
                       int pt, int pb, int pl, int pr, int method, const float *dzdy, float *dx_out,
                       void *stream);

/* Extension (max pooling): the forward pass also records, per output, the position of the first
 * maximum inside its window (one byte: dh + ph * dw); the backward pass then routes DZDY from that
 * table without re-reading X.  Results are identical to xm_nnpool_forward / xm_nnpool_backward. */
int xm_nnpool_forward_argmax(const float *x, int H, int W, int C, int N, int ph, int pw, int sy,
                             int sx, int pt, int pb, int pl, int pr, float *y, unsigned char *argmax,
                             void *stream);
int xm_nnpool_backward_argmax(const unsigned char *argmax, int H, int W, int C, int N, int ph, int pw,
                              int sy, int sx, int pt, int pb, int pl, int pr, const float *dzdy,
                              float *dx_out, void *stream);
/* Global average pooling (mcnExtraLayers dagnn.GlobalPooling, the SE squeeze) backward where X has a second consumer
 * that already left its derivative (the SE excite: dagnn accumulates derivatives at forks): dx = accum + dzdy / (H W)
 * in one pass; bit-identical to xm_nnpool_backward followed by the sum. */
int xm_nnpool_global_avg_backward_accum(const float *dzdy, const float *accum, float *dx_out, int H, int W, int C, int N,
                                        void *stream);

/* ---- vl_nnbnorm  (matlab/vl_nnbnorm.m) -----------------------------------------------------
 * Y = vl_nnbnorm(X, G, B, 'epsilon', e [, 'moments', M]); M is C x 2 = [mean, sqrt(var+e)].
 * moments_in == NULL: train mode (batch moments, biased variance); they are written to
 * moments_out when it is non-NULL.  moments_in != NULL: test mode. */
int xm_nnbnorm_forward(const float *x, int H, int W, int C, int N, const float *g, const float *b,
                       float epsilon, const float *moments_in, float *y, float *moments_out,
                       void *stream);
/* Extension: vl_nnbnorm followed by vl_nnrelu in one pass (flags = XM_FUSE_RELU). */
int xm_nnbnorm_forward_fused(const float *x, int H, int W, int C, int N, const float *g,
                             const float *b, float epsilon, const float *moments_in, float *y,
                             float *moments_out, int flags, void *stream);
/* [DX, DG, DB, MOMENTS] = vl_nnbnorm(X, G, B, DZDY, ...) */
int xm_nnbnorm_backward(const float *x, int H, int W, int C, int N, const float *g, const float *b,
                        const float *dzdy, float epsilon, const float *moments_in, float *dx_out,
                        float *dg_out, float *db_out, float *moments_out, void *stream);
/* Extension: backward through relu(bnorm(x)): `y` is the fused forward output; dzdy is masked
 * by (y > 0) before the vl_nnbnorm backward formulas (flags & XM_FUSE_RELU).
 * flags & XM_BN_BATCH_MOMENTS: moments_in holds the BATCH moments the forward call returned for this
 * very X (train mode): they are not recomputed (one pass over X less), the train-mode formulas apply. */
int xm_nnbnorm_backward_fused(const float *x, const float *y, int H, int W, int C, int N,
                              const float *g, const float *b, const float *dzdy, float epsilon,
                              const float *moments_in, float *dx_out, float *dg_out, float *db_out,
                              float *moments_out, int flags, void *stream);

/* Extension: xm_nnbnorm_backward_fused that also returns dxsum_out (C x 1) = sum of DX over H x W x N per channel.  When
 * X is the output of a vl_nnconv with biases, that sum IS the convolution's DZDB (vl_nnconv: dzdb = sum of dzdy), so the
 * host skips the bias half of xm_nnconv_backward (db_out = NULL) -- one pass over DX and three launches less per layer
 * (emoVoxZoo.m:118-123: conv -> bnorm -> relu for every layer of the student).  dx_out must not be NULL. */
int xm_nnbnorm_backward_dxsum(const float *x, const float *y, int H, int W, int C, int N,
                              const float *g, const float *b, const float *dzdy, float epsilon,
                              const float *moments_in, float *dx_out, float *dg_out, float *db_out,
                              float *moments_out, float *dxsum_out, int flags, void *stream);

/* Extension: vl_nnbnorm -> vl_nnrelu -> vl_nnpool('max') as one fused operator pair.  The
 * normalised / rectified tensor is never materialised: forward = moments (train mode) + one pass
 * that normalises, rectifies and pools while recording the argmax table; backward = two passes
 * over X that rebuild the routed, ReLU-masked derivative on the fly.  Results are identical to the
 * three separate operators.  `moments` (backward) is what the forward returned; train != 0 applies
 * the batch-statistics terms of vl_nnbnorm's backward (train mode), 0 treats them as constants.
 * y_pool (backward, optional): the forward's pooled output; with it the two per-channel sums are formed from
 * the pooled tensors alone (x is read once instead of twice).
 * dxsum_out (optional, C floats): per-channel sum of DX = the DZDB of a vl_nnconv that produced X. */
int xm_nnbnorm_relu_pool_forward(const float *x, int H, int W, int C, int N, const float *g,
                                 const float *b, float epsilon, const float *moments_in, int ph, int pw,
                                 int sy, int sx, int pt, int pb, int pl, int pr, float *y_pool,
                                 unsigned char *argmax, float *moments_out, void *stream);
int xm_nnbnorm_relu_pool_backward(const float *x, int H, int W, int C, int N, const float *g,
                                  const float *b, const float *moments, int train, int ph, int pw,
                                  int sy, int sx, int pt, int pb, int pl, int pr,
                                  const unsigned char *argmax, const float *y_pool, const float *dzdy_pool,
                                  float *dx_out, float *dg_out, float *db_out, float *dxsum_out, void *stream);

/* ---- elementwise: vl_nnrelu, vl_nnsigmoid, dagnn.Sum, mcnExtraLayers Scale/Axpy ------------
 * dzdy == NULL: forward; otherwise y receives DZDX. */
int xm_nnrelu(const float *x, size_t n, float leak, const float *dzdy, float *y, void *stream);
int xm_nnsigmoid(const float *x, size_t n, const float *dzdy, float *y, void *stream);
/* y = a + b, optional fused relu (flags = XM_FUSE_RELU) -- dagnn.Sum (+ vl_nnrelu) */
int xm_sum2(const float *a, const float *b, size_t n, int flags, float *y, void *stream);
/* SE excite: y(:,:,c,n) = a(c,n) * x(:,:,c,n) [+ r(:,:,c,n)] [relu]; a is 1 x 1 x C x N */
int xm_scale_axpy(const float *x, int HW, int CN, const float *a, const float *r, int flags,
                  float *y, void *stream);
/* backward of y = a .* x: dx = a .* dzdy (NULL to skip), da(c,n) = sum_hw dzdy .* x */
int xm_scale_backward(const float *x, int HW, int CN, const float *a, const float *dzdy,
                      float *dx_out, float *da_out, void *stream);

/* ---- vl_nndropout (dagnn.DropOut, inserted behind fc6 / fc7 by emoVoxZoo.m:116-135,272-277 when opts.dropout > 0) ----
 * [Y, MASK] = vl_nndropout(X, 'rate', r):  MASK = (u >= r) / (1 - r), u ~ U[0, 1), Y = MASK .* X.  MATLAB's random
 * stream cannot be reproduced; the mask comes from a stateless Philox4x32-10 stream: key = seed, counter = element
 * index / 4 + offset (four elements per counter).  The host advances `offset` by ceil(n / 4) per call so that masks
 * never repeat within a run.  mask_out (size of X, single, values 0 or 1 / (1 - r)) may be NULL. */
int xm_nndropout_forward(const float *x, size_t n, float rate, unsigned long long seed, unsigned long long offset,
                         float *y, float *mask_out, void *stream);
/* Y = X .* MASK: DZDX = vl_nndropout(X, DZDY, 'mask', MASK), and the forward call with a given mask */
int xm_nndropout_apply(const float *x, const float *mask, size_t n, float *y, void *stream);

/* Extension: backward of the TAIL of an SE bottleneck block in training mode (the trainable SE-ResNet-50 teacher,
 * teacher/ferplus_baselines.m:140-141; BASELINE config 5):
 *     U -> vl_nnbnorm(G, B) -> X;   GP = mean_hw(X) -> fc1 -> relu -> fc2 -> sigmoid = A;   Y = vl_nnrelu(A .* X + S)
 * Two calls replace vl_nnrelu / Axpy / GlobalPooling / vl_nnbnorm backward (13 passes over block-sized tensors -> 8):
 *   xm_se_tail_backward_reduce  reads Y, DZDY, U;  leaves DA = dz/dA (1 x 1 x C x N, what the gate's backward consumes)
 *                               and three sums per (channel, sample) plane in `plane_sums` (caller-owned, 3 C N doubles);
 *   xm_se_tail_backward_apply   after the gate's backward has produced DGP = dz/dGP (1 x 1 x C x N): writes
 *                               DZ = [Y > 0] .* DZDY (the derivative of the shortcut S) and DU = dz/dU, and the bnorm's
 *                               DG / DB.  `moments` are the batch moments of U the forward pass used (train = 1) or
 *                               the stored ones (train = 0).  Same formulas as the separate operators (the bnorm's
 *                               per-element expression in fp64); X is recomputed from U where it is needed. */
/* ... and its forward without materialising X: GP = mean_hw(vl_nnbnorm(U)) and Y = [relu](A .* vl_nnbnorm(U) + S) straight
 * from U (the bnorm's own per-element expression: the same bits as vl_nnbnorm followed by vl_nnpool / Axpy), `moments`
 * as above.  With the two backward calls X is never needed, so the bnorm's apply pass disappears. */
int xm_se_squeeze_bn(const float *u, int H, int W, int C, int N, const float *g, const float *b, const float *moments,
                     float *gp_out, void *stream);
int xm_scale_axpy_bn(const float *u, int H, int W, int C, int N, const float *a, const float *r, const float *g,
                     const float *b, const float *moments, int flags, float *y, void *stream);
int xm_se_tail_backward_reduce(const float *y, const float *dzdy, const float *u, int H, int W, int C, int N,
                               const float *g, const float *b, const float *moments, float *da_out, double *plane_sums,
                               void *stream);
int xm_se_tail_backward_apply(const float *y, const float *dzdy, const float *u, int H, int W, int C, int N,
                              const float *gate, const float *dgp, const float *g, const float *moments, int train,
                              const double *plane_sums, float *dz_out, float *du_out, float *dg_out, float *db_out,
                              void *stream);

/* ---- losses --------------------------------------------------------------------------------
 * vl_nnsoftmaxt(X, 'temperature', T): softmax(X / T) along dim 3; X is HW x C x N */
int xm_nnsoftmaxt(const float *x, int HW, int C, int N, float temperature, float *y, void *stream);
/* DZDX = vl_nnsoftmax(X, DZDY) [EXT, SURVEY 8b] generalised to a temperature:
 * y = softmax(x/T) along C; dx = y .* (dzdy - sum_c(dzdy .* y)) / T.  Same indexing as above. */
int xm_nnsoftmaxt_backward(const float *x, const float *dzdy, int HW, int C, int N, float temperature,
                           float *dx, void *stream);
/* vl_nnsoftmaxceloss(X, P [, DZDY], 'temperature', T, 'logitTargets', tf, 'instanceWeights', w)
 * (dagnn.SoftmaxCELoss at emoVoxZoo.m:152, ferPlusZoo.m:244).  X, P: 1 x 1 x C x N, C <= 64.
 * forward (dzdy == NULL): y[0] = sum_n w_n * CE(softmax(P/T) or P, softmax(X/T));
 * backward: y (C*N floats) = dzdy[0] * w_n * (softmax(X/T) * sum(p) - p) / T.
 * dzdy is a DEVICE pointer to one float. */
int xm_nnsoftmaxceloss(const float *x, const float *p, int C, int N, float temperature,
                       int logit_targets, const float *instance_weights, const float *dzdy,
                       float *y, void *stream);
/* vl_nneuclideanloss(X, T [, DZDY], 'instanceWeights', w)  /  vl_nnhuberloss(X, T [, DZDY], 'sigma', s,
 * 'instanceWeights', w) -- mcnExtraLayers; dagnn.EuclideanLoss / dagnn.HuberLoss at emoVoxZoo.m:139-146.
 * X, T: E elements per sample x N samples; w: N weights or NULL (broadcast over a sample's elements).
 * forward (dzdy == NULL): y[0] = sum_n w_n sum_e l(x - t), l(d) = d^2/2 (euclidean) or smooth-L1 with
 * knee 1/sigma^2 (huber); backward: y (E*N floats) = dzdy[0] * w_n * l'(x - t).  dzdy: DEVICE pointer. */
#define XM_REGLOSS_EUCLIDEAN 0
#define XM_REGLOSS_HUBER 1
int xm_nnregloss(const float *x, const float *t, int E, int N, int kind, float sigma,
                 const float *instance_weights, const float *dzdy, float *y, void *stream);
/* vl_nnloss(X, c [, DZDY], 'loss', 'softmaxlog'|'classerror'); labels are 1-based floats.  A sample whose label is
 * outside 1..C (MatConvNet's "label 0 is skipped", extended to every invalid label) adds 0 to Y and gets a zero column of
 * DZDX, for both losses. */
int xm_nnloss(const float *x, const float *labels, int C, int N, int loss, const float *dzdy,
              float *y, void *stream);

/* ---- cnn_train_dag accumulateGradients + ParameterServer (run_distillation.m:88,170-182) ----
 * trainMethod 'gradient':  m <- momentum*m - (wd*w + der/batch);  w <- w + lr*m */
int xm_sgd_update(float *w, float *m, const float *der, size_t n, float lr, float momentum,
                  float weight_decay, float batch, void *stream);
/* cnn_train_dag's 'solver' option and the 'nesterovUpdate' arm of its default solver (ABI 118).  One launch updates one flat
 * segment in place.  The formulas are restated from MatConvNet's +solver package and cnn_train_dag.m [EXT]; MatConvNet is
 * not part of this tree, so parity with it is not pinned by a test (the tests hold the kernel to a numpy restatement of
 * the lines below).  First  g = der * (1/batch) + weight_decay * w  (vl_taccum(1/batchSize, parDer, thisDecay, value)),
 * then, in fp32 and in this order of operations:
 *   XM_SOLVER_ADAGRAD   s1 = g_sqr                  g_sqr = g_sqr*rho + g.^2;  w = w - lr*g ./ (sqrt(g_sqr) + epsilon)
 *   XM_SOLVER_RMSPROP   s1 = g_sqr                  g_sqr = g_sqr*rho + g.^2*(1-rho);  w = w - lr*g ./ (sqrt(g_sqr) + epsilon)
 *   XM_SOLVER_ADADELTA  s1 = g_sqr, s2 = delta_sqr  g_sqr = g_sqr*rho + g.^2*(1-rho);
 *                                                   delta = -sqrt((delta_sqr + epsilon) ./ (g_sqr + epsilon)) .* g;
 *                                                   delta_sqr = delta_sqr*rho + delta.^2*(1-rho);  w = w + lr*delta
 *   XM_SOLVER_ADAM      s1 = m, s2 = v              m = m + (1-beta1)*(g - m);  v = v + (1-beta2)*(g.^2 - v);
 *                                                   w = w - lr_t * m ./ (sqrt(v) + epsilon),
 *                                                   lr_t = lr*sqrt(1 - beta2^t)/(1 - beta1^t), t = updates so far, this one
 *                                                   included (the HOST counts t and computes lr_t; `lr` is not read)
 *   XM_SOLVER_NESTEROV  s1 = momentum state         m = mom*m - g;  w = w + lr*(mom*m - g)
 * States start at zero (MatConvNet's empty state).  s2 is read and written by ADADELTA and ADAM only; the other kinds
 * accept NULL there and leave a passed buffer untouched.
 * `coef`: HOST pointer to 4 floats, read during the call.  MATLAB evaluates a double scalar expression such as
 * (1 - opts.beta2) in double and only then multiplies the single array, so the host forms these in double and rounds once
 * (1 - 0.999f in fp32 is 1.3e-5 off):
 *                       coef[0]     coef[1]     coef[2]     coef[3]
 *   ADAGRAD             epsilon     rho         -           -          defaults 1e-10, 1
 *   RMSPROP             epsilon     rho         1 - rho     -          defaults 1e-8, 0.99
 *   ADADELTA            epsilon     rho         1 - rho     -          defaults 1e-6, 0.9
 *   ADAM                epsilon     1 - beta1   1 - beta2   lr_t       defaults 1e-8, beta1 0.9, beta2 0.999
 *   NESTEROV            momentum    -           -           -          cnn_train_dag's 'momentum'
 * Unused slots are not read.  XM_EINVAL, before anything touches the device: unknown kind, batch <= 0, NULL coef, and for
 * n > 0 a NULL w, der or s1, or a NULL s2 for ADADELTA / ADAM.  n == 0: XM_OK without a launch. */
enum { XM_SOLVER_ADAGRAD = 0, XM_SOLVER_RMSPROP = 1, XM_SOLVER_ADADELTA = 2, XM_SOLVER_ADAM = 3, XM_SOLVER_NESTEROV = 4 };
int xm_solver_update(int kind, float *w, float *s1, float *s2, const float *der, size_t n, float lr,
                     float weight_decay, float batch, const float *coef, void *stream);
/* trainMethod 'average' (BN moments):  w <- (1-lr)*w + lr*der/denom.
 * MatConvNet [EXT]: dagnn.BatchNorm hands back moments * (its worker's batch size), the workers' values are summed
 * and accumulateGradients divides by the GLOBAL batch size -- workers with ragged shards are weighted by their
 * sample counts.  Single worker: der = the batch moments, denom = 1. */
int xm_average_update(float *w, const float *der, size_t n, float lr, float denom,
                      void *stream);
/* x <- a * x (the worker-batch-size weighting of the moments before the exchange) */
int xm_scale_f32(float *x, size_t n, float a, void *stream);
/* ParameterServer.{start,push,sync,pull}: sum of `buf` over all workers, in place, via RCCL.
 * xm_comm_init takes the 128-byte ncclUniqueId produced by xm_comm_unique_id on rank 0 and
 * distributed by the host (MATLAB labBroadcast / torch.distributed broadcast).
 * CALL ORDER: create the communicator FIRST, before the first operator call / buffer upload of the process (in
 * cnn_train_dag terms: in startup, before net.move('gpu')).  Measured on ROCm 7.0 / RCCL 2.26: a communicator created
 * after the operator streams were in use makes every later step 12 % slower (the backward pass 0.8 ms longer at 32
 * pairs, even if no collective is ever issued); created first, the step time is that of a process without it. */
int xm_comm_unique_id(void *id128);
int xm_comm_init(const void *id128, int rank, int world);
int xm_allreduce_sum_f32(float *buf, size_t n, void *stream);   /* blocking-in-stream-order form: runs on `stream` */
/* Overlapped form (what cnn_train_dag's push-as-derivatives-become-ready / sync-before-update does with 'tmove'):
 *   xm_parserv_push(buf, n, producer)  after the kernels that wrote buf[0..n) were enqueued on `producer`: the sum over
 *                                      all workers starts when they finish and runs on the communicator's own HIP
 *                                      stream -- the producer stream goes on with the rest of the backward pass;
 *   xm_parserv_sync(consumer)          once per minibatch before accumulateGradients: `consumer` waits (on the
 *                                      device, not the host) for every push since the previous sync.
 * Every element must be pushed exactly once per minibatch.  After xm_comm_init(.., world == 1) both are no-ops;
 * WITHOUT a successful xm_comm_init they (and xm_allreduce_sum_f32) return XM_EINVAL -- a worker must never go on
 * training with derivatives that were silently not exchanged. */
int xm_parserv_push(float *buf, size_t n, void *producer_stream);
int xm_parserv_sync(void *consumer_stream);
/* ncclCommCount of the communicator (1 when no communicator exists): proof of the worker count */
int xm_comm_count(int *ranks);
int xm_comm_destroy(void);

/* ---- batch-provider arithmetic (device side of getBatchEmoVoxCeleb / getImageBatch) ---------
 * getBatchEmoVoxCeleb.m:164-169: per-frequency-row mean / unbiased std over time; H x W x 1 x N */
int xm_spec_rownorm(const float *spec, int H, int W, int N, float *out, void *stream);
/* z = resample(zo, p, q) of the speed-perturbation branch (getBatchEmoVoxCeleb.m:102-108, transformation 'S'; MATLAB
 * Signal Processing Toolbox [EXT]): y[j] = sum_k h[(j + delay) q - k p] x[k], j = 0 .. Ly - 1 -- upfirdn(x, h, p, q)
 * with the filter delay removed.  The host designs h (Kaiser-windowed ideal low-pass, batch.resample_design restates
 * the toolbox's recipe) and passes it with p, q already reduced by their gcd. */
int xm_resample(const float *x, int Lx, const float *h, int Lh, int p, int q, int delay, float *y, int Ly, void *stream);
/* The waveform front-end of a whole batch (ABI 111; getBatchEmoVoxCeleb.m:102-135): crop or speed-perturb, zero-pad and
 * mix noise into the L x N sample matrix runSpec takes, clip n at z + n L.  wav / noise are device banks (all tracks /
 * all noise files concatenated, wav_len / noise_len samples); desc holds {src, len, p, q, nsrc, nlen} per clip (device,
 * contiguous), ratio one float per clip (device).  Every z(j, n), j = 0 .. L-1, is written exactly once:
 *   p == q   v = j < len ? wav[src + j] : 0                          (audioread window, zero padded when short, :109-119)
 *   p != q   v = sample j of resample(wav[src .. src + len), p, q) for j < min(ceil(len p / q), L), 0 behind   (:102-108)
 *   nlen > 0 for j < nlen: v += ratio[n] noise[nsrc + j]                                        (z + y .* Nratio, :123-135)
 * resample is the recipe of xm_resample's host design (batch.resample_design) with no filter in memory: p, q are
 * reduced by their gcd here, the 2 * 10 * max(p, q) + 1 Kaiser(5)-windowed sinc taps are evaluated where they are
 * used (~21 per output; the sine from m mod max(p, q) in integers, I0 by its power series) and the gain p / sum(h) of
 * each clip is summed in fp64 by a first kernel into the stream's workspace.  Two launches whatever N is, no atomics;
 * clip n depends on its own descriptor only.  A read outside [0, wav_len) / [0, noise_len) yields 0 and never reaches
 * memory; a descriptor with p or q outside 1 .. 2^20 resamples to zeros.  XM_EINVAL: N < 0, L <= 0, a negative bank
 * length, a NULL tensor with N > 0 (noise may be NULL when noise_len == 0); XM_ETOOBIG: N > 65535; N == 0: XM_OK. */
int xm_wav_batch(const float *wav, long long wav_len, const float *noise, long long noise_len, const long long *desc,
                 const float *ratio, int N, float *z, int L, void *stream);
/* The whole-clip front-end of external/compute_audio_feats.m:160-185 for N clips of different lengths (ABI 112): runSpec,
 * mean / unbiased std of every frequency row over ALL frames of the clip, centre crop to the bucket width.  wav is the
 * device bank of xm_wav_batch (wav_len samples); desc holds {src, len, f0} per clip (int64, device, contiguous); bank is
 * the device filter bank of batch.runSpec, taps x 2B with the tap fastest (taps = Nw + 1: pre-emphasis * Hamming window
 * * DFT, column b = Re of bin b, column B + b = Im), hop = Ns.  With T = floor((len - Nw) / hop) + 1:
 *   frame j covers samples src + hop j - 1 .. src + hop j + Nw - 1; the sample in front of src is ZERO (filter([1 -a],
 *   1, z) starts from rest), samples at or beyond src + len are never read;
 *   mag(b, j) = |sum_k bank(k, b) s(k) + i sum_k bank(k, B + b) s(k)|, j = 0 .. T - 1;
 *   mu(b), sd(b) = mean and unbiased std of mag(b, :) over all T frames;
 *   out(b, i, 1, n) = (mag(b, f0 + i) - mu(b)) / sd(b), i = 0 .. rsize - 1; out is B x rsize x 1 x N.
 * Every output element is written exactly once; clip n depends on its own descriptor only (the grouping of its partial
 * statistics follows the tile list of the call: they are merged in fp64, so the output moves by less than fp32
 * resolves).  Four launches whatever N and the lengths are, no tuning entries, no atomics, scratch from the stream's
 * workspace (transposed bank, tile list, partial statistics, the N rsize B magnitudes of the crops).  A read outside
 * [0, wav_len) yields 0 and never reaches memory; frames of the crop outside [0, T) count as magnitude 0; T < 2 gives
 * NaN as std() of one sample does; len is cut at 2^31.  XM_EINVAL: N < 0, rsize <= 0, a negative bank length, taps < 2,
 * hop < 2, B <= 0, a NULL tensor with N > 0; XM_ETOOBIG: N > 65535; XM_ENOTSUP: B != 512 or a 64-frame sample span
 * beyond 64 KB; N == 0: XM_OK. */
int xm_spec_bucket_batch(const float *wav, long long wav_len, const long long *desc, int N, int rsize, const float *bank,
                         int taps, int hop, int B, float *out, void *stream);
/* |STFT| from the output of the framing convolution (runSpec of getBatchEmoVoxCeleb.m:162 [EXT VGGVox]):
 * reim is 1 x Wo x 2B x N (channel b = Re of bin b, channel B+b = Im), out is B x Wo x 1 x N with
 * out(b, j, 1, n) = sqrt(Re^2 + Im^2).  The framing/windowing/pre-emphasis/DFT itself is one
 * xm_nnconv_forward with a 1 x (Nw+1) x 1 x 2B filter bank and stride [1 Ns] (batch.runSpec). */
int xm_spec_magnitude(const float *reim, int Wo, int B, int N, float *out, void *stream);
/* getBatchEmoVoxCeleb.m:145-158,179-188: for sample n aggregate frame logits (F_total x E,
 * column-major, all wavs concatenated) over rows [first[n], last[n]] (1-based, inclusive)
 * -> out 1 x 1 x E x N and maxLabel (1-based argmax, getBatchEmoVoxCeleb.m:32).
 * agg = XM_AGG_MAX | XM_AGG_MEAN, or XM_AGG_PEAK (ABI 108; selectPeakLogit, external/run_cross_val.m:149-155): the
 * whole row of the block that holds its largest entry, the first one in column-major order as max(logits(:)) finds
 * it (lowest e, then lowest row); an empty range gives -Inf as XM_AGG_MAX does. */
int xm_aggregate_logits(const float *frame_logits, int F_total, int E, const int *first,
                        const int *last, int N, int agg, float *out, float *max_label,
                        void *stream);
/* getBatchEmoVoxCeleb.m:32: [~, maxLabel] = max(lgo, [], 3); x is 1 x 1 x C x N, labels 1-based */
int xm_max_label(const float *x, int C, int N, float *labels, void *stream);
/* getBatchEmoVoxCeleb.m:30-32,145-158,179-188 in ONE launch, straight from the teacher's output (ABI 121): logits is
 * 1 x 1 x E x n as the frozen teacher wrote it (frame f's E logits contiguous), first / last are 1-based inclusive rows
 * into those n frames.  Pair j: the max or mean over its rows of emotions 1..P (lgo = lgo(:,:,1:numPredEmotions,:))
 * -> out 1 x 1 x P x N, and max_label[j] = the first maximum of those P values, 1-based.  Bit for bit what
 * xm_aggregate_logits on the transposed n x E copy, the channel cut and xm_max_label give: the mean is summed in
 * ascending row order, a NaN is dropped by max, propagated by mean and never wins the label, an empty range gives -Inf
 * (max) or 0 / (last - first + 1) (mean: NaN when first == last + 1) and label 1.  Rows are clamped to [0, n).
 * XM_EINVAL: E outside 1..64, P outside 1..E, n < 0, N < 0, an unknown agg (XM_AGG_PEAK included), a NULL tensor with
 * N > 0; N == 0: XM_OK. */
int xm_window_targets(const float *logits, int E, int n, const int *first, const int *last, int N, int agg, int P,
                      float *out, float *max_label, void *stream);
/* mcnExtraLayers dagnn.ErrorStats bookkeeping (emoVoxZoo.m:165-169, read by extractStats,
 * run_distillation.m:186-207): for every sample n with label c = labels[n] (1-based):
 * population[c-1] += 1, correct[c-1] += (argmax_c x(:, n) == c).  ACCUMULATES into the two
 * C-element device arrays (zero them at the start of an epoch); first maximum wins ties. */
int xm_class_stats(const float *x, const float *labels, int C, int N, float *correct,
                   float *population, void *stream);
/* fetch_emovoxceleb_imdb.m:176-193: rgb2gray -> replicate x3 -> minus averageImage(c).
 * avg3 is a HOST pointer to the three per-channel means (meta.normalization.averageImage). */
int xm_normalize_face(const float *rgb, int H, int W, int N, const float *avg3, float *out,
                      void *stream);
/* getImageBatch from decoded frames (fetch_emovoxceleb_imdb.m:152-193): centred crop of relative size
 * `crop` (1/1.6), bilinear resample to Ho x Wo (pixel-centre aligned, edge clamped, rounded to uint8 as
 * `uint8(data{1})` does), rgb2gray, replicate x3, minus averageImage -- one pass.
 * src: Hin x Win x 3 x N with values 0..255 (single holding the decoded uint8); avg3: HOST pointer. */
int xm_crop_resize_face(const float *src, int Hin, int Win, int N, float crop, int Ho, int Wo,
                        const float *avg3, float *out, void *stream);

/* ---- mnrfit / mnrval (Statistics Toolbox; external/run_cross_val.m:138-145, external/emo_benchmarks.m:90-100) --------
 * Extensions, not MatConvNet operators.  G independent problems per call, one workgroup each; every sum runs in a fixed
 * order without float atomics, so a problem's outputs are the same bits whatever G is and whatever else shares the call.
 * X is p x n single with each sample's features contiguous (the 1 x 1 x p x n output of xm_aggregate_logits), labels n
 * int32 in 1..k, problem g owns rows[offsets[g] .. offsets[g+1]) (int32, 1-based sample indices; nnz = size of rows).
 * B (per problem (p+1) x (k-1) doubles, column-major, problems one after another) is MATLAB's nominal model
 *     log(pi_j / pi_k) = B(1, j) + x * B(2:end, j),  j < k  (the last category is the reference),
 * i.e. what mnrfit returns and mnrval takes.  D = (p+1)(k-1) <= 64, p >= 1, k >= 2, else XM_EINVAL before any launch.
 *
 * coefficients = mnrfit(double(X(:, rows)'), labels(rows)): Newton-Raphson from B = 0 in fp64; the information matrix
 * is accumulated per entry in row order and solved by Cholesky in LDS; a step whose log-likelihood is lower than the
 * current one is halved (at most 30 times); stop when a step that raised it has max|dB| <= tol_x * max(1, max|B|)
 * (statset('mnrfit'): 100 iterations, 1e-6) or after max_iter iterations.  Per problem: B, deviance = -2 log-likelihood, the iteration count
 * and status_out = XM_MNR_CONVERGED | XM_MNR_ITERLIMIT (separable data ends here with finite B) | XM_MNR_NOTPD (a
 * Cholesky pivot <= 1e-14 x the largest diagonal entry; B = the last accepted iterate) | XM_MNR_BADINPUT (a label
 * outside 1..k, a row outside 1..n, bad offsets, or a class absent from the training rows -- where mnrfit would drop
 * the category and shift the columns; B = 0, deviance NaN). */
int xm_mnrfit(const float *x, int p, int n, const int *labels, int k, const int *offsets, const int *rows, int nnz,
              int G, int max_iter, double tol_x, double *b_out, double *dev_out, int *iters_out, int *status_out,
              void *stream);
/* preds = mnrval(B, double(X(:, rows)')); [~, cls] = max(preds, [], 2); confusionmat(labels, cls, 'Order', 1:k).
 * probs_out (optional): k doubles per listed row, contiguous (the transpose of mnrval's n x k), in the order of rows;
 * preds_out: the 1-based class per row, the first maximum winning ties; conf_out (optional, with labels): k x k int32
 * per problem, column-major, (true label, predicted class), exact counts, overwritten.  A row index outside 1..n gets
 * NaN probabilities and class 0 and is not counted; neither is a label outside 1..k. */
int xm_mnrval(const double *b, const float *x, int p, int n, int k, const int *offsets, const int *rows, int nnz, int G,
              const int *labels, double *probs_out, int *preds_out, int *conf_out, void *stream);

/* ---- vl_roc / histcounts (vlfeat [EXT]; emoVoxCeleb/student_stats.m:65-68,97-125, emoVoxCeleb/teacher_stats.m:28-29,57)
 * Extensions, not MatConvNet operators (ABI 109).
 *
 * xm_roc: [~, ~, info] = vl_roc(labels, scores) with vlfeat's default options for G x E problems in one call.
 * scores is n x E single, column-major (column c = the scores of emotion c + 1); cls holds n int32 classes (1-based, the
 * teacher's label of each row); set g owns rows[offsets[g] .. offsets[g+1]) (int32, 1-based rows, nnz = size of rows,
 * as xm_mnrfit).  Problem (g, c): the rows of set g, label +1 where cls == c + 1 and -1 elsewhere, score scores[row, c].
 *   - p / n = the number of +1 / -1 labels over ALL rows of the set;
 *   - the rows are ranked by score, descending and stable: equal scores (-0.0 == +0.0) keep the order of `rows`, as
 *     MATLAB's sort(..., 'descend'); ties are not grouped, every row is a curve point;
 *   - rows scoring -Inf are never retrieved: they count in p / n, the curve stops before them
 *     (retrieved = the number of rows with score > -Inf);
 *   - tp = [0 cumsum(label > 0)], fp = [0 cumsum(label < 0)] over the retrieved rows, tpr = tp / max(p, 1e-10),
 *     fpr = fp / max(n, 1e-10), auc = the trapezoid sum of tpr over fpr.  A positive step adds no area and a negative
 *     step adds tp / (p n), so with S = sum over retrieved negatives of the positives ranked before them (an exact
 *     64-bit integer)  auc = (double)S / ((double)p * (double)n), one division; auc = 0 when p == 0 or n == 0.
 * Outputs, all overwritten: auc (E x G doubles, column-major: entry c + E g), area (E x G, S), counts (3 x E x G:
 * p, n, retrieved), status (E x G): XM_ROC_OK; XM_ROC_NAN = a NaN score in the problem (auc = NaN, the other problems
 * of the call are unaffected); XM_ROC_BADINPUT = a row outside 1..n in the set, or offsets that are not 0 <= ascending
 * <= nnz (then every problem; auc = NaN; no row is read through a bad index).  A host that has the index sets checks
 * them before the call (vl.roc does).  An empty set gives p = n = 0, auc = 0, XM_ROC_OK.
 * perm_out / tp_out (optional, both or neither; E x nnz int32 each, entry c nnz + offsets[g] + i): the row (1-based)
 * ranked i-th in problem (g, c) and the positives among the first i + 1 rows, over all rows of the set, not only the
 * retrieved ones; fp = i + 1 - tp.  With `retrieved` this is the whole curve.  For a problem whose status is not
 * XM_ROC_OK they hold a permutation of the set in an unspecified order.
 * Only integers are accumulated (integer atomics), there are no float atomics: every output bit is a function of the
 * problem's own rows -- independent of G, of the order of the sets, of the launch shape and of scheduling.  A problem is
 * spread over workgroups of 2048 entries; the number of launches (xm_roc_launches(): four 8-bit passes of a stable
 * radix sort, three launches each, plus six) does not depend on n, nnz, G or E.  Scratch (16 nnz E bytes plus the tile
 * tables) comes from the stream's workspace.  XM_EINVAL before any device work: E < 1, G < 0, n < 1, nnz < 0, a NULL
 * required pointer, one of perm_out / tp_out without the other.  Supported: nnz E < 2^31, E <= 65535, 3 E G < 2^31;
 * XM_ENOTSUP beyond. */
int xm_roc(const float *scores, int n, int E, const int *cls, const int *offsets, const int *rows, int nnz, int G,
           double *auc, long long *area, int *counts, int *status, int *perm_out, int *tp_out, void *stream);
int xm_roc_launches(void);
/* xm_roc_geometry (ABI 126): host only, the constants of the kernels; a NULL pointer is skipped.  tile: entries of a
 * problem one workgroup owns; wave_span: consecutive entries of a tile one wave ranks and scans (tile / wave_span waves);
 * threads: the workgroup size, which is also the number of threads that share the per-call set loop and the per-problem
 * tile scan; hist_classes_max: the largest E xm_label_hist takes. */
int xm_roc_geometry(int *tile, int *wave_span, int *threads, int *hist_classes_max);
/* histcounts(labels, 0.5:E+0.5) of [~, labels] = max(x, [], 2): the first maximum per sample (as xm_max_label) counted
 * into E 64-bit integer bins, one launch, exact in any order.  x holds N samples of E logits: sample_major = 0 is
 * E x N (a sample's logits contiguous, the 1 x 1 x E x N layout of xm_max_label), sample_major = 1 is N x E column-major
 * (vertcat(imdb.wavLogits{:})).  ADDS to bins (zero them before the first block of a stream of blocks).  E <= 4096. */
int xm_label_hist(const float *x, int N, int E, int sample_major, long long *bins, void *stream);

/* ---- teacher logits per track (emoVoxCeleb/fetch_emovoxceleb_imdb.m:119-148, emoVoxCeleb/sample_audio.m:69-74) -------
 * Extensions, not MatConvNet operators (ABI 110).  Index sets as xm_roc / xm_mnrfit: `offsets` holds G + 1 0-based
 * positions, `rows` 1-based rows.  No float atomics, every output bit is a function of the inputs alone, the number of
 * launches does not depend on the sizes, scratch comes from the stream's workspace.  XM_EINVAL (a NULL required pointer,
 * a negative count) and XM_ENOTSUP (a size past 2^31) are returned before any device work.
 *
 * xm_group_rows: wavLogits{ii} = logits(denseFramesWavIds == images.id(ii), :) for all ii at once
 * (fetch_emovoxceleb_imdb.m:140-148), as index sets.  ids: the int32 wav id of each of n frames, in any order; keys:
 * T DISTINCT ids in 0 < key <= key_max (a key outside that range claims nothing; duplicate keys are the caller's
 * error -- which of them receives the rows is unspecified --, the host wrapper refuses them).  Group t receives the
 * 1-based rows i + 1 with ids[i] == keys[t] in ascending order (the grouping is stable):
 *   offsets_out (T + 1 int32), rows_out (n int32: the first nnz entries are the groups one after another, the rest is
 *   0), nnz_out (one int32: the number of rows kept = offsets_out[T]).
 * A row whose id is in no key is dropped: the "unclaimed" id 0, the tracks past `limit`, ids <= 0 or > key_max.
 * A table of key_max + 1 slots maps id -> group, the rows are sorted by group with the stable 8-bit LSD radix passes of
 * xm_roc (four passes, dropped rows carry the largest key), the offsets are lower bounds in the sorted keys.  16 launches
 * whatever n, T and key_max are (one when n == 0 or T == 0).  Scratch: 16 n + 4 (key_max + 1) bytes plus the tile
 * histograms.  Supported: key_max < 2^28; XM_ENOTSUP beyond. */
int xm_group_rows(const int *ids, int n, const int *keys, int T, int key_max, int *offsets_out, int *rows_out,
                  int *nnz_out, void *stream);
/* The `out'` store of fetch_emovoxceleb_imdb.m:130-131 and its inverse: E-wide rows between the 1 x 1 x E x n layout a
 * network emits (`packed`, sample i at packed[E i .. E i + E)) and an F x E column-major matrix (`mat`).  Row i of the
 * packed side is matrix row rows[i] (1-based) when rows != NULL, else row0 + i + 1 (row0 0-based).
 *   xm_gather_rows:   packed[e + E i] = mat[row + F e];  a row outside 1..F gives NaN
 *   xm_scatter_rows:  mat[row + F e] = packed[e + E i];  a row outside 1..F is skipped; the other rows of mat are left
 *                     as they were; the listed rows must be distinct
 * One launch each.  XM_EINVAL: n < 0, E < 1, F < 1, row0 < 0, a NULL tensor (n > 0); without a row list also
 * row0 + n > F.  XM_ENOTSUP: F E >= 2^31 or n E >= 2^31. */
int xm_gather_rows(const float *mat, int F, int E, int row0, const int *rows, int n, float *packed, void *stream);
int xm_scatter_rows(const float *packed, int n, int E, float *mat, int F, int row0, const int *rows, void *stream);
/* sample_audio.m:69-74 for all tracks in one launch.  logits: F x E column-major; group t = the rows
 * rows[offsets[t] .. offsets[t+1]) (1-based), or, with rows == NULL, the contiguous rows offsets[t] + 1 .. offsets[t+1].
 *   [~, m] = max(x(:)); [frameIdx, tag] = ind2sub(size(x), m)  -> frame_idx[t], tag[t] (int32, both 1-based; frame_idx is
 *                        the position within the group, not the matrix row)
 *   max(x, [], 1)       -> maxed, 1 x 1 x E x T
 * Ties go to the first entry in column-major order: lowest emotion, then lowest position.  NaN as XM_AGG_PEAK /
 * XM_AGG_MAX of xm_aggregate_logits: a NaN never wins (v > best is false) and fmaxf drops it, so a group without any
 * entry > -Inf gives frame_idx = tag = 1 and a column of NaN gives -Inf.  An empty group (or offsets that descend)
 * gives 0, 0 and -Inf.  A listed row outside 1..F is passed over like a NaN; contiguous groups are cut to 0..F.  With a
 * row list the caller guarantees offsets[T] <= the length of rows (the host wrapper checks).
 * One wave per group: lane l reads positions l, l + 64, ... of every column (consecutive lanes read consecutive floats
 * when the rows are contiguous), the column maxima are reduced with wave shuffles and the peak with a shuffle reduction
 * on (value, then lower emotion, then lower position).  Comparisons only: the result does not depend on the order of
 * the reduction.  One launch.  XM_EINVAL: F < 1, E < 1, T < 0, a NULL tensor (T > 0).  XM_ENOTSUP: F E or T E >= 2^31. */
int xm_track_peaks(const float *logits, int F, int E, const int *offsets, const int *rows, int T, int *frame_idx,
                   int *tag, float *maxed, void *stream);

/* ---- vl_nnaffinegrid / vl_nnbilinearsampler  (MatConvNet; getBatchFerPlus, teacher/ferplus_baselines.m:209-213) ------
 * PARITY UNPINNED: MatConvNet is not available to compare against; the formulas below restate its documented
 * behaviour.  FINITE INPUTS: results are specified for finite A, X, GRID, DY; a non-finite grid
 * coordinate samples nothing (output 0), as a coordinate far outside the image does.
 *
 * GRID = vl_nnaffinegrid(A, [Ho Wo]):  A is 1 x 1 x 6 x N (c1..c6 per sample), GRID is 2 x Ho x Wo x N with
 *   GRID(1, i, j, n) = c1 y_i + c3 x_j + c5  (the Y coordinate),  GRID(2, i, j, n) = c2 y_i + c4 x_j + c6  (X),
 *   y = linspace(-1, 1, Ho), x = linspace(-1, 1, Wo), linspace(-1, 1, 1) = 1 as in MATLAB: A reshaped column-major to
 *   2 x 3 is [c1 c3 c5; c2 c4 c6] applied to (y, x, 1).
 * DA = vl_nnaffinegrid(A, [Ho Wo], DGRID): dA (1 x 1 x 6 x N) = sums over Ho x Wo of [dG1 y, dG2 y, dG1 x, dG2 x, dG1,
 *   dG2]; wave-shuffle reductions in a fixed order, no atomics (fixed bits).  A itself is not read. */
int xm_nnaffinegrid(const float *A, int N, int Ho, int Wo, float *grid, void *stream);
int xm_nnaffinegrid_backward(const float *dgrid, int N, int Ho, int Wo, float *dA, void *stream);
/* Y = vl_nnbilinearsampler(X, GRID):  X is H x W x C x N, GRID 2 x Ho x Wo x No with No = k N (k >= 1 integer, else
 * XM_EINVAL), Y is Ho x Wo x C x No; output image m (0-based) reads input image floor(m / k).
 *   py = (gy + 1)(H - 1) / 2, px = (gx + 1)(W - 1) / 2 (in double from the fp32 grid value; a position within
 *   (H - 1) 2^-25 resp. (W - 1) 2^-25 of an integer is that integer, so that an identity grid returns X bit for bit);
 *   sy = floor(py), sx = floor(px), wy = py - sy, wx = px - sx;
 *   Y = sum over a, b in {0, 1} of (a ? wy : 1 - wy)(b ? wx : 1 - wx) X(sy + a, sx + b); a tap outside the image adds 0
 *   (zero padding, no clamping).  The grid is read once per output pixel for all C channels.
 * [DX, DGRID] = vl_nnbilinearsampler(X, GRID, DY):  either output may be NULL (not computed).
 *   DX (H x W x C x N, overwritten) receives w DY in each tap through no-return float atomic adds: overlapping grids add
 *   into the same pixels, so THE LAST BITS OF DX DEPEND ON SCHEDULING (see the determinism note of the tile table).
 *   DGRID (2 x Ho x Wo x No) is the derivative of the formula above with sy, sx held fixed (the one-sided derivative
 *   from above at integer coordinates), summed over C inside one thread: fixed bits. */
int xm_nnbilinearsampler(const float *x, int H, int W, int C, int N, const float *grid, int Ho, int Wo, int No,
                         float *y, void *stream);
int xm_nnbilinearsampler_backward(const float *x, int H, int W, int C, int N, const float *grid, int Ho, int Wo,
                                  int No, const float *dy, float *dx, float *dgrid, void *stream);
/* Extension: the whole data path of getBatchFerPlus (ferplus_baselines.m:182-213) in one launch -- grey H x W x 1 x N
 * (single, 0..255) -> fliplr where flip[n] != 0 (device int array of N, NULL = none) -> replicate x3 minus averageImage
 * (avg3: HOST pointer, as xm_crop_resize_face) -> affine grid of A (device, 1 x 1 x 6 x N) at Ho x Wo -> bilinear
 * sampler; out is Ho x Wo x 3 x N.  The normalisation comes BEFORE the zero padding, as in the reference: from the
 * in-bounds taps S = sum w g and Omega = sum w, out_c = S - avg_c Omega.  Neither the RGB tensor nor the grid is ever
 * written.  Equal to xm_nnaffinegrid + xm_nnbilinearsampler on the normalised image up to fp32 rounding (the grid
 * coordinates are the same bits). */
int xm_ferplus_batch(const float *grey, int H, int W, int N, const int *flip, const float *A, int Ho, int Wo,
                     const float *avg3, float *out, void *stream);

/* vl_imreadjpeg(paths, 'Pack', 'Interpolation', 'bilinear', 'CropSize', 1/1.6, 'CropLocation', 'center', 'Resize',
 * imageSize) of fetch_emovoxceleb_imdb.m:160-172 and compute_visual_feats.m:130-143 for a batch of files, decoded on the
 * device (ABI 113).  Supported: baseline sequential DCT (SOF0), 8-bit, Huffman, one interleaved scan; one component
 * (grey; R = G = B = Y) or three (YCbCr) with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1; any DQT / DHT tables with
 * 8-bit quantiser entries; restart intervals; 1 x 1 up to 4096 x 4096 per image and fewer than 2^31 coefficients and
 * pixel values per batch.  The arithmetic is libjpeg's default integer path (ISLOW IDCT with 13-bit constants and
 * PASS1_BITS 2, "fancy" triangle upsampling for h2v1 / h2v2 -- replication where the chroma plane has one or two
 * columns --, 16-bit fixed-point YCbCr -> RGB with range limiting): results are equal to libjpeg's, not close.  There
 * is no host decode.
 *
 * xm_jpeg_plan: host only, no device call (usable without a GPU).  File i is bytes[offsets[i] .. offsets[i + 1]).
 *   desc    N rows of XM_JPEG_DESC int64: 0, 1 byte range of the entropy data in `bytes`; 2 H; 3 W; 4 components (1 | 3);
 *           5, 6 luma sampling h, v; 7 restart interval in MCUs (0 = none); 8, 9 MCUs across, down; 10-12 quantiser
 *           table slot per component; 13-15 DC and 16-18 AC Huffman table slot per component (a grey image repeats
 *           component 0); 19 first coefficient (int16 elements), 20 first plane byte, 21 first pixel value (floats) of
 *           the image in the ragged device buffers; 22 first lane, 23 number of lanes
 *   lanes   XM_JPEG_LANE int64 per restart interval (one per image without DRI): image, byte range, first MCU
 *   tables  nq quantiser tables of XM_JPEG_QT_BYTES (64 uint16, row-major) then nh Huffman tables of XM_JPEG_HT_BYTES
 *           (lookahead uint16[256] = code length << 8 | symbol for codes of up to 8 bits, symbols uint8[256],
 *           maxcode int32[17], valoff int32[17] as jpeg_make_d_derived_tbl, zero padding); equal tables share a slot
 *   sizes   XM_JPEG_SIZES int64: table bytes, nq, nh, coefficients, plane bytes, pixel values, lanes, N
 * XM_ENOTSUP (valid file this build does not decode: progressive, arithmetic, 12-bit, multi-scan, 4 components, Adobe
 * transform 0, other sampling factors, 16-bit quantiser tables, larger than the limit) and XM_EINVAL (malformed: no
 * SOI, cut inside its headers, bad segment, missing table) name the index of the file.  A file whose entropy data is
 * cut short is planned; decoding it reports XM_JPEG_TRUNCATED.  XM_ENOMEM: lanes_cap / tables_cap too small, `sizes`
 * holds what is needed.  XM_EINVAL: NULL or negative arguments.
 *
 * xm_jpeg_decode_batch: device.  bytes (16-byte aligned, allocated up to the next multiple of 16 past nbytes), desc,
 * lanes and tables (16-byte aligned) are the uploaded outputs of the plan.  pixels (optional): pixel_floats single,
 * image i as H x W x 3 with values 0..255 in MATLAB layout at desc[i][21] -- vl_imreadjpeg without 'Resize'.  faces
 * (optional): Ho x Wo x 3 x N, per image bit for bit xm_crop_resize_face of its pixels (centre crop of relative size
 * `crop`, bilinear resize, uint8 rounding, rgb2gray, x3, minus avg3 -- HOST pointer; avg3 == NULL: the resized R, G, B
 * instead).  status: N int32, a bit set of XM_JPEG_TRUNCATED (bits past the end of the image's entropy data were used;
 * the reader yields zeros there) and XM_JPEG_BADCODE (an invalid Huffman code or a run past coefficient 63 ended a
 * lane).  Four launches, five with faces, whatever N and the sizes are; no synchronisation.  Every read of file bytes
 * is clamped to the image's byte range and every coefficient write to the image's blocks by the indexing itself. */
enum { XM_JPEG_OK = 0, XM_JPEG_TRUNCATED = 1, XM_JPEG_BADCODE = 2 };
enum { XM_JPEG_DESC = 24, XM_JPEG_LANE = 4, XM_JPEG_QT_BYTES = 128, XM_JPEG_HT_BYTES = 1024, XM_JPEG_SIZES = 8 };
int xm_jpeg_plan(const unsigned char *bytes, const long long *offsets, int N, long long *desc, long long *lanes,
                 long long lanes_cap, unsigned char *tables, long long tables_cap, long long *sizes);
int xm_jpeg_decode_batch(const unsigned char *bytes, long long nbytes, const long long *desc, int N, const long long *lanes,
                         int nlanes, const unsigned char *tables, int nq, int nh, long long coef_elems,
                         long long plane_bytes, long long pixel_floats, float *pixels, float *faces, float crop, int Ho,
                         int Wo, const float *avg3, int *status, void *stream);

/* xm_jpeg_decode_batch with a segment-parallel entropy stage (ABI 115): what a file without restart markers needs, whose
 * one lane is otherwise one serial decoder.  The arguments up to `status` are those of xm_jpeg_decode_batch and mean
 * the same; the plan, its descriptors and its lanes are the same.  Segment i of a lane is the raw bytes
 * [begin + i * seg_bytes, min(begin + (i + 1) * seg_bytes, end)) of the lane's range.  One workgroup owns a lane, one
 * thread a segment: every thread decodes its segment from a guessed state, takes its predecessor's exit state (bit
 * position, block inside the MCU, coefficient index) as its entry until no exit changes -- that fixed point is the
 * sequential decode --, and decodes once more to write.  A lane of more segments than xm_jpeg_split_geometry's
 * segments_per_pass runs in consecutive passes inside its workgroup.  seg_bytes: a multiple of 16 in 16 .. 65536, else
 * XM_EINVAL before any device call.  rounds (optional, device): nlanes int32, the decode rounds a lane took, the first
 * one included, summed over its passes (1 <= rounds <= segments).  Pixels, faces and status are bit for bit those of
 * xm_jpeg_decode_batch for every input, truncated and corrupted files included.  The number of launches is that of
 * xm_jpeg_decode_batch and xm_jpeg_split_geometry reports it (with faces); no synchronisation.
 * xm_jpeg_split_geometry: host only, no device call. */
int xm_jpeg_decode_batch_split(const unsigned char *bytes, long long nbytes, const long long *desc, int N,
                               const long long *lanes, int nlanes, const unsigned char *tables, int nq, int nh,
                               long long coef_elems, long long plane_bytes, long long pixel_floats, float *pixels,
                               float *faces, float crop, int Ho, int Wo, const float *avg3, int *status, int seg_bytes,
                               int *rounds, void *stream);
int xm_jpeg_split_geometry(int *segments_per_pass, int *launches);

/* Progressive files in vl_imreadjpeg (ABI 120): MatConvNet's vl_imreadjpeg is libjpeg and reads a progressive file as it
 * reads a baseline one; xm_jpeg_plan refuses it, and stays as it is.  This pair is the opt-in that accepts what
 * xm_jpeg_plan accepts and, in addition, SOF2: 8-bit, Huffman, 1 or 3 components within the same sampling limits, any
 * scan script that satisfies T.81 G.1.1.1.1 -- Ss <= Se <= 63; Ss == 0 implies Se == 0; an AC scan has one component;
 * Ah == 0, or Ah == Al + 1 with Ah the Al of the previous scan of every coefficient of the band; Al <= 13 -- and sends
 * no coefficient first twice.  A violation is XM_EINVAL with the file's index and the scan's number.  Deviation from
 * libjpeg: libjpeg only warns about a bogus progression and decodes on; here the refinement of a coefficient that no
 * earlier scan sent, and any other violation, refuses the batch.  Still XM_ENOTSUP, with the file's index: SOF1 and SOF3
 * to SOF15 (extended, lossless, hierarchical, arithmetic), 12-bit samples, 4 components, multi-scan SOF0, more than
 * XM_JPEG_MAX_SCANS scans in a file.  A file that ends after any of its scans (EOI, or the end of the bytes) is valid
 * and decodes to what the coefficients sent so far give; a component's quantiser table is the one that stood at the
 * file's first scan.  Such a file gets what libjpeg, and with it vl_imreadjpeg, gives it: while one of the first ten
 * coefficients (zigzag order) of a component has not arrived in full, libjpeg's block smoothing estimates the ones
 * that are still zero from the DC values of the 5 x 5 blocks around (jdcoefct.c, the form of libjpeg-turbo 2.1 and
 * later), so the pixels equal libjpeg's there too.
 *
 * xm_jpeg_plan_prog: host only, no device call (usable without a GPU).  bytes, offsets, desc, tables as xm_jpeg_plan;
 * for a baseline file the descriptor row and the table slots are those of xm_jpeg_plan; for SOF2 columns 13-18 mean
 * nothing, 0 .. 1 span the entropy data of all scans, 7 is the restart interval at the first scan, 22, 23 the lanes
 * of all scans -- but in a file that is smoothed column 13 + c is XM_JPEG_SMOOTH plus one nibble per coefficient 0 .. 9
 * of component c, nibble z = 1 + the Al the coefficient stands at, 0 = never sent.
 *   scans   XM_JPEG_SCAN int64 per (image, scan), in file order: 0 image; 1 components in the scan; 2-4 their index in
 *           the frame (-1: none); 5 Ss; 6 Se; 7 Ah; 8 Al; 9-11 DC and 12-14 AC Huffman table slot per scan component, as
 *           DHT stood at this scan (a progressive file redefines its tables between scans; 0 where the kind of scan
 *           reads none); 15, 16 byte range of the entropy data; 17, 18 the raster, in MCUs, across and down: the
 *           frame's MCUs for a scan of several components, else the component's own blocks ceil(ceil(W * h / hmax) /
 *           8) x ceil(ceil(H * v / vmax) / 8), each block one MCU, not the MCU-padded count (the coefficient buffer
 *           keeps its padded pitch); 19 level: 0 if no earlier scan of the image sends a (component, coefficient) it
 *           sends, else 1 + the largest level among those that do -- scans of one level write disjoint coefficients;
 *           20 first lane, 21 lanes; 22 restart interval in MCUs at this scan; 23 kind (XM_JPEG_SCAN_*)
 *   lanes   XM_JPEG_LANE int64 per (scan, restart interval): scan row, byte range, first MCU
 *   sizes   XM_JPEG_PROG_SIZES int64: the eight of xm_jpeg_plan, then 8 scans, 9 levels (at most XM_JPEG_MAX_LEVELS:
 *           every scan of a coefficient lowers its Al by one), 10 whether a file of the batch is smoothed
 * XM_ENOMEM: scans_cap / lanes_cap / tables_cap too small, `sizes` holds what is needed.
 *
 * xm_jpeg_decode_batch_prog: device.  The arguments up to `status` are those of xm_jpeg_decode_batch, from the plan
 * above; scans (device, 8-byte aligned), nscans, levels and smooth are the plan's.  Launches: clear; the progressive entropy
 * kernel once per level (one lane per (scan, restart interval), DC predictors and the end-of-band run zero at the
 * start of each; DC first / refinement, AC first / refinement as T.81 G.1.2, the one scan of a baseline file as
 * xm_jpeg_decode_batch decodes it); with `smooth` the two smoothing kernels; then IDCT, colour and faces exactly as
 * xm_jpeg_decode_batch: 4 + levels launches, two more with smoothing, one more with faces, whatever N and the sizes
 * are; no synchronisation.  Coefficients are read and written as int16
 * only.  status as xm_jpeg_decode_batch, ORed over the image's lanes; XM_JPEG_BADCODE also covers a run or an
 * end-of-band run that leaves the band or the restart interval.  Baseline files in the batch give pixels, faces and
 * status bit for bit those of xm_jpeg_decode_batch. */
enum { XM_JPEG_SCAN = 24, XM_JPEG_PROG_SIZES = 11, XM_JPEG_MAX_SCANS = 256, XM_JPEG_MAX_LEVELS = 14 };
#define XM_JPEG_SMOOTH (1LL << 40)
enum { XM_JPEG_SCAN_SEQ = 0, XM_JPEG_SCAN_DC_FIRST = 1, XM_JPEG_SCAN_DC_REFINE = 2, XM_JPEG_SCAN_AC_FIRST = 3,
       XM_JPEG_SCAN_AC_REFINE = 4 };
int xm_jpeg_plan_prog(const unsigned char *bytes, const long long *offsets, int N, long long *desc, long long *scans,
                      long long scans_cap, long long *lanes, long long lanes_cap, unsigned char *tables, long long tables_cap,
                      long long *sizes);
int xm_jpeg_decode_batch_prog(const unsigned char *bytes, long long nbytes, const long long *desc, int N,
                              const long long *lanes, int nlanes, const unsigned char *tables, int nq, int nh,
                              long long coef_elems, long long plane_bytes, long long pixel_floats, float *pixels, float *faces,
                              float crop, int Ho, int Wo, const float *avg3, int *status, const long long *scans, int nscans,
                              int levels, int smooth, void *stream);

/* audioinfo / audioread of a batch of WAV files, decoded on the device into the waveform bank that xm_wav_batch and
 * xm_spec_bucket_batch read (ABI 114): info = audioinfo(audfile) -> TotalSamples, SampleRate (getBatchEmoVoxCeleb.m:79),
 * audioread(audfile, [wr wend]) and whole files (:97-117), the noise files %02d.wav (:126), and [z, fs] = audioread of
 * compute_audio_feats.m:173-175 with its assert(size(z,2) <= 2) and z(:,1).  There is no host decode.
 *
 * xm_wav_plan: host only, no device call (usable without a GPU).  File i is bytes[offsets[i] .. offsets[i + 1]).
 *   ranges   optional N x 2 int64, 1-based inclusive [first last] as audioread(file, [a b]); last == -1: to the end
 *   channel  -1: every channel; c >= 0: channel c only (z(:, c + 1))
 *   out_base first float of the batch in the bank (chunked calls fill one bank)
 *   desc     N rows of XM_WAV_DESC int64: 0, 1 byte range of the sample data in `bytes`, clamped to the file; 2 SampleRate;
 *            3 NumChannels; 4 BitsPerSample; 5 format (XM_WAV_U8 .. XM_WAV_F64); 6 TotalSamples = floor(data bytes / block
 *            align) frames; 7 first frame decoded (0-based); 8 frames decoded; 9 channels written; 10 the channel
 *            selector; 11 first output float (out_base + the floats of the files before); 12 status (XM_WAV_TRUNCATED:
 *            the data chunk claimed more bytes than the file holds); 13 block align; 14, 15 zero (xm_wav_plan_fs: p, q)
 *   sizes    XM_WAV_SIZES int64: output floats of the batch, N
 * Accepted: RIFF ... WAVE, chunks walked with the pad byte after odd sizes, unknown chunks (LIST, fact, bext ...) skipped
 * before and after `data`, `fmt ` before `data`, the first `data` chunk; format tag 1 (PCM 8 / 16 / 24 / 32 bits), 3
 * (IEEE float 32 / 64) and 0xFFFE (extensible) whose SubFormat is one of the two and whose valid bits equal the container
 * bits; block align == channels x bits / 8; 1 .. 64 channels.  A data size past the end of the file (0xFFFFFFFF of a
 * streamed writer) is clamped and flagged, a trailing partial frame is dropped, a file of 0 frames yields 0 floats.
 * XM_ENOTSUP (valid file this build does not decode: RF64 / BW64, RIFX, A-law, mu-law, ADPCM, MPEG and every other tag,
 * valid bits unlike the container bits, any other bit depth, more than 64 channels) and XM_EINVAL (malformed: no RIFF /
 * WAVE, cut inside its headers, an fmt chunk shorter than 16 bytes -- 40 when extensible --, data before fmt, no data
 * chunk, a wrong block align, zero channels or rate; a range outside 1 .. TotalSamples or with first > last; a channel
 * the file does not have) name the index of the file.  XM_EINVAL: NULL or negative arguments.
 *
 * xm_wav_decode_batch: device, ONE launch whatever N, the formats and the lengths are; no atomics, no workspace, no
 * tuning entries, no synchronisation.  bytes (16-byte aligned, allocated up to the next multiple of 16 past nbytes) and
 * desc (8-byte aligned) are the uploaded file bytes and plan.  File i is written at out + desc[i][11] as a frames x
 * channels-written matrix in MATLAB layout (channel c at + c * frames); every float of the batch is written exactly
 * once and nothing outside [0, out_floats).  Values are single(audioread's double): U8 (v - 128) / 128; S16 v / 2^15;
 * S24 v / 2^23; S32 float(v) * 2^-31 with the conversion rounding to nearest even; F32 the bits unchanged (NaN payloads
 * included); F64 rounded to nearest even.  Every byte read is clamped to the file's data range by the indexing itself.
 * N == 0: XM_OK.  XM_EINVAL: a negative argument, a NULL or misaligned pointer with N > 0. */
enum { XM_WAV_U8 = 0, XM_WAV_S16 = 1, XM_WAV_S24 = 2, XM_WAV_S32 = 3, XM_WAV_F32 = 4, XM_WAV_F64 = 5 };
enum { XM_WAV_OK = 0, XM_WAV_TRUNCATED = 1 };
enum { XM_WAV_DESC = 16, XM_WAV_SIZES = 2 };
int xm_wav_plan(const unsigned char *bytes, const long long *offsets, int N, const long long *ranges, int channel,
                long long out_base, long long *desc, long long *sizes);
int xm_wav_decode_batch(const unsigned char *bytes, long long nbytes, const long long *desc, int N, float *out,
                        long long out_floats, void *stream);

/* WAV files of any rate resampled into the bank while they are decoded (ABI 122): [z, Fs] = audioread(f) followed by
 * z = resample(z(:, c), fs, Fs), what compute_audio_feats.m:173-175 and emo_benchmarks need for RML / eNTERFACE / AFEW
 * audio (22.05, 44.1, 48 kHz, often stereo) and upstream left to ffmpeg (getBatchEmoVoxCeleb.m:149).
 *
 * xm_wav_plan_fs: host only, no device call.  The parse, the refusals and the rows of xm_wav_plan, except that slots
 *   14, 15 hold p, q = fs / SampleRate reduced by their gcd (1, 1 when the file is at fs already) and that slot 11 and
 *   sizes[0] count OUTPUT floats: file i takes ceil(frames decoded * p / q) floats per channel written, a matrix of that
 *   many rows in MATLAB layout (channel c at + c * rows).  Slot 8 stays the SOURCE frames decoded.  `ranges` are in source
 *   frames, as in audioread(file, [a b]) followed by resample: samples outside the range count as zero, they are not the
 *   file's neighbouring samples.  XM_ENOTSUP naming the file's index when, after the reduction, max(p, q) > 2^20 (the
 *   limit of xm_wav_batch), q > 16 p or p > 16 q (these bound the tap loop, 20 max(p, q) / p + 1 taps per output, and
 *   the window of source frames a tile keeps in LDS).  XM_EINVAL: fs < 1, and whatever xm_wav_plan refuses.
 *
 * xm_wav_decode_resample_batch: device, at most TWO launches whatever N, the formats, the rates and the lengths are --
 *   one workgroup per file sums the filter's taps in fp64 for its gain, then one launch laid out by the output floats
 *   decodes each tile's source window into LDS once and runs the taps from there.  No atomics, no tuning entries, no
 *   synchronisation; the workspace holds the per-file gains only.  Arguments as xm_wav_decode_batch, with the rows of
 *   xm_wav_plan_fs.  Output j of a channel is gain * sum_k u(j q - k p) x[k] over the decoded frames k, the taps, their
 *   order (k descending) and the gain those of xm_wav_batch: the floats are bit for bit what xm_wav_batch returns for the
 *   descriptor {src, frames, fs, SampleRate, 0, 0} on the bank xm_wav_decode_batch fills, and do not depend on what else
 *   is in the batch or on where the tiles fall.  A file with p == q is copied: bit for bit xm_wav_decode_batch's floats.
 *   Every float of the batch is written exactly once and nothing outside [0, out_floats); every byte read is clamped to
 *   the file's data range, itself clamped to [0, nbytes); a row whose ratio is outside the plan's bounds is read as 1 / 1.
 *   N == 0: XM_OK.  XM_EINVAL, before any device call: a negative argument, a NULL or misaligned pointer with N > 0.
 *
 * xm_wav_resample_geometry: host only.  tile: the output floats of one tile (at ratio 1 a tile is one run; at other
 * ratios it is cut into runs whose source windows fit LDS); launches: what one decode-and-resample call enqueues. */
int xm_wav_plan_fs(const unsigned char *bytes, const long long *offsets, int N, const long long *ranges, int channel,
                   long long fs, long long out_base, long long *desc, long long *sizes);
int xm_wav_decode_resample_batch(const unsigned char *bytes, long long nbytes, const long long *desc, int N, float *out,
                                 long long out_floats, void *stream);
int xm_wav_resample_geometry(int *tile, int *launches);

/* The pixel column of the FER2013 CSV, decoded on the device into the image array of the FER+ imdb (ABI 116): what
 * imdb = getFerPlusImdb(opts.dataDir) (ferplus_baselines.m:103-110) reads before getBatchFerPlus gathers
 * imdb.images.data(:,:,:,batch) (:181), and the `dataDir` of benchmark_ferplus_models.m:15-17,46-54 ("the FER2013 and
 * FER2013+ datasets files (in csv format)").  A row of fer2013.csv is `emotion,pixels,Usage`; `pixels` holds the 48 x 48
 * image row-major as 2304 decimal numbers separated by blanks.  There is no host parse of the numbers.
 *
 * xm_pixcsv_plan: host only, no device call (usable without a GPU).  Finds the rows and their pixel fields.
 *   An optional UTF-8 byte order mark is skipped.  A line ends at LF or CRLF; a last line without a newline is a row;
 *   empty lines are skipped (they count in the line numbers).  Fields split at commas outside double quotes; a quote
 *   still open at the end of its line is an error.  If the first byte of the first non-empty line is not a digit the
 *   line is a header and the columns are found by name (one pair of enclosing quotes and blanks around the name are
 *   dropped): `pixels` is required, `emotion` and `Usage` are optional, other columns are ignored.  Without a header the
 *   columns are emotion,pixels,Usage.  A row needs at least as many fields as the header (3 without one).
 *   desc     N rows of XM_PIX_DESC int64: 0, 1 byte range of the pixel field in `bytes`, one pair of enclosing quotes
 *            stripped; 2 `emotion` as an integer (up to nine digits), -1 if the column or the value is absent or is not
 *            one; 3 usage code: 0 Training, 1 PublicTest, 2 PrivateTest, -1 anything else or no column; 4 1-based line
 *            number; 5 output image index, preset to the row's ordinal -- the caller may overwrite it, a negative value
 *            means "skip this row"; 6, 7 zero.  desc == NULL only counts (max_rows is then not looked at).
 *   sizes    XM_PIX_SIZES int64: the row count, the longest pixel field in bytes
 *   XM_EINVAL names the line: an unterminated quote, a row with fewer fields than the header, a header without a `pixels`
 *   column, more rows than max_rows.  XM_EINVAL: NULL sizes, NULL bytes with nbytes > 0, negative arguments.
 *
 * xm_pixcsv_decode_batch: device, ONE launch whatever N, the field lengths and their alignments are; no atomics, no
 * workspace, no tuning entries, no synchronisation.  bytes (16-byte aligned, allocated up to the next multiple of 16
 * past nbytes) holds the file or a part of it, desc (device, 8-byte aligned) the plan's rows with byte ranges relative
 * to `bytes`.  The k-th number of row i's field is written as a float at out + desc[i][5] * H * W + p, where
 * p = (k mod W) * H + k div W when transpose is 1 (the MATLAB H x W array of a row-major image) and p = k when it is 0.
 * Every float of every image that is not skipped is written exactly once; positions the field has no number for get 0;
 * numbers past H * W are counted and not written; nothing is written outside [0, out_floats).  Every byte read is
 * clamped to the field's range, itself clamped to [0, nbytes), by the indexing itself.
 *   A number is a maximal run of digits; every other byte separates.  status (device) is N x 2 int32: the count of
 *   numbers found and a flag word: XM_PIX_BADCHAR a byte that is not a digit, a space or a tab (it separates like a
 *   blank); XM_PIX_RANGE a run of more than three digits or a value above 255 -- that pixel is written as 255;
 *   XM_PIX_COUNT count != H * W; XM_PIX_NOFIT the image of the row's output index does not lie inside out_floats: no
 *   pixel of it is written and its count is 0 (the descriptor is device memory, so the kernel and not this entry point
 *   sees the index; vl.pixcsv_decode checks its host copy before the launch and raises).  Skipped rows get (0, 0).
 * N == 0: XM_OK.  XM_EINVAL: negative arguments; a transpose other than 0 / 1; with N > 0: NULL or misaligned pointers,
 * H * W <= 0, out_floats < H * W.
 *
 * xm_pixcsv_geometry: host only.  bytes_per_pass: a block walks a field in passes of that many bytes, starting at the
 * 16-byte boundary at or below the field's first byte, 16 bytes per thread; launches: what one decode call enqueues. */
enum { XM_PIX_DESC = 8, XM_PIX_SIZES = 2 };
enum { XM_PIX_BADCHAR = 1, XM_PIX_RANGE = 2, XM_PIX_COUNT = 4, XM_PIX_NOFIT = 8 };
int xm_pixcsv_plan(const unsigned char *bytes, long long nbytes, long long *desc, long long max_rows, long long *sizes);
int xm_pixcsv_decode_batch(const unsigned char *bytes, long long nbytes, const long long *desc, int N, int H, int W,
                           int transpose, float *out, long long out_floats, int *status, void *stream);
int xm_pixcsv_geometry(int *bytes_per_pass, int *launches);

/* ---- vl_nnnormalize [EXT: vl_nnnormalize.m, normalize_cpu]: cross-channel (local response) normalisation, the norm1 /
 * norm2 layers of the VGG-M / VGG-F / AlexNet family (dagnn.LRN) ----
 *   Y = vl_nnnormalize(X, PARAM), DZDX = vl_nnnormalize(X, PARAM, DZDY), PARAM = [N KAPPA ALPHA BETA], X H x W x C x S:
 *     m1 = floor((N - 1) / 2), m2 = N - 1 - m1, G(k) = [k - m1, k + m2] within the C channels
 *     L(i,j,k,s) = KAPPA + ALPHA * sum_{t in G(k)} X(i,j,t,s)^2,   Y = X .* L.^(-BETA)
 *     DX(k) = DZDY(k) L(k)^(-BETA) - 2 ALPHA BETA X(k) sum_{t: k in G(t)} DZDY(t) X(t) L(t)^(-BETA - 1)
 *   (the adjoint window is the mirrored one, [k - m2, k + m1]; for even N it differs from G(k)).
 * Any N >= 1 (N > 2 C included) and any H * W * C * S the address space holds.  y / dx may NOT alias x or dzdy: a block
 * reads channels that another block writes.  One launch, no scratch, no synchronisation.
 * XM_EINVAL before any device work: N < 1, a negative dimension, a NULL or aliasing pointer; a tensor with a zero
 * dimension is a no-op (XM_OK).
 * xm_nnnormalize_geometry: host only, the constants of the kernels.  pixels_per_block: pixels of one sample a block owns;
 * channels_per_pass: the shortest chunk of a split channel axis (planes with few pixels split it until the launch fills
 * the device; a chunk re-reads the m1 + m2 channels its windows need on each side); window_in_registers: the widest N
 * of the register arm, wider windows take the general arm.  A kernel without one of these notions reports 0. */
int xm_nnnormalize_forward(const float *x, int H, int W, int C, int S, int N, float kappa, float alpha, float beta,
                           float *y, void *stream);
int xm_nnnormalize_backward(const float *x, const float *dzdy, int H, int W, int C, int S, int N, float kappa,
                            float alpha, float beta, float *dx, void *stream);
int xm_nnnormalize_geometry(int *pixels_per_block, int *channels_per_pass, int *window_in_registers);

/* ---- vl_imreadjpeg's crop, flip, filter and colour options (ABI 125) [EXT: vl_imreadjpeg; its sources are not at hand, so
 * the definitions of DESIGN section 24 are the specification] ----
 * One stage behind the JPEG decoders: it reads the ragged `pixels` buffer they write (image n: H x W x 3, 0..255, MATLAB
 * layout) and writes single outputs, never rounded to uint8.
 *
 * xm_imread_plan: host only, no device call (usable without a GPU).
 *   hw      N x 3 int64: H, W, offset of the image's pixels in `pixels` (floats)
 *   opts    XM_IMREAD_OPTS doubles: 0 Resize mode (0 none: the output has the image's size; 1 [Ho Wo]; 2 scalar S: the
 *           shorter side becomes S, the other max(1, floor(S long / short + 0.5))); 1, 2 Ho (or S), Wo; 3, 4
 *           CropAnisotropy [amin amax] ([0 0]: the window has the image's aspect ratio); 5, 6 CropSize [smin smax] in
 *           (0, 1]; 7 CropLocation (0 center, 1 random); 8 Flip; 9 filter (XM_IMREAD_BOX / _BILINEAR / _BICUBIC: Keys,
 *           a = -1/2); 10 antialias (widen the kernel by max(r, 1)); 11 Contrast C; 12 Saturation S; 13-21 Brightness B,
 *           3 x 3 row-major; 22 SubtractAverage (0 none, 1 three values, 2 an Ho x Wo x 3 image)
 *   draws   N x XM_IMREAD_DRAWS doubles: u0 anisotropy, u1 size, u2 y, u3 x, u4 flip (mirrored when < 0.5), u5 contrast, u6
 *           saturation in [0, 1], then g0..g2 ~ N(0, 1) for Brightness; NULL when no option is random
 *   rows    N rows of XM_IMREAD_ROW doubles: 0 H; 1 W; 2 pixel offset; 3 Ho; 4 Wo; 5 offset of the Ho x Wo x 3 output in
 *           `out` (floats); 6-9 the window y0, x0, ch, cw; 10 flip; 11 filter; 12 antialias; 13, 14 taps Ty, Tx; 15-23 the
 *           colour matrix sigma gamma I + (1 - sigma) gamma / 3 11' (row-major); 24-26 its product with b = B g; 27 gamma;
 *           28 sigma; 29-31 b; 32 offset of the image's tap tables in the stage's scratch (4-byte words: Ty x Ho and
 *           Wo x Tx weights, Ho and Wo first taps); 33 output rows per LDS chunk; 34, 35 the ratios ch / Ho, cw / Wo;
 *           36, 37 the kernel widening per axis; 38 column tiles; 39 offset of its partial sums; 40 SubtractAverage kind;
 *           41 Contrast on; 42, 43 zero
 *   sizes   XM_IMREAD_SIZES int64: output floats, table words, partial sums, most column tiles of an image, Contrast on,
 *           all outputs of one size, longest output side, N
 * XM_EINVAL with a message: CropSize outside (0, 1], amin > amax, a random option without draws, an average image with
 * ragged outputs ...; XM_ENOTSUP naming the image: a window reduced by more than 64 on an axis; XM_ETOOBIG: a side above
 * 32768.
 * xm_imread_transform_batch: device.  desc: the rows on the device; rows: the same rows on the host, from which the launch
 * geometry is read and which are checked against what the plan writes; avg: three floats or an Ho x Wo x 3 image on the
 * device (NULL without SubtractAverage); out: sizes[0] floats.  Output sample o of an axis with n inputs, m outputs and
 * window (c0, len) reads at u = c0 + (o' + 1/2) len / m - 1/2 (o' = m - 1 - o on the mirrored horizontal axis) the taps
 * floor(u - S s / 2) + 1 ... with weights k((t - u) / s) divided by their sum, indices clamped to [0, n - 1]; weights in
 * double rounded once to float, sums in fp32, horizontal pass first.  Then p - a + b, contrast towards the channel means
 * of that, saturation towards the pixel's grey.  The same bits on every run, and for an image alone
 * or in any batch.  xm_imread_geometry's launches (2, with Contrast 3) whatever N and the sizes; scratch from the
 * stream's workspace; no synchronisation.
 * xm_imread_geometry: host only.  tile_rows x tile_cols x 3 floats is the LDS tile of the resampling kernel.
 * xm_imread_round_u8: y = min(max(floor(x + 1/2), 0), 255) over n values (y may be x), one launch: the uint8 conversion
 * of the narrow path for a caller that hands the stage's unrounded outputs to a consumer of uint8 values. */
enum { XM_IMREAD_ROW = 44, XM_IMREAD_OPTS = 24, XM_IMREAD_DRAWS = 10, XM_IMREAD_SIZES = 8 };
enum { XM_IMREAD_BOX = 0, XM_IMREAD_BILINEAR = 1, XM_IMREAD_BICUBIC = 2 };
int xm_imread_plan(const long long *hw, int N, const double *opts, const double *draws, double *rows, long long *sizes);
int xm_imread_transform_batch(const float *pixels, const double *desc, int N, const double *rows, const float *avg,
                              float *out, void *stream);
int xm_imread_geometry(int *launches, int *launches_contrast, int *tile_rows, int *tile_cols);
int xm_imread_round_u8(const float *x, long long n, float *y, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* XMODAL_H */

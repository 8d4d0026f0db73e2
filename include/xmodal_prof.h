/*
 * xmodal_prof.h -- measurement hooks of libxmodal_hip.so (NOT part of the drop-in operator ABI).
 * bench.py uses them to time each convolution kernel instantiation with HIP events recorded on
 * the stream the kernel is launched on, and to attach the algorithmic FLOPs of every launch
 * (2 * M * pixels * taps, un-padded), so that roofline.achieved is measured live; the tests read
 * from them which kernel a call ran.  csrc/prof.h (ProfScope, the keys), csrc/prof.cpp (the table
 * of keys and names); from Python: mcncrossmodalemotions_amd/prof.py.
 */
/*
 * Environment the library reads (nothing else): every name is read once.
 *   tuning table   XM_TUNE_FILE (path; "" disables), XM_AUTOTUNE=0 (analytic model only), XM_TUNE_REPS, XM_TUNE_VERBOSE,
 *                  XM_HALO_MARGIN (a challenger kernel must win by this fraction, default 0.04), XM_W8_MIN_TILES (the
 *                  eight-wave configuration is a candidate for launches of at least this many 128 x 128 tiles, default 1024),
 *                  XM_WGRAD_PATCH_SLOTS (conv_wgrad_patch_kernel's grid: blocks per round, default 768; WHETHER that kernel
 *                  is a candidate is the host's xm_set_exec_hint(XM_EXEC_SINGLE_STREAM), not an environment setting)
 *                  XM_WGRAD_PATCH_MIN_STAGES (conv_wgrad_patch_kernel without the one-stream hint: launches of at least this
 *                  many output columns, default 4096), XM_DGRAD_S2_MIN_BLOCKS (conv_dgrad_s2_kernel: launches of at least this
 *                  many blocks, default 6 x 768), XM_STEM3_WIDE=0 (conv_stem3_kernel with 128- instead of 256-pixel block tiles)
 *   workspace log  XM_WS_VERBOSE
 *   kernel-path selectors (csrc/xm_common.h `enum Path`, read in ONE place, csrc/context.cpp): XM_NO_HYBRID, XM_NO_HALO,
 *                  XM_NO_SKINNY, XM_NO_SKINNY4, XM_NO_STEM, XM_NO_STEM_WGRAD, XM_NO_DMA, XM_NO_FUSED_STATS,
 *                  XM_DGRAD_MERGE, XM_NO_FAST_TRANSPOSE, XM_NO_POOL_LDS, XM_NO_POOL_PATCH, XM_NO_POOL_POOLED,
 *                  XM_NO_W8, XM_NO_WGRAD_PATCH, XM_NO_WGRAD_PATCH_S2, XM_NO_DGRAD_S2, XM_NO_STEM3.
 *                  Each chooses between two complete, parity-tested implementations of the same operator (the operator tests
 *                  force both arms through xm_debug_set; tests/test_gpu_path_switches.py runs whole passes
 *                  with every selector set, in fresh processes, against the default; profiles/ holds the A/B lines);
 *                  none changes what is computed.
 */
#ifndef XMODAL_PROF_H
#define XMODAL_PROF_H
#ifdef __cplusplus
extern "C" {
#endif
/* on != 0: start recording (drops previous records); on == 0: stop recording, keep records */
int xm_prof_enable(int on);
/* after the stream has been synchronised: per-kernel totals in first-launch order; writes at most cap entries (cap 0:
 * none, the arrays may be NULL) and returns #distinct kernels */
int xm_prof_collect(int cap, int *keys, double *total_ms, double *total_flops, long long *launches);
/* algorithmic HBM bytes (x + f + y [+ residual], every operand once) of the recorded launches, per kernel */
int xm_prof_collect_bytes(int cap, int *keys, double *total_bytes);
/* name of a key, identical to the kernel name rocprofv3 --kernel-trace prints (sans namespace); a key that no launch
 * site records is XM_EINVAL and leaves buf empty */
int xm_prof_kernel_name(int key, char *buf, int len);
/* Test / tools switches: ONE entry (round 6; rounds 2-5 exported one xm_debug_force_* function per switch).  They select
 * between complete, parity-tested implementations of an operator (never what is computed) and are process-global: a host
 * that embeds the library has no reason to call this.  xm_debug_set returns the previous value, xm_debug_get the current
 * one; INT_MIN = unknown key.
 *   "conv_cfg"       tile configuration of every implicit-GEMM launch, 0 .. xm_debug_get("num_conv_cfgs") - 1; -1 = measured / modelled choice
 *   "conv_splits"    split-K factor of the implicit-GEMM launches (0 = automatic)
 *   "conv_last_combine"  (read only) what the most recent implicit-GEMM launch left to conv_splitk_epilogue_kernel: 0 = nothing,
 *                    z > 0 = z partial slabs combined by its 16-byte form, z < 0 = |z| slabs by its scalar form
 *   "conv_last_lattice"  (read only) 1: the most recent xm_nnconv_forward_lattice call computed the lattice pixels only; 0: it ran
 *                    the layer at full extent (the full-extent selection of the shape was not known without a measurement, or
 *                    was no implicit-GEMM launch, or the layer has filter groups)
 *   "wgrad_last_splits"  (read only) the final split count of the most recent filter-derivative launch (generic or patch kernel):
 *                    the number of partial slabs reduce_splits_kernel added, 1 = none
 *   "bias_grad_last_splits"  (read only) sample splits S of the most recent bias-derivative launch
 *   "stats_last_splits"  (read only) tile splits S of the most recent reduction of the forward epilogue's batch statistics;
 *                    0: the most recent forward with batch moments took them from a pass over Y instead
 *   "dgrad_last_transpose"  (read only) 1: the most recent dgrad filter operand came from transpose_filter_kernel, 0: from
 *                    prep_dgrad_filter_kernel (neither is profiled)
 *   "dgrad_last_prepared"  (read only) where the most recent DZDX call (xm_nnconv_prepare_backward does not count) took its filter
 *                    operand from: 1 = the operand xm_nnconv_prepare_backward had built, 0 = built inside the call, -1 = the call
 *                    went a route without such an operand (conv_dgrad_s2_kernel, or no stride class that holds a tap)
 *   "conv_halo"      1 + v: halo-patch kernel variant v (0: 128-row tiles, 1: 96-row tiles, 2: 96-row tiles / tall patch) wherever it
 *                    can run, another runnable variant otherwise; 0: never; -1: measured choice (default)
 *   "conv_stem"      1: the single-channel stem kernels (conv_stem_kernel, conv_stem_wgrad_*; also gates the Gram route's kernels)
 *                    wherever they can run; 0: never; -1: measured choice (default)
 *   "conv_stem3"     the same for the three-channel 7 x 7 / stride 2 stem kernel (conv_stem3_kernel: the teachers' first layer)
 *   "wgrad_patch"    1: conv_wgrad_patch_kernel (filter derivative of 3 x 3 / stride 1 / pad 1 layers) wherever it can run; 0: never; -1: default
 *   "wgrad_patch_s2" the same for conv_wgrad_patch_s2_kernel (5 x 5 / stride 2: the student's conv2)
 *   "dgrad_s2"       0: never conv_dgrad_s2_kernel (dgrad of 5 x 5 / stride 2 layers); 1 / -1: wherever it can run (default)
 *   "spec_blocks"    v >= 1: xm_spec_bucket_batch launches spec_gemm_kernel with min(v, 65535) blocks (and sizes the partial
 *                    slots from it), so that a small input gives every block many tiles; 0 or negative: CUs x 2 (default).
 *                    Only the grouping of the fp64 merges of a clip's statistics follows it (tests/test_gpu_spec_edges.py)
 *   "conv_split_want"  what xm_nnconv_split_geometry reports as WANT: 1 wherever the bf16x3 kernel can run, 0 nowhere, -1 the
 *                    measured rule of conv_split_plan.h (default).  The kernel itself runs whenever it is called
 *   "comm_single"    1: xm_comm_init with one worker creates a real one-rank RCCL communicator (tests of the exchange path)
 * (xm_debug_conv_cycles -- per-block shader-clock records for tools/conv_bench.py --cycles -- exists only in a library
 * built with XM_DEBUG_CYCLES=1.) */
int xm_debug_set(const char *key, int value);
int xm_debug_get(const char *key);
#ifdef __cplusplus
}
#endif
#endif

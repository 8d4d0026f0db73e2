"""Worker of tests/test_gpu_conv_dispatch_digest.py.  Run in a fresh process (the library reads XM_AUTOTUNE once):

    python tests/_dispatch_worker.py results out.json     every dispatch arm of csrc/conv.hip, forced or analytic:
                                                           kernel names + SHA-256 of every output (XM_AUTOTUNE=0)
    python tests/_dispatch_worker.py keys out.json        one launch per tune kind with find mode on: the table keys

Only vl.* (the public C ABI) and the debug switches of _lib are used.  Inputs are seeded on the host."""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEM = dict(H=268, W=13, N=2)          # 7 x 7 / stride 2, no padding: 131 x 4 outputs per sample


class Recorder:
    def __init__(self):
        import torch
        from mcncrossmodalemotions_amd import _lib, prof, vl
        self.torch, self.vl, self.prof, self.L = torch, vl, prof, _lib.load()
        self.cases = {}
        self.count = 0

    def arr(self, *shape, scale=1.0):
        """seeded host data -> device tensor in MATLAB layout (a new seed per tensor, in call order)"""
        self.count += 1
        rng = np.random.default_rng(1000 + self.count)
        return self.vl.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))

    def digest(self, t):
        if t.dtype == self.torch.float32 and t.dim() > 1:
            t = t.permute(*reversed(range(t.dim())))
        return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()

    def case(self, name, fn, **switches):
        """run fn() under the given debug switches; store the kernels it launched and the digests of what it returned"""
        L = self.L
        old = {k: L.xm_debug_set(k.encode(), int(v)) for k, v in switches.items()}
        try:
            out, rows = self.prof.kernels_run(fn, L)
        finally:
            for k, v in old.items():
                L.xm_debug_set(k.encode(), v)
        assert out is not None, name + ": the entry point refused the shape"
        outs = [t for t in (out if isinstance(out, (tuple, list)) else [out]) if t is not None]
        assert name not in self.cases, name
        self.cases[name] = {"kernels": ["%s x%d" % (r.name, r.launches) for r in rows], "sha256": [self.digest(t) for t in outs]}
        return out


def results(rec):
    vl, torch, A = rec.vl, rec.torch, rec.arr
    conv = vl.vl_nnconv

    # ---- forward -------------------------------------------------------------------------------------------------
    x33, f33, b32 = A(12, 10, 16, 3), A(3, 3, 16, 32, scale=0.1), A(32, 1)
    rec.case("fwd_plain", lambda: conv(x33, f33, b32, pad=1))
    x77, f77 = A(20, 20, 3, 2), A(7, 7, 3, 16, scale=0.1)
    rec.case("fwd_padded_rows", lambda: conv(x77, f77, None, pad=3))
    xw, fw = A(4, 100, 1, 2), A(1, 65, 1, 8, scale=0.1)
    rec.case("fwd_65_taps", lambda: conv(xw, fw, None))
    xg, fg, bg = A(8, 8, 8, 2), A(3, 3, 4, 16, scale=0.1), A(16, 1)
    rec.case("fwd_groups", lambda: conv(xg, fg, bg, pad=1))
    xs2, fs2 = A(13, 11, 4, 2), A(3, 3, 4, 8, scale=0.1)
    rec.case("fwd_stride2_asym", lambda: conv(xs2, fs2, None, stride=2, pad=[0, 1, 1, 0]))
    xd2, fd2 = A(12, 12, 4, 2), A(3, 3, 4, 8, scale=0.1)
    rec.case("fwd_dilate2", lambda: conv(xd2, fd2, None, dilate=2, pad=2))
    # 1 x 1 layers: 192 pixels (more than the skinny route takes); 8 x 8 planes are LDS-DMA eligible, 7 x 7 are not
    x11, x11o, f11 = A(8, 8, 64, 3), A(7, 7, 64, 3), A(1, 1, 64, 64, scale=0.1)
    for ci in range(rec.L.xm_debug_num_conv_cfgs()):
        rec.case("fwd_1x1_cfg%d" % ci, lambda: conv(x11, f11, None), conv_cfg=ci)
        rec.case("fwd_1x1_odd_cfg%d" % ci, lambda: conv(x11o, f11, None), conv_cfg=ci)
    rec.case("fwd_splits3", lambda: conv(x33, f33, b32, pad=1), conv_splits=3)
    xh, fh = A(64, 64, 256, 17), A(1, 1, 256, 128, scale=0.05)
    rec.case("fwd_hybrid", lambda: conv(xh, fh, None), conv_cfg=0)
    del xh, fh

    def with_moments(x, f, b, **kw):
        mo = vl.mat_empty(f.shape[3], 2)
        return conv(x, f, b, moments_out=mo, **kw), mo

    rec.case("moments_plain", lambda: with_moments(x33, f33, b32, pad=1))
    x33w, f33w = A(12, 10, 32, 3), A(3, 3, 32, 32, scale=0.1)
    rec.case("moments_splitk", lambda: with_moments(x33w, f33w, b32, pad=1))
    rec.case("moments_halo", lambda: with_moments(x33, f33, b32, pad=1), conv_halo=1)
    xst, fst96, fst40 = A(STEM["H"], STEM["W"], 1, STEM["N"]), A(7, 7, 1, 96, scale=0.1), A(7, 7, 1, 40, scale=0.1)
    b96, b40 = A(96, 1), A(40, 1)
    rec.case("moments_stem", lambda: with_moments(xst, fst96, b96, stride=2), conv_stem=1)
    sc, sh, rs = A(32, 1), A(32, 1), A(12, 10, 32, 3)
    rec.case("fwd_fused_epilogue", lambda: conv(x33, f33, b32, pad=1, scale=sc, shift=sh, residual=rs, relu=True))
    gate = A(1, 1, 32, 3)
    rec.case("fwd_gated", lambda: conv(x33, f33, b32, pad=1, scale=sc, shift=sh, gate=gate, residual=rs, relu=True))
    xh8, fh96 = A(12, 10, 8, 3), A(3, 3, 8, 96, scale=0.1)
    rec.case("fwd_halo1", lambda: conv(xh8, fh96, b96, pad=1), conv_halo=1)
    rec.case("fwd_halo2", lambda: conv(xh8, fh96, b96, pad=1), conv_halo=2)
    xtall = A(100, 6, 8, 2)             # 102-row patch columns: more than 512 floats per channel under a pixel tile
    rec.case("fwd_halo3", lambda: conv(xtall, fh96, b96, pad=1), conv_halo=3)
    rec.case("fwd_stem_k96", lambda: conv(xst, fst96, b96, stride=2), conv_stem=1)
    rec.case("fwd_stem_k40", lambda: conv(xst, fst40, b40, stride=2), conv_stem=1)
    xrgb, frgb, b64 = A(128, 4, 3, 2), A(7, 7, 3, 64, scale=0.1), A(64, 1)
    rec.case("fwd_stem3", lambda: conv(xrgb, frgb, b64, stride=2, pad=3), conv_stem3=1)

    # ---- dgrad ---------------------------------------------------------------------------------------------------
    def dgrad(x, f, dz, acc=None, **kw):
        return conv(x, f, None, dz, no_der_filters=True, dx_accum=acc, **kw)[0]

    dz33, acc33 = A(12, 10, 32, 3), A(12, 10, 16, 3)
    rec.case("dgrad_s1", lambda: dgrad(x33, f33, dz33, pad=1))
    rec.case("dgrad_s1_accum", lambda: dgrad(x33, f33, dz33, acc33, pad=1))
    xq, fq, dzq, accq = A(13, 11, 8, 2), A(3, 3, 8, 16, scale=0.1), A(7, 6, 16, 2), A(13, 11, 8, 2)
    rec.case("dgrad_s2", lambda: dgrad(xq, fq, dzq, stride=2, pad=1))
    rec.case("dgrad_s2_accum", lambda: dgrad(xq, fq, dzq, accq, stride=2, pad=1))
    x1s, f1s, dz1s, acc1s = A(8, 8, 8, 2), A(1, 1, 8, 16, scale=0.1), A(4, 4, 16, 2), A(8, 8, 8, 2)
    rec.case("dgrad_1x1_s2", lambda: dgrad(x1s, f1s, dz1s, stride=2))
    rec.case("dgrad_1x1_s2_accum", lambda: dgrad(x1s, f1s, dz1s, acc1s, stride=2))
    xf, ff, dzf = A(9, 20, 8, 2), A(9, 1, 8, 16, scale=0.1), A(1, 20, 16, 2)
    rec.case("dgrad_foldH", lambda: dgrad(xf, ff, dzf))
    xfc, ffc, dzfc = A(1, 1, 64, 8), A(1, 1, 64, 32, scale=0.1), A(1, 1, 32, 8)
    rec.case("dgrad_skinny_fc", lambda: dgrad(xfc, ffc, dzfc))
    dzg = A(8, 8, 16, 2)
    rec.case("dgrad_groups", lambda: dgrad(xg, fg, dzg, pad=1))
    xm, fm, dzm = A(64, 64, 8, 32), A(5, 5, 8, 8, scale=0.1), A(32, 32, 8, 32)
    rec.case("dgrad_merged", lambda: dgrad(xm, fm, dzm, stride=2, pad=2))
    rec.case("dgrad_merged_halo", lambda: dgrad(xm, fm, dzm, stride=2, pad=2), conv_halo=1)
    x52, f52, dz52 = A(8, 8, 8, 2), A(5, 5, 8, 8, scale=0.1), A(4, 4, 8, 2)
    rec.case("dgrad_s2_kernel", lambda: dgrad(x52, f52, dz52, stride=2, pad=[1, 2, 1, 2]), dgrad_s2=1)

    def prepared():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            vl.conv_prepare_backward(xq, fq, stride=2, pad=1)
        return dgrad(xq, fq, dzq, stride=2, pad=1)

    rec.case("dgrad_prepared", prepared)

    # ---- wgrad ---------------------------------------------------------------------------------------------------
    def wgrad(x, f, b, dz, **kw):
        return conv(x, f, b, dz, no_der_data=True, **kw)[1:]

    for ci in range(7):
        rec.case("wgrad_cfg%d" % ci, lambda: wgrad(x33, f33, b32, dz33, pad=1), conv_cfg=ci)
    dzst = A(131, 4, 96, STEM["N"])
    rec.case("wgrad_stem", lambda: wgrad(xst, fst96, b96, dzst, stride=2), conv_stem=1)
    xp, fp, dzp = A(30, 8, 16, 8), A(3, 3, 16, 16, scale=0.1), A(30, 8, 16, 8)
    rec.case("wgrad_patch", lambda: wgrad(xp, fp, None, dzp, pad=1), wgrad_patch=1)
    xp2, fp2, dzp2 = A(16, 16, 8, 16), A(5, 5, 8, 16, scale=0.1), A(8, 8, 16, 16)
    rec.case("wgrad_patch_s2", lambda: wgrad(xp2, fp2, None, dzp2, stride=2, pad=[1, 2, 1, 2]), wgrad_patch_s2=1)

    # ---- the fused stem entry points (smallest shapes of tests/test_gpu_stem_pool.py / test_gpu_ops.py) ------------
    xs, fs, bs = A(256, 36, 1, 2), A(6, 7, 1, 40, scale=0.2), A(40, 1)
    g40, bb40 = A(40, 1), A(40, 1)
    fwd = rec.case("stem_fused_forward", lambda: vl.conv_bnorm_relu_pool(xs, fs, bs, g40, bb40, [3, 3], stride=2,
                                                                         pad=[2, 3, 1, 1], pool_stride=2, pool_pad=0))
    yp, am, mo, gram = fwd
    dzs = A(*yp.shape)
    for tag, ypool in (("table", None), ("ypool", yp)):
        rec.case("stem_fused_backward_" + tag, lambda: vl.conv_backward_filter_bnrelupool_gram(
            xs, fs, bs, g40, mo, am, ypool, dzs, [3, 3], stride=2, pad=[2, 3, 1, 1], pool_stride=2, pool_pad=0, gram=gram))
    xg2, fg2 = A(132, 20, 1, 2), A(7, 7, 1, 40, scale=0.2)
    y2 = conv(xg2, fg2, bs, stride=2, pad=1)
    yp2, am2, mo2 = vl.bnorm_relu_pool(y2, g40, bb40, [3, 3], stride=2, pad=0)
    dz2 = A(*yp2.shape)
    rec.case("stem_gram_backward", lambda: vl.conv_backward_filter_bnrelupool_gram(
        xg2, fg2, bs, g40, mo2, am2, yp2, dz2, [3, 3], stride=2, pad=1, pool_stride=2, pool_pad=0))
    xb, fb = A(264, 12, 1, 2), A(7, 7, 1, 40, scale=0.2)
    y3 = conv(xb, fb, bs, stride=2, pad=1)
    yp3, am3, mo3 = vl.bnorm_relu_pool(y3, g40, bb40, [3, 3], stride=2, pad=0)
    dz3 = A(*yp3.shape)
    rec.case("stem_bnp_backward", lambda: vl.conv_backward_filter_bnrelupool(
        xb, (7, 7, 1, 40), y3, g40, bb40, mo3, am3, yp3, dz3, [3, 3], stride=2, pad=1, pool_stride=2, pool_pad=0))
    return rec.cases


def keys(rec):
    """one launch per tune kind just above its policy threshold, no force hook: the keys xm_tune_save writes"""
    vl, A = rec.vl, rec.arr
    conv = vl.vl_nnconv
    x33, f33, dz33 = A(12, 10, 16, 3), A(3, 3, 16, 32, scale=0.1), A(12, 10, 32, 3)
    conv(x33, f33, None, pad=1)                                              # kinds 0 and 4
    conv(x33, f33, None, dz33, pad=1)                                        # 1, 5 (one class) and 2
    xm, fm, dzm = A(64, 64, 8, 32), A(5, 5, 8, 8, scale=0.1), A(32, 32, 8, 32)
    conv(xm, fm, None, dzm, stride=2, pad=2, no_der_filters=True)            # 3 and 6: 512 tiles over the four classes
    xs, fs, dzs = A(512, 60, 1, 10), A(7, 7, 1, 96, scale=0.1), A(254, 28, 96, 10)
    conv(xs, fs, None, stride=2, pad=1)                                      # 7: 71 120 outputs
    conv(xs, fs, None, dzs, stride=2, pad=1, no_der_data=True)               # 8
    xr, fr = A(224, 224, 3, 6), A(7, 7, 3, 64, scale=0.1)
    conv(xr, fr, None, stride=2, pad=3)                                      # 12: 75 264 outputs
    xp, fp, dzp = A(30, 8, 16, 8), A(3, 3, 16, 16, scale=0.1), A(30, 8, 16, 8)
    old = vl.set_exec_hint(vl.EXEC_SINGLE_STREAM)
    conv(xp, fp, None, dzp, pad=1, no_der_data=True)                         # 9: N W = 64
    vl.set_exec_hint(old)
    xp2, fp2, dzp2 = A(16, 16, 8, 8), A(5, 5, 8, 16, scale=0.1), A(8, 8, 16, 8)
    conv(xp2, fp2, None, dzp2, stride=2, pad=[1, 2, 1, 2], no_der_data=True)  # 10: N Wo ceil(Ho / 32) = 64
    rec.torch.cuda.synchronize()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "keys.txt")
        vl.tune_save(path)
        lines = open(path).read().splitlines()[1:]
    return sorted([int(v) for v in ln.split()[:9]] for ln in lines)


if __name__ == "__main__":
    what, out = sys.argv[1], sys.argv[2]
    res = results(Recorder()) if what == "results" else keys(Recorder())
    with open(out, "w") as fp:
        json.dump(res, fp, indent=0, sort_keys=True)

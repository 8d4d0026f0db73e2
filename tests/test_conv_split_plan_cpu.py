"""CPU (no device): the planning and the argument checks of the bf16x3 arm of 1 x 1 layers (csrc/conv_split_plan.h through
xm_nnconv_split_geometry, xm_nnconv_forward_split's refusals), the bound its GPU test uses pinned by emulation, and the
plumbing of the option through vl_nnconv, dagnn plans and the <teacher>-logits.mat cache."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

XM_EINVAL, XM_ENOTSUP = 1, 5
RELU, SIGMOID = 1, 4


def geometry(H, W, Cc, N, FH, FW, FC, K, stride=(1, 1), pad=(0, 0, 0, 0), dilate=(1, 1), flags=0):
    from mcncrossmodalemotions_amd import _lib
    out = [C.c_int(-7) for _ in range(4)]
    rc = _lib.load().xm_nnconv_split_geometry(H, W, Cc, N, FH, FW, FC, K, *stride, *pad, *dilate, flags,
                                              *[C.byref(o) for o in out])
    assert rc == 0
    return dict(zip(("can", "want", "blocks", "launches"), (o.value for o in out)))


def test_abi_revision():
    from mcncrossmodalemotions_amd import _lib
    assert _lib.load().xm_version() >= 124


def test_can():
    assert geometry(1, 1, 1, 1, 1, 1, 1, 1) == dict(can=1, want=0, blocks=1, launches=1)     # every extent 1
    assert geometry(14, 14, 64, 2, 1, 1, 64, 32, dilate=(2, 3))["can"] == 1                   # dilation: accepted, ignored
    assert geometry(14, 14, 64, 2, 1, 1, 64, 32, stride=(2, 3), flags=RELU)["can"] == 1
    refused = [geometry(14, 14, 64, 2, 3, 3, 64, 32), geometry(14, 14, 64, 2, 1, 3, 64, 32),
               geometry(14, 14, 64, 2, 1, 1, 32, 32),                                          # FC != C: filter groups
               geometry(14, 14, 64, 2, 1, 1, 64, 32, flags=SIGMOID),
               geometry(14, 14, 64, 2, 1, 1, 64, 32, stride=(0, 1)),
               geometry(0, 14, 64, 2, 1, 1, 64, 32), geometry(14, 14, 64, 0, 1, 1, 64, 32),
               geometry(256, 256, 4096, 8, 1, 1, 4096, 8),                                     # x has 2^31 elements
               geometry(256, 256, 8, 8, 1, 1, 8, 4096)]                                        # y has 2^31 elements
    refused += [geometry(14, 14, 64, 2, 1, 1, 64, 32, pad=tuple(int(i == j) for j in range(4))) for i in range(4)]
    assert all(g == dict(can=0, want=0, blocks=0, launches=0) for g in refused), refused
    assert geometry(256, 256, 4095, 8, 1, 1, 4095, 8)["can"] == 1                             # just below the limit


# the shapes of tests/test_gpu_conv_split.py: (H, W, C, N, K, stride)
GPU_SHAPES = [(1, 1, 1, 1, 1, (1, 1)), (5, 7, 15, 3, 31, (1, 1)), (9, 4, 16, 1, 32, (1, 1)), (5, 7, 17, 3, 33, (1, 1)),
              (9, 4, 24, 3, 40, (1, 1)), (3, 3, 2048, 1, 33, (1, 1)), (12, 11, 40, 3, 70, (1, 1)), (7, 5, 17, 3, 40, (2, 2)),
              (7, 5, 17, 3, 40, (2, 1)), (7, 5, 17, 3, 40, (1, 3)), (5, 7, 300, 3, 33, (2, 3)), (3, 3, 64, 2, 8, (1, 1)),
              (14, 14, 1024, 128, 256, (1, 1)), (56, 56, 64, 32, 256, (2, 2))]


def test_launch_geometry_matches_its_restatement():
    for H, W, Cc, N, K, (sy, sx) in GPU_SHAPES:
        pixels = ((H - 1) // sy + 1) * ((W - 1) // sx + 1) * N
        want = -(-pixels // 128) * -(-K // 64)          # 128 pixels (numbered across samples) x 64 output channels per block
        g = geometry(H, W, Cc, N, 1, 1, Cc, K, stride=(sy, sx))
        assert (g["can"], g["blocks"], g["launches"]) == (1, want, 1), (H, W, Cc, N, K, sy, sx, g)


def test_want_switch_and_rule_are_pure():
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    shape = (14, 14, 1024, 128, 1, 1, 1024, 256)
    rule = geometry(*shape)["want"]
    assert geometry(*shape)["want"] == rule
    old = L.xm_debug_set(b"conv_split_want", 1)
    try:
        assert old == -1 and geometry(*shape)["want"] == 1
        assert geometry(14, 14, 64, 2, 3, 3, 64, 32)["want"] == 0           # never without can
        L.xm_debug_set(b"conv_split_want", 0)
        assert geometry(*shape)["want"] == 0
    finally:
        L.xm_debug_set(b"conv_split_want", -1)
    assert geometry(*shape)["want"] == rule


def split(x, f, y, shape, stride=(1, 1), pad=(0, 0, 0, 0), resid=None, res=(0, 0, 1, 1), flags=0, precision=1):
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    rc = L.xm_nnconv_forward_split(x, *shape[:4], f, *shape[4:], None, y, *stride, *pad, 1, 1, None, None, None, resid, *res,
                                   flags, precision, None)
    return rc, L.xm_last_error().decode()


def test_refusals_come_before_any_device_call():
    """there is no device here: a call that got as far as a launch would return XM_EHIP (3)"""
    one = (14, 14, 64, 2, 1, 1, 64, 32)
    for shape, kw, word in [((14, 14, 64, 2, 3, 3, 64, 32), {}, "larger than 1 x 1"),
                            (one, dict(pad=(1, 1, 1, 1)), "padding"), (one, dict(pad=(0, 0, 0, 1)), "padding"),
                            ((14, 14, 64, 2, 1, 1, 32, 32), {}, "filter groups"),
                            (one, dict(flags=SIGMOID), "sigmoid")]:
        rc, msg = split(None, None, None, shape, **kw)
        assert rc == XM_ENOTSUP and word in msg, (shape, kw, rc, msg)
    rc, msg = split(None, None, None, one, precision=0)
    assert rc == XM_EINVAL and "XM_CONV_F32" in msg
    for p in (2, -1, 77):
        rc, msg = split(None, None, None, one, precision=p)
        assert rc == XM_EINVAL and "unknown precision %d" % p in msg
    rc, msg = split(None, None, None, one)
    assert rc == XM_EINVAL and "NULL tensor" in msg
    # a residual whose sampled extent is not the output's (the operand is a host buffer nothing reads: x is NULL too)
    host = (C.c_float * 16)()
    for res in [(13, 14, 1, 1), (14, 14, 2, 1), (14, 14, 1, 0), (0, 14, 1, 1)]:
        rc, msg = split(None, None, None, one, resid=C.cast(host, C.c_void_p), res=res)
        assert rc == XM_EINVAL and ("does not give" in msg), (res, rc, msg)
    rc, msg = split(None, None, None, one, stride=(2, 2), resid=C.cast(host, C.c_void_p), res=(14, 14, 2, 2))
    assert rc == XM_EINVAL and "NULL tensor" in msg          # extents fine (7 x 7 output): stopped by the NULL operands


# ---- the bound of the GPU test, pinned by emulation --------------------------------------------------------------------
def fixed_mantissa(rng, shape):
    j, e = rng.integers(0, 4, shape), rng.integers(-3, 3, shape)
    return ((1 + 2.0 ** -8 - 2.0 ** -17 + j * 2.0 ** -23) * 2.0 ** e).astype(np.float32)


def halves(v):
    t = torch.from_numpy(v)
    hi = t.to(torch.bfloat16).to(torch.float32)          # round to nearest even
    lo = (t - hi).to(torch.bfloat16).to(torch.float32)   # t - hi is exact in fp32
    return hi.numpy().astype(np.float64), lo.numpy().astype(np.float64)


def operands(kind, rng, Cc, P=24, K=16):
    if kind == "fixed":
        return fixed_mantissa(rng, (P, Cc)), fixed_mantissa(rng, (Cc, K))
    x, f = rng.standard_normal((P, Cc)).astype(np.float32), rng.standard_normal((Cc, K)).astype(np.float32)
    return (np.maximum(x, 0) if kind == "relu" else x), f


@pytest.mark.parametrize("Cc", [16, 64, 2048])
@pytest.mark.parametrize("kind", ["randn", "relu", "fixed"])
def test_three_terms_meet_the_bound_and_two_do_not(kind, Cc):
    x, f = operands(kind, np.random.default_rng(Cc), Cc)
    (xh, xl), (fh, fl) = halves(x), halves(f)
    exact = x.astype(np.float64) @ f.astype(np.float64)
    bound = 3 * 2.0 ** -16 * (np.abs(x).astype(np.float64) @ np.abs(f).astype(np.float64))
    three = xl @ fh + xh @ fl + xh @ fh                       # fp64 sums of exact bf16 x bf16 products
    ratio = float((np.abs(three - exact) / bound).max())
    print("%s C=%d: three terms, worst error / bound = %.3f" % (kind, Cc, ratio))
    assert ratio <= 1.0
    # one cross term forgotten: over the bound at every depth up to 256; at 2048 the random signs of randn operands can
    # average the missing term away, the one-signed fixed-mantissa operands cannot
    if Cc <= 256 or kind == "fixed":
        for name, two in (("x_lo f_hi missing", xh @ fl + xh @ fh), ("x_hi f_lo missing", xl @ fh + xh @ fh)):
            r2 = float((np.abs(two - exact) / bound).max())
            print("   %s: %.1f x the bound" % (name, r2))
            assert r2 > 4.0, (name, r2)


# ---- plumbing -----------------------------------------------------------------------------------------------------------
def quarter_resnet(se):
    from mcncrossmodalemotions_amd import zoo
    net = zoo.resnet50(se, width_mult=0.25, blocks=(1, 1, 1, 1))
    for name in ("top1error", "loss", "classifier", "pool5"):
        net.removeLayer(name)
    net.mode = "test"
    net.vars["res5ax"].precious = True
    return net


def shape_of(plan):
    return [(type(st).__name__, [q.name for q in st.recs], st.run_stride, st.out_lattice) for st in plan]


@pytest.mark.parametrize("se", [False, True], ids=["plain", "se"])
def test_default_plan_is_untouched_and_the_option_marks_conv_steps_only(se):
    from mcncrossmodalemotions_amd import dagnn
    net = quarter_resnet(se)
    assert net.convPrecision == "fp32" and net.replica().convPrecision == "fp32"
    base = net._plan(False)
    assert all(st.precision is None for st in base)
    assert sorted(st.rec.name for st in base if st.run_stride not in (None, (1, 1))) == \
        ["res2a_branch2c", "res3a_branch2c", "res4a_branch2c"]
    want = shape_of(base)
    net.convPrecision = "bf16x3"
    assert net.replica().convPrecision == "bf16x3"
    plan = net._plan(False)
    assert plan is not base and shape_of(plan) == want       # same steps, same layers, same pruning
    marked = [st for st in plan if st.precision is not None]
    assert marked and all(st.precision == "bf16x3" for st in marked)
    assert all(isinstance(st.rec.block, dagnn.Conv) for st in marked)
    assert len(marked) == sum(isinstance(l.block, dagnn.Conv) and not any(l in st.recs[1:] for st in plan) for l in net.layers)
    assert all(st.precision is None for st in net._plan(True))        # a training plan never looks at it
    net.mode = "normal"
    assert all(st.precision is None for st in net._plan(False))       # nor does a forward plan outside test mode
    net.convPrecision = "tf32"
    with pytest.raises(ValueError, match="convPrecision"):
        net._plan(False)


def test_vl_nnconv_precision_is_forward_only():
    from mcncrossmodalemotions_amd import vl
    x = torch.zeros(1)
    for kw in (dict(dzdy=x), dict(moments_out=x), dict(out_lattice=(2, 2)), dict(sigmoid=True)):
        with pytest.raises(ValueError, match="forward mode"):
            vl.vl_nnconv(x, x, precision="bf16x3", **kw)
    with pytest.raises(ValueError, match="unknown precision"):
        vl.vl_nnconv(x, x, precision="bf16")
    assert vl.conv_split_geometry((14, 14, 64, 2), (1, 1, 64, 32))["can"] is True
    assert vl.conv_split_geometry((14, 14, 64, 2), (3, 3, 64, 32), pad=1) == dict(can=False, want=False, blocks=0, launches=0)


def tiny_imdb(fe, precision=None):
    images = {"name": ["a.wav", "b.wav"], "video": ["v1", "v2"], "track": np.array([1, 1]), "id": np.array([1, 2]),
              "set": np.array([1, 2]), "numSamples": np.array([16000, 32000])}
    logits = [np.arange(16, dtype=np.float32).reshape(2, 8), np.ones((3, 8), np.float32)]
    return fe.EmoVoxImdb(images, wavLogits=logits) if precision is None else fe.EmoVoxImdb(images, wavLogits=logits, precision=precision)


def test_logits_cache_records_its_precision(tmp_path):
    from scipy.io import loadmat, savemat
    from mcncrossmodalemotions_amd import fetch_emovoxceleb_imdb as fe
    d = str(tmp_path)
    fe.save_imdb(fe.getImdbPath(d, "split"), tiny_imdb(fe, "bf16x3"))
    assert str(loadmat(fe.getImdbPath(d, "split"))["precision"][0]) == "bf16x3"
    assert fe.load_imdb(fe.getImdbPath(d, "split")).precision == "bf16x3"
    with pytest.raises(ValueError, match="'bf16x3'.*'fp32'"):                      # both names
        fe.fetch_emovoxceleb_imdb("split", d, verbose=False)
    got = fe.fetch_emovoxceleb_imdb("split", d, verbose=False, teacherPrecision="bf16x3")
    assert got.precision == "bf16x3" and np.array_equal(got.wavLogits[0], np.arange(16, dtype=np.float32).reshape(2, 8))
    with pytest.raises(ValueError, match="'bf16x3'.*'fp32'"):                      # the module cache is checked as well
        fe.fetch_emovoxceleb_imdb("split", d, verbose=False, teacherPrecision="fp32")
    # a file from before the field existed is an fp32 cache
    fe.save_imdb(fe.getImdbPath(d, "plain"), tiny_imdb(fe))
    m = {k: v for k, v in loadmat(fe.getImdbPath(d, "plain")).items() if not k.startswith("__") and k != "precision"}
    savemat(fe.getImdbPath(d, "old"), m)
    assert "precision" not in loadmat(fe.getImdbPath(d, "old"))
    assert fe.fetch_emovoxceleb_imdb("old", d, verbose=False).precision == "fp32"
    fe._CACHE.pop(("old", os.path.abspath(d)))
    with pytest.raises(ValueError, match="'fp32'.*'bf16x3'"):
        fe.fetch_emovoxceleb_imdb("old", d, verbose=False, teacherPrecision="bf16x3")
    with pytest.raises(ValueError, match="precision"):
        fe.fetch_emovoxceleb_imdb("old", d, verbose=False, teacherPrecision="half")


def test_drivers_refuse_an_unknown_precision():
    from mcncrossmodalemotions_amd import run_distillation as rd
    with pytest.raises(ValueError, match="teacherPrecision"):
        rd.run_distillation(teacherMode="online", teacherPrecision="half")
    with pytest.raises(ValueError, match="belong to teacherMode='online'"):
        rd.run_distillation(teacherPrecision="bf16x3")

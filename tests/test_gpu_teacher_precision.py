"""GPU: the bf16x3 option of the frozen teachers, from the plan to the drivers.

  * quarter-width (SE-)ResNet of tests/test_gpu_stride_prune_net.py: which kernels a bf16x3 plan runs (the split kernel once
    per 1 x 1 step it can take -- counted from the graph --, the fp32 kernels for every other convolution; the SE gate's two
    layers run fc_skinny_kernel, which the profiler does not record: that they stay fp32 shows in the launch count of the
    split kernel, which has no launch to spare for them), that the default
    precision never reaches it, agreement with the fp32 plan, and pruned == unpruned bit for bit (xmodal.h: the bits of an
    output depend on its own operands only);
  * full-size resnet50 / senet50 on the two fixture faces of tests/golden/nets_full.npz through
    zoo.FrozenTeacher(precision='bf16x3'): logits and sampled intermediate tensors within the project's forward tolerance,
    1e-4 of each tensor's largest reference magnitude (check_summary of tests/test_gpu_nets_full.py);
  * buildImdb(teacherPrecision='bf16x3') writes the field and fetch_emovoxceleb_imdb at the default precision refuses it.

The plans are built with the test switch "conv_split_want" at 1 (every layer the kernel can run), so that they do not
depend on the measured rule of conv_split_plan.h -- which may send fewer layers, never others.

Measured on the fixture faces (largest error of the sampled entries / largest reference magnitude, per tensor; allowance 1e-4):
see DESIGN.md section 23 for the figures of both precisions."""
import importlib.util
import os

import numpy as np
import pytest

from test_gpu_nets_full import build_teacher, check_summary
from test_gpu_stride_prune_net import TOL, agree, build

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SPLIT = "conv_split_kernel"


@pytest.fixture(scope="module")
def Z():
    return np.load(os.path.join(HERE, "golden", "nets_full.npz"))


@pytest.fixture(scope="module")
def M():
    spec = importlib.util.spec_from_file_location("make_golden_nets", os.path.join(HERE, "golden", "make_golden_nets.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture
def want_everywhere():
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    L.xm_debug_set(b"conv_split_want", 1)
    yield
    L.xm_debug_set(b"conv_split_want", -1)


def split_steps(net):
    """(1 x 1 steps the split kernel can take, the other convolution steps) of the forward plan, from the graph: a step
    whose head is an unpadded 1 x 1 Conv without a sigmoid behind it; the SE gate's two layers run inside their _SEFoldStep
    and are no steps of their own"""
    from mcncrossmodalemotions_amd import dagnn, vl
    can, other = [], []
    for st in net._plan(False):
        blk = st.rec.block
        if not isinstance(blk, dagnn.Conv):
            continue
        one = tuple(blk.size[:2]) == (1, 1) and not any(vl._pad4(blk.pad))
        sig = isinstance(st, dagnn._ConvActStep) and isinstance(st.act_rec.block, dagnn.Sigmoid)
        (can if one and not sig else other).append(st.rec.name)
    return can, other


def profiled_eval(net, x):
    from mcncrossmodalemotions_amd import prof, vl
    _, rows = prof.kernels_run(lambda: net.eval(["data", x]))
    split = sum(r.launches for r in rows if r.name == SPLIT)
    fp32 = sum(r.launches for r in rows if r.name != SPLIT and r.name.startswith("conv_"))
    return vl.to_numpy(net.vars["res5ax"].value), split, fp32


@pytest.mark.parametrize("se", [False, True], ids=["plain", "se"])
def test_quarter_width_plans(gpu, se, want_everywhere):
    from mcncrossmodalemotions_amd import vl
    from oracle import oracle as O
    net = build(se)
    x = vl.from_numpy(O.F(np.random.default_rng(3).standard_normal((64, 64, 3, 3))))
    ref, nsplit, nfp32 = profiled_eval(net, x)                       # default precision: want is on, nobody asks
    can, other = split_steps(net)
    assert nsplit == 0 and nfp32 >= len(other)
    assert len(can) == 12 and len(other) == 5, (can, other)          # 4 blocks x (branch1, 2a, 2c); the stem + 4 x 2b
    net.convPrecision = "bf16x3"
    got, nsplit, nfp32_split = profiled_eval(net, x)
    assert nsplit == len(can), (nsplit, can)                         # once per 1 x 1 step
    assert len(other) <= nfp32_split < nfp32                         # every 3 x 3 and the stem stay on the fp32 kernels
    agree(got, ref, "res5ax, bf16x3 against fp32")
    assert sorted(st.rec.name for st in net._plan(False) if st.run_stride not in (None, (1, 1))) == \
        ["res2a_branch2c", "res3a_branch2c", "res4a_branch2c"]
    net.stridePrune = False
    unpruned, nsplit2, _ = profiled_eval(net, x)
    assert nsplit2 == len(can) and not any(st.run_stride is not None for st in net._plan(False))
    assert np.array_equal(got, unpruned)                             # bit for bit
    net.stridePrune, net.convPrecision = True, "fp32"
    again, nsplit, _ = profiled_eval(net, x)
    assert nsplit == 0 and np.array_equal(again, ref)                # back on the default: the bits of before


def fraction(Z, prefix, name, got):
    flat = np.asarray(got, np.float32).ravel(order="F")
    ref = Z["%s_%s_samp" % (prefix, name)]
    idx = np.unique(np.linspace(0, flat.size - 1, min(flat.size, 256)).astype(np.int64))
    return float(np.abs(flat[idx].astype(np.float64) - ref).max()) / max(float(np.abs(ref).max()), 1.0)


@pytest.mark.parametrize("tag,se,seed,in_seed", [("r50", False, 100, 1), ("se50", True, 300, 3)])
def test_full_teacher_within_the_forward_tolerance(gpu, Z, M, tag, se, seed, in_seed):
    """zoo.FrozenTeacher(precision='bf16x3') as shipped -- the layers the `want` rule of conv_split_plan.h sends to the split
    kernel -- keeps the logits and the sampled intermediate tensors within 1e-4 of each tensor's largest reference
    magnitude, like the fp32 teacher.  The third run, with EVERY 1 x 1 layer on the split kernel (test switch), is measured
    and printed, not held to that bound: it does not meet it (measured on an MI355X, error / largest magnitude,
    fp32 -> all layers: r50 res2cx 1.3e-6 -> 3.1e-5, res4fx 2.4e-5 -> 5.4e-4, res5cx 6.1e-5 -> 1.9e-3, logits 2.0e-5 ->
    4.3e-4; se50 res5cx 1.0e-5 -> 3.4e-4, logits 4.2e-6 -> 9.5e-5), which is why `want` may never grow to those layers:
    DESIGN.md section 23.  What is asserted of it is what the operator promises: the split kernel ran once per 1 x 1 step
    and every output is finite."""
    from mcncrossmodalemotions_amd import _lib, prof, vl, zoo
    from oracle import graphs as G
    L = _lib.load()
    keep = ("pool1", "res2cx", "res3dx", "res4fx", "res5cx", "pool5")
    x = vl.from_numpy(G.face_batch(M.TEACHER_N, in_seed))
    ref = Z[tag + "_logits"]
    scale = max(1.0, float(np.abs(ref).max()))
    bits = {}
    for label, precision, switch in (("fp32", "fp32", -1), ("bf16x3", "bf16x3", -1), ("bf16x3, every 1 x 1 layer", "bf16x3", 1)):
        net = build_teacher(Z, M, tag, se, seed)
        net.move("gpu")
        net.mode = "test"
        for v in keep:
            net.vars[v].precious = True
        teacher = zoo.FrozenTeacher(net, lanes=2, output="prediction", precision=precision)
        assert teacher.precision == precision and all(n.convPrecision == precision for n in teacher.nets)
        L.xm_debug_set(b"conv_split_want", switch)
        try:
            logits, rows = prof.kernels_run(lambda: vl.to_numpy(teacher.logits(x)))
        finally:
            L.xm_debug_set(b"conv_split_want", -1)
        nsplit = sum(r.launches for r in rows if r.name == SPLIT)
        wanted = [st for st in net._plan(False) if any(st._split_ok.values())]
        assert nsplit == len(wanted) and (precision == "bf16x3" or nsplit == 0)
        fr = {v: fraction(Z, tag + "_var", v, vl.to_numpy(net.vars[v].value)) for v in keep}
        fr["logits"] = float(np.abs(logits.astype(np.float64) - ref).max()) / scale
        print("%s %s (%d split launches): error / largest magnitude  %s" % (
            tag, label, nsplit, "  ".join("%s %.2e" % kv for kv in fr.items())))
        if switch == 1:
            assert nsplit == len(split_steps(net)[0]) == 37 and np.isfinite(logits).all()
            continue
        for v in keep:
            check_summary(Z, tag + "_var", v, vl.to_numpy(net.vars[v].value), tol=1e-4)
        assert fr["logits"] <= 1e-4, (tag, label, fr)
        bits[label] = (logits, nsplit)
    # the layers `want` leaves on fp32 keep their bits: where it wants none, the option changes nothing at all
    if bits["bf16x3"][1] == 0:
        assert np.array_equal(bits["bf16x3"][0], bits["fp32"][0])


def test_built_imdb_records_the_precision_and_the_default_refuses_it(gpu, tmp_path, want_everywhere):
    from mcncrossmodalemotions_amd import fetch_emovoxceleb_imdb as fe
    from test_gpu_imdb import framed_imdb, small_teacher
    imdb, frames = framed_imdb(3, 5, frameSize=(80, 72), min_seconds=1.0, max_seconds=1.5)
    d = str(tmp_path)
    built = fe.fetch_emovoxceleb_imdb("tiny-bf16x3", d, net=small_teacher(), imdb=imdb, frames=frames, batchSize=16,
                                      verbose=False, teacherPrecision="bf16x3")
    assert built.precision == "bf16x3" and sum(c.shape[0] for c in built.wavLogits) == len(imdb.images["denseFrames"])
    assert fe.load_imdb(fe.getImdbPath(d, "tiny-bf16x3")).precision == "bf16x3"
    fe._CACHE.pop(("tiny-bf16x3", os.path.abspath(d)))
    with pytest.raises(ValueError, match="'bf16x3'.*'fp32'"):
        fe.fetch_emovoxceleb_imdb("tiny-bf16x3", d, verbose=False)
    plain = fe.buildImdb(small_teacher(), imdb, frames, batchSize=16)
    assert plain.precision == "fp32"
    a, b = np.concatenate(built.wavLogits, 0), np.concatenate(plain.wavLogits, 0)
    assert a.shape == b.shape and not np.array_equal(a, b)
    assert float(np.abs(a - b).max()) <= TOL * max(1.0, float(np.abs(b).max()))

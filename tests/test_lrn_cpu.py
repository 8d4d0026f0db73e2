"""CPU: everything about the VGG face teachers that is host data.  The fp64 restatement of vl_nnnormalize that the GPU
tests compare against (tests/lrn_ref.py) is itself checked here, against torch's local_response_norm (forward, odd N) and
against central differences (backward); then the C ABI's argument checks, dagnn.LRN in model files, insertBNLayers, the
ferPlusZoo names and the geometry pins of the two VGG graphs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import lrn_ref as R
from test_matfile_cpu import assert_same_net

from mcncrossmodalemotions_amd import dagnn, matfile, zoo

XM_EINVAL = 1


# ---------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("C_,N", [cn for cn in R.WINDOW_CASES if cn[1] % 2 == 1])
def test_reference_forward_is_torch_lrn_for_odd_windows(C_, N):
    x, _ = R.case((3, 4, C_, 2), seed=100 * C_ + N)
    for param in (R.strong(N), R.strong(N, 0.5), [N, 2.0, 1e-4, 0.75]):
        _, kappa, alpha, beta = param
        t = torch.from_numpy(np.ascontiguousarray(x.astype(np.float64).transpose(3, 2, 0, 1)))       # S x C x H x W
        want = torch.nn.functional.local_response_norm(t, size=N, alpha=alpha * N, beta=beta, k=kappa).numpy()
        got = R.forward(x, param).transpose(3, 2, 0, 1)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("C_,N", R.WINDOW_CASES)
def test_reference_backward_is_the_derivative_of_its_forward(C_, N):
    """central differences of z = <dzdy, forward(x)> in fp64, step 1e-5: truncation ~ h^2 |f'''| / 6 ~ 1e-10 and rounding
    ~ 1e-16 * |z| / h ~ 1e-10, both far below the 1e-6 asked of it"""
    x, dzdy = R.case((2, 2, C_, 1), seed=7 * C_ + N)
    x, dzdy = x.astype(np.float64), dzdy.astype(np.float64)
    for param in (R.strong(N), [N, 2.0, 1e-2, 0.5]):
        dx = R.backward(x, param, dzdy)
        num = np.zeros_like(x)
        h = 1e-5
        for idx in np.ndindex(*x.shape):
            e = np.zeros_like(x)
            e[idx] = h
            num[idx] = ((dzdy * R.forward(x + e, param)).sum() - (dzdy * R.forward(x - e, param)).sum()) / (2 * h)
        assert np.abs(dx - num).max() <= 1e-6 * max(1.0, np.abs(num).max()), param


def test_a_mirrored_window_is_far_outside_the_gpu_tolerance():
    """the GPU tests could not tell G(k) = [k - m1, k + m2] from its mirror image if the two agreed within the tolerance:
    under the strong parameters every even-N case whose window leaves a channel out differs by more than 100 x the bound
    (VGG-M's own parameters move the result by < 1e-3, which is why the parity cases do not use them)"""
    even = [(C_, N) for C_, N in R.WINDOW_CASES if N % 2 == 0 and not R.covers_all(C_, N)]
    assert even == [(6, 4), (6, 2), (7, 6)]
    for C_, N in even:
        x, _ = R.case((5, 13, C_, 2), seed=C_ * 31 + N)
        ref = R.forward(x, R.strong(N))
        diff = np.abs(R.forward(x, R.strong(N), mirrored=True) - ref).max()
        assert diff > 100 * R.TOL * max(1.0, np.abs(ref).max()), (C_, N, diff)
        weak = np.abs(R.forward(x, [N] + R.VGG_M_PARAM[1:], mirrored=True) - R.forward(x, [N] + R.VGG_M_PARAM[1:])).max()
        assert 0 < weak < 10 * R.TOL
    assert R.covers_all(3, 8) and R.covers_all(1, 1) and not R.covers_all(3, 4)


# ------------------------------------------------------------------------------------------------------------- the C ABI
def test_abi_checks_arguments_without_a_device():
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    assert L.xm_version() >= 119
    for name in ("xm_nnnormalize_forward", "xm_nnnormalize_backward", "xm_nnnormalize_geometry"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    f = C.c_float
    one = C.c_void_p(16)         # never dereferenced: every call below returns before any device work
    other = C.c_void_p(32)
    fwd = lambda x, dims, N, y: L.xm_nnnormalize_forward(x, *dims, N, f(1), f(1), f(0.75), y, None)
    bwd = lambda x, d, dims, N, y: L.xm_nnnormalize_backward(x, d, *dims, N, f(1), f(1), f(0.75), y, None)
    assert fwd(one, (4, 4, 3, 2), 0, other) == XM_EINVAL and b"N must be a positive integer" in L.xm_last_error()
    assert bwd(one, one, (4, 4, 3, 2), -5, other) == XM_EINVAL and b"N must be a positive integer" in L.xm_last_error()
    assert fwd(one, (4, -1, 3, 2), 5, other) == XM_EINVAL and b"negative dimension" in L.xm_last_error()
    assert bwd(one, one, (4, 4, 3, -2), 5, other) == XM_EINVAL and b"negative dimension" in L.xm_last_error()
    assert fwd(None, (4, 4, 3, 2), 5, other) == XM_EINVAL and b"NULL tensor" in L.xm_last_error()
    assert fwd(one, (4, 4, 3, 2), 5, None) == XM_EINVAL and b"NULL tensor" in L.xm_last_error()
    assert bwd(one, None, (4, 4, 3, 2), 5, other) == XM_EINVAL and b"NULL tensor" in L.xm_last_error()
    assert fwd(one, (4, 4, 3, 2), 5, one) == XM_EINVAL and b"alias" in L.xm_last_error()
    assert bwd(one, other, (4, 4, 3, 2), 5, other) == XM_EINVAL and b"alias" in L.xm_last_error()
    for dims in ((0, 4, 3, 2), (4, 0, 3, 2), (4, 4, 0, 2), (4, 4, 3, 0)):          # the empty tensor: nothing to do
        assert fwd(None, dims, 5, None) == 0 and bwd(None, None, dims, 5, None) == 0
    g = [C.c_int(-1) for _ in range(3)]
    assert L.xm_nnnormalize_geometry(*[C.byref(v) for v in g]) == 0
    ppb, cpp, wir = (v.value for v in g)
    assert ppb > 0 and cpp >= 0 and wir >= 0 and (wir == 0 or wir >= 5)       # the register arm covers VGG-M's N = 5
    assert L.xm_nnnormalize_geometry(None, None, None) == 0


def test_cpu_tensors_are_refused():
    from mcncrossmodalemotions_amd import vl
    x = torch.zeros(2, 3, 2, 2).permute(3, 2, 1, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        vl.vl_nnnormalize(x, [5, 1, 1, 0.75])
    with pytest.raises(RuntimeError, match="no CPU path"):
        vl.vl_nnnormalize(x, [5, 1, 1, 0.75], x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dagnn.LRN().forward([x], [])


def test_profiler_rows_name_kernels_of_the_library():
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    syms = subprocess.run(["nm", "-C", _lib.SO_PATH], check=True, capture_output=True, text=True).stdout
    names = []
    for key in range(2500, 2600):
        buf = C.create_string_buffer(128)
        rc = L.xm_prof_kernel_name(key, buf, 128)
        assert (rc == 0) == (key < 2506), key
        if rc == 0:
            names.append(buf.value.decode())
            assert "xm::%s(" % names[-1] in syms, names[-1]
    assert len(set(names)) == 6 and all(n.startswith("lrn_") for n in names)


# ---------------------------------------------------------------------------------------------------- dagnn.LRN in a file
def _lrn_net():
    net = zoo.vgg_m_face(bn=False, num_classes=5, width_mult=1 / 16)
    net.initParams(3)
    return net


def test_lrn_block_defaults_and_round_trip(tmp_path):
    assert dagnn.LRN().param == [5, 1, 1e-4 / 5, 0.75]
    with pytest.raises(ValueError, match="four"):
        dagnn.LRN([5, 1, 1])
    net = _lrn_net()
    norms = [l for l in net.layers if isinstance(l.block, dagnn.LRN)]
    assert [l.name for l in norms] == ["norm1", "norm2"] and all(l.block.param == [5, 2, 1e-4, 0.75] for l in norms)
    assert not norms[0].params and norms[0].inputs == ["relu1"]
    path = str(tmp_path / "m.mat")
    dagnn.save_mat(net, path)
    assert_same_net(net, dagnn.load_mat(path))
    for column in (False, True):                       # block.param as MATLAB may hold it: 1 x 4 or 4 x 1
        s = net.saveobj()
        for i in range(s["layers"].shape[1]):
            if s["layers"][0, i]["type"] == "dagnn.LRN":
                p = np.array([7, 1.5, 0.25, 0.5], np.float64)
                s["layers"][0, i]["block"] = {"param": p.reshape((4, 1) if column else (1, 4))}
        matfile.write_mat(path, s)
        back = dagnn.load_mat(path)
        assert [l.block.param for l in back.layers if isinstance(l.block, dagnn.LRN)] == [[7, 1.5, 0.25, 0.5]] * 2
    s = net.saveobj()
    for i in range(s["layers"].shape[1]):
        if s["layers"][0, i]["type"] == "dagnn.LRN":
            s["layers"][0, i]["block"] = {"param": np.array([[5.0, 1.0, 1.0]])}
    matfile.write_mat(path, s)
    with pytest.raises(ValueError, match="norm1.*`param` has 3 values"):
        dagnn.load_mat(path)


def test_an_unknown_block_type_is_still_refused(tmp_path):
    net = _lrn_net()
    s = net.saveobj()
    for i in range(s["layers"].shape[1]):
        if s["layers"][0, i]["type"] == "dagnn.LRN":
            s["layers"][0, i]["type"] = "dagnn.SpatialNorm"
    path = str(tmp_path / "u.mat")
    matfile.write_mat(path, s)
    with pytest.raises(ValueError, match=r"block type 'dagnn.SpatialNorm' is not built \(.*dagnn\.LRN.*are\)"):
        dagnn.load_mat(path)


# ------------------------------------------------------------------------------------------------------- insertBNLayers
def _vd(seed=5):
    net = zoo.vgg_vd_face(width_mult=1 / 16, image_size=64)
    zoo.synthetic_pretrained(net, seed)
    zoo.prepareFromDagNN(net, 7, seed)
    zoo.configureForClassification(net, 0.1, 0.5, "distributions")
    return net


def _signature(net):
    return [(l.name, type(l.block).__name__, tuple(l.inputs), tuple(l.outputs), tuple(l.params)) for l in net.layers]


def test_insert_bn_layers_on_vgg_vd(tmp_path):
    net = _vd()
    before = _signature(net)
    filters = {p: net.params[p].value.copy() for p in net.params}
    net._flat = "stale"
    assert zoo.insertBNLayers(net) is net and net._flat is None
    bns = [l for l in net.layers if isinstance(l.block, dagnn.BatchNorm)]
    convs = [l for l in net.layers if isinstance(l.block, dagnn.Conv)]
    assert len(bns) == 15 and len(convs) == 16 and len(net.layers) == len(before) + 15
    assert convs[-1].outputs == ["prediction"] and not any(b.inputs == ["prediction"] for b in bns)
    order = [l.name for l in net.layers]
    for cv in convs[:-1]:
        i = order.index(cv.name)
        bn, nxt = net.layers[i + 1], net.layers[i + 2]
        assert bn.name == cv.name + "_bn" and bn.inputs == cv.outputs and bn.outputs == [cv.name + "_bn"]
        assert bn.params == [bn.name + s for s in ("_mult", "_bias", "_moments")]
        assert bn.block.numChannels == cv.block.size[3]
        assert isinstance(nxt.block, dagnn.ReLU) and nxt.inputs == bn.outputs          # conv -> bn -> relu
        assert [q.name for q in net.layers if cv.outputs[0] in q.inputs] == [bn.name]  # every consumer was rewired
        assert cv.block.hasBias and len(cv.params) == 2                                # the biases stay
    # values and rates: what addLayer + initParams give a BatchNorm anywhere else in the package
    fresh = dagnn.DagNN()
    fresh.addLayer("bn", dagnn.BatchNorm(bns[0].block.numChannels), "x", "y", ["g", "b", "m"])
    fresh.initParams(0)
    for got, want in zip(bns[0].params, ["g", "b", "m"]):
        p, q = net.params[got], fresh.params[want]
        assert np.array_equal(p.value, q.value) and p.value.dtype == q.value.dtype
        assert (p.learningRate, p.weightDecay, p.trainMethod) == (q.learningRate, q.weightDecay, q.trainMethod)
    assert bns[0].block.epsilon == fresh.layers[0].block.epsilon
    for p, v in filters.items():                                     # nothing else was re-initialised
        assert np.array_equal(net.params[p].value, v), p
    assert net.params["conv1_1f"].learningRate == 0.1                # configureForClassification's rates are kept
    assert net.getInputs() == ["data", "label", "hardlabel"] and net.getOutputs() == ["objective", "classerror"]
    once = _signature(net)
    zoo.insertBNLayers(net)                                          # a second call changes nothing
    assert _signature(net) == once
    path = str(tmp_path / "bn.mat")
    dagnn.save_mat(net, path)
    assert_same_net(net, dagnn.load_mat(path))


def test_insert_bn_layers_leaves_networks_with_batch_norm_alone():
    for net in (zoo.resnet50(width_mult=1 / 16, blocks=(1, 1, 1, 1)), zoo.vgg_m_face(bn=True, width_mult=1 / 16)):
        before, params = _signature(net), list(net.params)
        zoo.insertBNLayers(net)
        assert _signature(net) == before and list(net.params) == params


# ------------------------------------------------------------------------------------------------------ ferPlusZoo names
def test_ferpluszoo_builds_the_vgg_names():
    kw = dict(width_mult=1 / 16, seed=3)
    for name in ("vgg-vd-face", "vgg_face"):
        plain = zoo.ferPlusZoo(name, image_size=64, dropoutRate=0.5, **kw)
        withbn = zoo.ferPlusZoo(name, image_size=64, dropoutRate=0.5, useBnorm=1, **kw)
        count = lambda n, cls: sum(isinstance(l.block, cls) for l in n.layers)
        assert count(plain, dagnn.BatchNorm) == 0 and count(withbn, dagnn.BatchNorm) == 15
        assert count(plain, dagnn.DropOut) == 2                       # its own dropout6 / dropout7; none is added
        for net in (plain, withbn):
            assert net.getInputs() == ["data", "label", "hardlabel"] and net.getOutputs() == ["objective", "classerror"]
            assert net.getLayer("fc8").block.size == (1, 1, 256, 7) and net.getLayer("fc8").outputs == ["prediction"]
            assert net.meta["normalization"] == {"imageSize": [64, 64, 3], "averageImage": [129.1863, 104.7624, 93.5940]}
            assert net.meta["modelName"] == name
    a = zoo.ferPlusZoo("vgg-m-face-bn", **kw)
    b = zoo.ferPlusZoo("vgg-m-face-bn", useBnorm=1, **kw)
    assert _signature(a) == _signature(b) and sum(isinstance(l.block, dagnn.BatchNorm) for l in a.layers) == 7
    assert a.getOutputs() == ["objective", "classerror"] and a.getLayer("fc8").block.size[3] == 7
    assert zoo.ferPlusZoo("vgg-vd-face", numOutputs=8, image_size=32, **kw).getLayer("fc8").block.size[3] == 8
    for name, nbn in (("vgg-vd-face-fer", 0), ("vgg-m-face-bn-fer", 7)):       # the pretrained FER stand-ins
        net = zoo.ferPlusZoo(name, useBnorm=1, dropoutRate=0.5, **kw)
        assert net.getInputs() == ["data"] and net.getOutputs() == ["prediction"]
        assert not any(isinstance(l.block, (dagnn.LossBase, dagnn.SoftMax)) for l in net.layers)
        assert net.getLayer("fc8").block.size[3] == 7 and net.params["fc8f"].value.shape[3] == 7
        assert sum(isinstance(l.block, dagnn.BatchNorm) for l in net.layers) == nbn
        assert net.meta["normalization"]["imageSize"] == [224, 224, 3]
    for name in ("vgg-vd-face-sfew", "vgg-vd-face-sfew-dag", "resnet50-face-sfew", "alexnet"):
        with pytest.raises(ValueError, match="not a recognised FER\\+ teacher"):
            zoo.ferPlusZoo(name)


def test_ferpluszoo_from_a_model_file_inserts_batch_norm_when_asked(tmp_path):
    raw = zoo.vgg_vd_face(width_mult=1 / 16, image_size=32)
    zoo.synthetic_pretrained(raw, 1)
    dagnn.save_mat(raw, str(tmp_path / "vgg-vd-face.mat"))
    fer = zoo.vgg_m_face(bn=False, num_classes=7, width_mult=1 / 16)
    zoo.synthetic_pretrained(fer, 2)
    dagnn.save_mat(fer, str(tmp_path / "vgg-m-face-bn-fer.mat"))
    count = lambda n: sum(isinstance(l.block, dagnn.BatchNorm) for l in n.layers)
    plain = zoo.ferPlusZoo("vgg-vd-face", modelDir=tmp_path, dropoutRate=0.5)
    withbn = zoo.ferPlusZoo("vgg-vd-face", modelDir=tmp_path, dropoutRate=0.5, useBnorm=1)
    assert count(plain) == 0 and count(withbn) == 15 and len(withbn.layers) == len(plain.layers) + 15
    assert withbn.getInputs() == ["data", "label", "hardlabel"] and withbn.getOutputs() == ["objective", "classerror"]
    for p in plain.params:                         # the file's weights are kept
        assert np.array_equal(plain.params[p].value, withbn.params[p].value), p
    # a pretrained name returns as loaded, LRN layers and softmax included, whatever useBnorm says
    loaded = zoo.ferPlusZoo("vgg-m-face-bn-fer", modelDir=tmp_path, useBnorm=1)
    assert count(loaded) == 0 and [l.name for l in loaded.layers if isinstance(l.block, dagnn.LRN)] == ["norm1", "norm2"]
    assert loaded.getInputs() == ["data"] and loaded.getOutputs() == ["prob"]


# --------------------------------------------------------------------------------------------------------- geometry pins
def _sizes(net, size):
    """output size of every layer for a size x size input, down the chain with the library's xm_out_size"""
    from mcncrossmodalemotions_amd import vl
    out, hw = {}, size
    for l in net.layers:
        b = l.block
        if isinstance(b, dagnn.Conv):
            p = vl._pad4(b.pad)
            assert p[0] == p[2] and p[1] == p[3] and b.size[0] == b.size[1] and b.stride[0] == b.stride[1]
            hw = vl.out_size(hw, p[0], p[1], b.size[0], b.dilate[0], b.stride[0])
        elif isinstance(b, dagnn.Pooling):
            p = vl._pad4(b.pad)
            assert p[0] == p[2] and p[1] == p[3] and b.poolSize[0] == b.poolSize[1]
            hw = vl.out_size(hw, p[0], p[1], b.poolSize[0], 1, vl._pair(b.stride, "STRIDE")[0])
        out[l.name] = hw
    return out


def test_geometry_pins():
    vd = _sizes(zoo.vgg_vd_face(width_mult=1 / 64), 224)
    assert [vd["pool%d" % i] for i in range(1, 6)] == [112, 56, 28, 14, 7] and vd["fc6"] == 1 and vd["prob"] == 1
    net = zoo.vgg_vd_face(width_mult=1 / 64)
    assert net.getLayer("fc6").block.size[:2] == (7, 7)
    assert [l.block.size[3] for l in zoo.vgg_vd_face(num_classes=4).layers if isinstance(l.block, dagnn.Conv)] == \
        [64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512, 4096, 4096, 4]
    assert _sizes(zoo.vgg_vd_face(width_mult=1 / 64, image_size=64), 64)["fc6"] == 1
    with pytest.raises(ValueError, match="multiple of 32"):
        zoo.vgg_vd_face(image_size=100)
    for bn in (True, False):
        m = _sizes(zoo.vgg_m_face(bn=bn, width_mult=1 / 64), 224)
        assert (m["conv1"], m["pool1"], m["conv2"], m["pool2"], m["conv5"], m["pool5"], m["fc6"], m["fc8"]) == \
            (109, 54, 26, 13, 13, 6, 1, 1)
    full = zoo.vgg_m_face(bn=False, width_mult=1 / 64)
    assert full.getLayer("fc6").block.size[:2] == (6, 6)
    names = [l.name for l in full.layers]
    assert names[:8] == ["conv1", "relu1", "norm1", "pool1", "conv2", "relu2", "norm2", "pool2"]

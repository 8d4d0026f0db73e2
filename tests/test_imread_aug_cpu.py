"""CPU: the host side of vl.vl_imreadjpeg -- xm_imread_plan -- and a float64 numpy restatement of DESIGN section 24
(window, weights, clamped taps, flip, colour) that tests/test_gpu_imread_aug.py imports as its reference.
  * xm_imread_plan, through ctypes and without a device, equals the restatement's output sizes, windows, tap counts and
    colour terms over sizes {1, 2, 3, 17, 37} x {1, 3, 23, 53}, outputs 1 x 1, 5 x 7, 16 x 20, a scalar Resize and none,
    every filter, both antialias values, both crop locations and the anisotropy and size ranges;
  * every refusal comes with its message before a device is needed;
  * PIL's 'F'-mode resize(box=) is a second opinion on the weights where every tap is in bounds;
  * tests/imread_plan_check.cpp -- the header alone -- is built with the address and undefined-behaviour sanitizers and run
    as a program of its own;
  * the three entries are declared, typed and exported.
Nothing here opens a device."""
import ctypes as C
import io
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ETOOBIG, ENOTSUP = 1, 4, 5
FILTERS = {"box": 0, "bilinear": 1, "bicubic": 2}
SUPPORT = {"box": 1.0, "bilinear": 2.0, "bicubic": 4.0}
U24 = 2.0 ** -24
DEFAULT_DRAWS = np.array([0.5] * 7 + [0.0] * 3)


# ---- the restatement (float64) ----------------------------------------------------------------------------------------
def kern(name, t):
    t = np.asarray(t, np.float64)
    a = np.abs(t)
    if name == "box":
        return ((t > -0.5) & (t <= 0.5)).astype(np.float64)
    if name == "bilinear":
        return np.maximum(0.0, 1.0 - a)
    return np.where(a <= 1, (1.5 * a - 2.5) * a * a + 1, np.where(a < 2, ((-0.5 * a + 2.5) * a - 4) * a + 2, 0.0))


def ref_plan(H, W, o, u=DEFAULT_DRAWS):
    """o: dict(resize None | S | (Ho, Wo), aniso (amin, amax), size (smin, smax), random, flip, filter, antialias,
    contrast, saturation, brightness 3 x 3); u: the image's ten draws.  Returns the planned quantities as a dict."""
    resize = o.get("resize")
    if resize is None:
        Ho, Wo = H, W
    elif np.ndim(resize) == 0:
        S = int(resize)
        other = max(1, int(np.floor(S * max(H, W) / min(H, W) + 0.5)))
        Ho, Wo = (S, other) if H <= W else (other, S)
    else:
        Ho, Wo = int(resize[0]), int(resize[1])
    amin, amax = o.get("aniso", (0.0, 0.0))
    ch0, cw0 = float(H), float(W)
    if not (amin == 0 and amax == 0):
        a = amin + u[0] * (amax - amin)
        rho = a * float(Wo) / float(Ho)
        if H * rho <= W:
            cw0 = H * rho
        else:
            ch0 = W / rho
    smin, smax = o.get("size", (1.0, 1.0))
    s = smin + u[1] * (smax - smin)
    ch, cw = s * ch0, s * cw0
    rnd = bool(o.get("random", False))
    y0, x0 = (u[2] if rnd else 0.5) * (H - ch), (u[3] if rnd else 0.5) * (W - cw)
    flip = bool(o.get("flip", False)) and u[4] < 0.5
    name, aa = o.get("filter", "bilinear"), bool(o.get("antialias", False))
    ry, rx = ch / Ho, cw / Wo
    sy, sx = (max(ry, 1.0), max(rx, 1.0)) if aa else (1.0, 1.0)
    Ty, Tx = int(np.ceil(SUPPORT[name] * sy)) + 1, int(np.ceil(SUPPORT[name] * sx)) + 1
    Cc, Ss = float(o.get("contrast", 0.0)), float(o.get("saturation", 0.0))
    gamma, sigma = 1 - Cc + 2 * Cc * u[5], 1 - Ss + 2 * Ss * u[6]
    B = np.asarray(o.get("brightness", np.zeros((3, 3))), np.float64)
    b = B @ np.asarray(u[7:10], np.float64)
    A = sigma * np.eye(3) + (1 - sigma) / 3 * np.ones((3, 3))
    return dict(H=H, W=W, Ho=Ho, Wo=Wo, y0=y0, x0=x0, ch=ch, cw=cw, flip=flip, filter=name, antialias=aa, ry=ry, rx=rx, sy=sy,
                sx=sx, Ty=Ty, Tx=Tx, gamma=gamma, sigma=sigma, b=b, A=A, M=gamma * A, contrast_on=Cc > 0)


def axis_taps(name, n, m, c0, length, s, flip=False):
    """(first (m,), weights (m, T), clamped indices (m, T)) of an axis with n inputs and m outputs over window (c0, length)"""
    r = length / m
    T = int(np.ceil(SUPPORT[name] * s)) + 1
    o = np.arange(m)
    op = (m - 1 - o) if flip else o
    u = c0 + (op + 0.5) * r - 0.5
    first = np.floor(u - SUPPORT[name] * s / 2).astype(np.int64) + 1
    taps = first[:, None] + np.arange(T)[None, :]
    w = kern(name, (taps - u[:, None]) / s)
    w = w / w.sum(1, keepdims=True)
    return first, w, np.clip(taps, 0, n - 1)


def axis_matrix(name, n, m, c0, length, s, flip=False):
    first, w, idx = axis_taps(name, n, m, c0, length, s, flip)
    A = np.zeros((m, n))
    np.add.at(A, (np.arange(m)[:, None].repeat(w.shape[1], 1), idx), w)
    Aabs = np.zeros((m, n))
    np.add.at(Aabs, (np.arange(m)[:, None].repeat(w.shape[1], 1), idx), np.abs(w))
    return A, Aabs, first


def ref_apply(img, p, avg=None):
    """img H x W x 3 (0..255) and a ref_plan -> (out Ho x Wo x 3 float64, tolerance Ho x Wo x 3, resampled p before colour).
    The tolerance is the derived one: (Ty + Tx + 4) 2^-24 sum |wy| |wx| |p| per pixel and channel; with colour options the
    same factor times the colour terms' absolute sum, plus, with Contrast, the bound of the Ho Wo-term fp32 sum behind mu."""
    img = np.asarray(img, np.float64)
    Ay, Ay_abs, _ = axis_matrix(p["filter"], p["H"], p["Ho"], p["y0"], p["ch"], p["sy"])
    Ax, Ax_abs, _ = axis_matrix(p["filter"], p["W"], p["Wo"], p["x0"], p["cw"], p["sx"], p["flip"])
    res = np.stack([Ay @ img[:, :, c] @ Ax.T for c in range(3)], 2)
    mag = np.stack([Ay_abs @ np.abs(img[:, :, c]) @ Ax_abs.T for c in range(3)], 2)
    factor = (p["Ty"] + p["Tx"] + 4) * U24
    a = np.zeros(3) if avg is None else np.asarray(avg, np.float64)
    colour = avg is not None or p["contrast_on"] or p["sigma"] != 1 or p["gamma"] != 1 or np.any(p["b"] != 0)
    if not colour:
        return res, factor * mag, res
    p1 = res - a + p["b"]
    mag1 = mag + np.abs(a) + np.abs(p["b"])
    mu = p1.mean((0, 1))
    p2 = p["gamma"] * p1 + (1 - p["gamma"]) * mu
    p3 = p["sigma"] * p2 + (1 - p["sigma"]) * p2.mean(2, keepdims=True)
    tol = factor * (mag1 @ np.abs(p["M"]).T + abs(1 - p["gamma"]) * (np.abs(p["A"]) @ mag1.mean((0, 1))))
    if p["contrast_on"]:
        tol = tol + abs(1 - p["gamma"]) * (np.abs(p["A"]) @ (p["Ho"] * p["Wo"] * U24 * mag1.mean((0, 1))))
    return p3, tol, res


# ---- the plan through ctypes -------------------------------------------------------------------------------------------
def opts_vector(o):
    v = np.zeros(24)
    resize = o.get("resize")
    if resize is not None:
        v[0:3] = (2, resize, 0) if np.ndim(resize) == 0 else (1, resize[0], resize[1])
    v[3:5] = o.get("aniso", (0.0, 0.0))
    v[5:7] = o.get("size", (1.0, 1.0))
    v[7], v[8] = bool(o.get("random", False)), bool(o.get("flip", False))
    v[9], v[10] = FILTERS[o.get("filter", "bilinear")], bool(o.get("antialias", False))
    v[11], v[12] = o.get("contrast", 0.0), o.get("saturation", 0.0)
    v[13:22] = np.asarray(o.get("brightness", np.zeros((3, 3))), np.float64).reshape(-1)
    v[22] = o.get("avg", 0)
    return v


def c_plan(hw, o, draws=None):
    """xm_imread_plan on plain host memory -> (rc, rows N x 44, sizes, message)"""
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    hw = np.ascontiguousarray(hw, np.int64).reshape(-1, 3)
    N = hw.shape[0]
    v = opts_vector(o) if isinstance(o, dict) else np.ascontiguousarray(o, np.float64)
    rows = np.full((max(N, 1), 44), -7.0)
    sizes = np.full(8, -7, np.int64)
    d = None if draws is None else np.ascontiguousarray(draws, np.float64)
    rc = L.xm_imread_plan(C.c_void_p(hw.ctypes.data), N, C.c_void_p(v.ctypes.data), None if d is None else C.c_void_p(d.ctypes.data),
                          C.c_void_p(rows.ctypes.data), C.c_void_p(sizes.ctypes.data))
    return rc, rows[:N], sizes, L.xm_last_error().decode()


def jpeg_bytes(arr, quality=92):
    from PIL import Image
    fh = io.BytesIO()
    Image.fromarray(np.asarray(arr, np.uint8)).save(fh, "JPEG", quality=quality)
    return fh.getvalue()


def test_symbols_are_declared_typed_and_exported():
    import torch
    from mcncrossmodalemotions_amd import _lib, vl
    before = torch.cuda.is_initialized()
    L = _lib.load()
    assert L.xm_version() >= 125
    hdr = open(os.path.join(ROOT, "include", "xmodal.h")).read()
    assert "125 = + xm_imread_plan, xm_imread_transform_batch, xm_imread_geometry, xm_imread_round_u8" in hdr
    for name, nargs in (("xm_imread_plan", 6), ("xm_imread_transform_batch", 7), ("xm_imread_geometry", 4),
                        ("xm_imread_round_u8", 4)):
        assert "int %s(" % name in hdr
        assert len(_lib.SIGNATURES[name]) == nargs and getattr(L, name).restype is C.c_int
    assert "enum { XM_IMREAD_ROW = 44, XM_IMREAD_OPTS = 24, XM_IMREAD_DRAWS = 10, XM_IMREAD_SIZES = 8 };" in hdr
    assert (vl.IMREAD_ROW, vl.IMREAD_OPTS, vl.IMREAD_DRAWS, vl.IMREAD_SIZES) == (44, 24, 10, 8)
    launches, with_contrast, tile_rows, tile_cols = vl.imread_geometry()
    assert (launches, with_contrast) == (2, 3) and tile_rows * tile_cols * 3 * 4 <= 160 * 1024 and tile_rows >= 258
    assert L.xm_imread_geometry(None, None, None, None) == 0
    # the device entry checks its arguments before any device call
    fn = L.xm_imread_transform_batch
    assert fn(None, None, 0, None, None, None, None) == 0
    assert fn(None, None, -1, None, None, None, None) == EINVAL
    assert fn(None, None, 1, None, None, None, None) == EINVAL and "NULL" in L.xm_last_error().decode()
    host = np.zeros(64, np.float64)                                        # host memory: never dereferenced as a device pointer
    a = host.ctypes.data
    rc, rows, _, _ = c_plan([[8, 8, 0]], dict(resize=(4, 4)))
    assert rc == 0
    assert fn(C.c_void_p(a + 2), C.c_void_p(a), 1, C.c_void_p(rows.ctypes.data), None, C.c_void_p(a), None) == EINVAL
    assert "aligned" in L.xm_last_error().decode()
    bad = rows.copy()
    bad[0, 13] += 1                                                        # a tap count the plan would not write
    assert fn(C.c_void_p(a), C.c_void_p(a), 1, C.c_void_p(bad.ctypes.data), None, C.c_void_p(a), None) == EINVAL
    assert "row 0" in L.xm_last_error().decode()
    sub = c_plan([[8, 8, 0]], dict(resize=(4, 4), avg=1))[1]
    assert fn(C.c_void_p(a), C.c_void_p(a), 1, C.c_void_p(sub.ctypes.data), None, C.c_void_p(a), None) == EINVAL
    assert "avg is NULL" in L.xm_last_error().decode()
    assert torch.cuda.is_initialized() == before


SIZES = [(H, W) for H in (1, 2, 3, 17, 37) for W in (1, 3, 23, 53)]
RESIZES = [(1, 1), (5, 7), (16, 20), 8, None]
RANGES = [dict(), dict(aniso=(0.75, 4 / 3), size=(0.35, 1.0)), dict(aniso=(1.0, 1.0), size=(0.625, 0.625))]


@pytest.mark.parametrize("name", list(FILTERS))
def test_plan_equals_the_restatement(name):
    rng = np.random.default_rng(5)
    hw = np.array([(H, W, 1000 * k) for k, (H, W) in enumerate(SIZES)], np.int64)
    cases = 0
    for resize, aa, rnd, rg, flip in itertools.product(RESIZES, (False, True), (False, True), RANGES, (False, True)):
        B = np.diag([2.0, 3.0, 1.0]) + 0.25
        o = dict(resize=resize, filter=name, antialias=aa, random=rnd, flip=flip, contrast=0.4, saturation=0.3, brightness=B, **rg)
        draws = np.concatenate([rng.random((len(SIZES), 7)), rng.standard_normal((len(SIZES), 3))], 1)
        rc, rows, sizes, msg = c_plan(hw, o, draws)
        assert rc == 0, msg
        out = tab = part = 0
        for k, ((H, W), d) in enumerate(zip(SIZES, rows)):
            p = ref_plan(H, W, o, draws[k])
            assert (d[0], d[1], d[2], d[3], d[4], d[5]) == (H, W, 1000 * k, p["Ho"], p["Wo"], out), (k, o)
            np.testing.assert_allclose(d[6:10], [p["y0"], p["x0"], p["ch"], p["cw"]], rtol=1e-14, atol=1e-14)
            assert -1e-12 <= d[6] and d[6] + d[8] <= H + 1e-12 and -1e-12 <= d[7] and d[7] + d[9] <= W + 1e-12
            assert (d[10], d[11], d[12], d[13], d[14]) == (p["flip"], FILTERS[name], aa, p["Ty"], p["Tx"]), (k, o)
            np.testing.assert_allclose(d[15:24].reshape(3, 3), p["M"], rtol=1e-14, atol=1e-15)
            np.testing.assert_allclose(d[24:27], p["M"] @ p["b"], rtol=1e-13, atol=1e-14)
            np.testing.assert_allclose([d[27], d[28]], [p["gamma"], p["sigma"]], rtol=1e-15)
            np.testing.assert_allclose(d[29:32], p["b"], rtol=1e-14, atol=1e-15)
            np.testing.assert_allclose(d[34:38], [p["ry"], p["rx"], p["sy"], p["sx"]], rtol=1e-14)
            assert (d[32], d[38], d[39], d[40], d[41]) == (tab, -(-p["Wo"] // 8), part, 0, 1)
            assert 1 <= d[33] <= p["Ho"]
            out += 3 * p["Ho"] * p["Wo"]
            tab += p["Ho"] * p["Ty"] + p["Wo"] * p["Tx"] + p["Ho"] + p["Wo"]
            part += 3 * -(-p["Wo"] // 8)
            cases += 1
        uniform = resize is not None and np.ndim(resize) != 0
        assert list(sizes) == [out, tab, part, max(-(-int(r[4]) // 8) for r in rows), 1, int(uniform),
                               max(int(max(r[3], r[4])) for r in rows), len(SIZES)]
    assert cases == 20 * 5 * 2 * 2 * 3 * 2
    # no random option: no draws are needed, and the defaults are the centre window of the whole image
    rc, rows, sizes, _ = c_plan(hw, dict(resize=(5, 7), filter=name))
    assert rc == 0 and sizes[4] == 0
    for (H, W), d in zip(SIZES, rows):
        assert (d[6], d[7], d[8], d[9], d[10], d[27], d[28]) == (0, 0, H, W, 0, 1, 1)
        assert np.array_equal(d[15:24].reshape(3, 3), np.eye(3)) and not d[24:27].any()
    assert c_plan(np.zeros((0, 3), np.int64), dict())[0] == 0


def test_draws_follow_the_documented_order_and_options_do_not_move_them():
    from mcncrossmodalemotions_amd import vl
    d = vl.imread_draws(np.random.default_rng(11), 6)
    g = np.random.default_rng(11)
    U = g.random((6, 7))
    G = g.standard_normal((6, 3))
    assert d.shape == (6, 10) and np.array_equal(d[:, :7], U) and np.array_equal(d[:, 7:], G)
    hw = [[37, 53, 0]] * 6
    base = dict(resize=(16, 20), random=True, size=(0.35, 1.0), aniso=(0.75, 4 / 3))
    plain, flipped = c_plan(hw, base, d)[1], c_plan(hw, dict(flip=True, **base), d)[1]
    assert np.array_equal(plain[:, 6:10], flipped[:, 6:10]) and not plain[:, 10].any()
    assert list(flipped[:, 10]) == list((U[:, 4] < 0.5).astype(float)) and 0 < flipped[:, 10].sum() < 6


def test_each_refusal_has_its_message_before_a_device_is_needed():
    import torch
    from mcncrossmodalemotions_amd import _lib, vl
    before = torch.cuda.is_initialized()
    rng = np.random.default_rng(3)
    small, wide, tall = (jpeg_bytes(rng.integers(0, 256, s + (3,))) for s in ((17, 23), (16, 40), (200, 8)))
    g = np.random.default_rng(0)
    for size in (0.0, 1.5, [0.5, 1.2], [-0.1, 0.5]):
        with pytest.raises(_lib.XmError, match=r"CropSize .* outside \(0, 1\]"):
            vl.vl_imreadjpeg([small], "CropSize", size, "Resize", [8, 8], rng=g)
    with pytest.raises(_lib.XmError, match="CropAnisotropy .* minimum is above the maximum"):
        vl.vl_imreadjpeg([small], "CropAnisotropy", [1.5, 0.75], "Resize", [8, 8], rng=g)
    with pytest.raises(_lib.XmError, match="image 2: .* reduces by more than 64"):
        vl.vl_imreadjpeg([small, wide, tall, small], "Resize", [2, 2])
    rc, _, _, msg = c_plan([[17, 23, 0], [16, 40, 2000], [200, 8, 5000]], dict(resize=(2, 2)))
    assert rc == ENOTSUP and "image 2:" in msg
    assert c_plan([[128, 8, 0]], dict(resize=(2, 2)))[0] == 0                # exactly 64 is served
    with pytest.raises(ValueError, match="'Pack' needs outputs of one size"):
        vl.vl_imreadjpeg([small, wide], "Pack", "Resize", 8)
    with pytest.raises(ValueError, match="'Pack' needs outputs of one size"):
        vl.vl_imreadjpeg([small, wide], "pack")
    with pytest.raises(ValueError, match="unknown option 'Rotate'"):
        vl.vl_imreadjpeg([small], "Resize", [8, 8], "Rotate", 3)
    with pytest.raises(ValueError, match="'Prefetch' is not supported"):
        vl.vl_imreadjpeg([small], "Prefetch")
    with pytest.raises(ValueError, match="needs rng"):
        vl.vl_imreadjpeg([small], "Flip", "Resize", [8, 8])
    with pytest.raises(ValueError, match="needs a value"):
        vl.vl_imreadjpeg([small], "Resize")
    with pytest.raises(ValueError, match="Interpolation must be"):
        vl.vl_imreadjpeg([small], "Interpolation", "lanczos")
    with pytest.raises(ValueError, match="CropLocation must be"):
        vl.vl_imreadjpeg([small], "CropLocation", "corner")
    # names without regard to case; NumThreads, Gpu and Verbose are accepted and ignored
    opt = vl.imread_options(["PACK", "resize", [8, 8], "NumThreads", 12, "gpu", "VERBOSE", "flip", False, "cropSIZE", 0.5])
    assert opt == dict(pack=True, resize=[8, 8], numthreads=12, gpu=True, verbose=True, flip=False, cropsize=0.5)
    v, avg = vl.imread_opts_vector(opt, antialias=True)
    assert list(v[:11]) == [1, 8, 8, 0, 0, 0.5, 0.5, 0, 0, 1, 1] and avg is None and not vl.imread_random(v)
    v, avg = vl.imread_opts_vector(vl.imread_options(["Brightness", [1, 2, 3], "SubtractAverage", [1, 2, 3], "Resize", 9]))
    assert np.array_equal(v[13:22].reshape(3, 3), np.diag([1.0, 2, 3])) and v[22] == 1 and list(v[:2]) == [2, 9] and vl.imread_random(v)
    # the plan's own refusals
    for o, what in ((dict(contrast=1.5), "Contrast"), (dict(saturation=-0.1), "Saturation"), (dict(aniso=(-1.0, 1.0)), "CropAnisotropy"),
                    (dict(flip=True), "needs the draws"), (dict(resize=(0, 4)), "positive integers")):
        rc, _, _, msg = c_plan([[8, 8, 0]], o)
        assert rc == EINVAL and what in msg, (o, msg)
    rc, _, _, msg = c_plan([[8, 8, 0], [8, 9, 192]], dict(avg=2))
    assert rc == EINVAL and "one size" in msg
    assert c_plan([[8, 40000, 0]], dict())[0] == EINVAL and c_plan([[8, 8, 0]], dict(resize=(4, 40000)))[0] == ETOOBIG
    assert torch.cuda.is_initialized() == before


@pytest.mark.parametrize("name", ["bilinear", "bicubic"])
@pytest.mark.parametrize("size", [(16, 20), (64, 80)])
def test_pil_is_a_second_opinion_on_the_weights(name, size):
    from PIL import Image
    H, W, (Ho, Wo) = 37, 53, size
    y0, x0, ch, cw = 3.25, 5.5, 30.0, 41.0
    img = np.random.default_rng(9).integers(0, 256, (H, W)).astype(np.float32)
    pil = Image.fromarray(img, mode="F").resize((Wo, Ho), resample=getattr(Image, name.upper()), box=(x0, y0, x0 + cw, y0 + ch))
    p = ref_plan(H, W, dict(resize=size, filter=name, antialias=True))
    p.update(y0=y0, x0=x0, ch=ch, cw=cw, ry=ch / Ho, rx=cw / Wo, sy=max(ch / Ho, 1.0), sx=max(cw / Wo, 1.0))
    ours = ref_apply(np.repeat(img[:, :, None], 3, 2), p)[0][:, :, 0]
    fy, wy, _ = axis_taps(name, H, Ho, y0, ch, p["sy"])
    fx, wx, _ = axis_taps(name, W, Wo, x0, cw, p["sx"])
    def in_bounds(first, w, n):                                            # every tap that carries weight lies inside the image
        taps = first[:, None] + np.arange(w.shape[1])[None, :]
        return ((w == 0) | ((taps >= 0) & (taps <= n - 1))).all(1)
    inside = in_bounds(fy, wy, H)[:, None] & in_bounds(fx, wx, W)[None, :]
    assert inside.all()                                                    # the window was chosen so that this holds everywhere
    # PIL rounds the horizontal pass and the result to float32: 2^-25 of at most L^2 255 each, L = 1.25 the largest
    # absolute weight sum of the Keys kernel -> 2^-24 * 1.5625 * 255 = 2.4e-5
    worst = np.abs(np.asarray(pil, np.float64) - ours).max()
    print("PIL %s %dx%d: worst difference %.3g" % (name, Ho, Wo, worst))
    assert worst <= U24 * 1.5625 * 255


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_plan_header_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "imread_plan_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "imread_plan_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout.strip())
    plans, images, samples, chunks, maxrows, refusals = (int(w) for w in r.stdout.split())
    geo_rows = 341
    assert plans == images + refusals and images > 10000 and samples > 10 ** 6 and refusals > 0
    assert chunks > images and 258 <= maxrows <= geo_rows                  # some windows were walked in several chunks

"""CPU: a numpy restatement of the baseline JPEG decode behind vl.imreadjpeg (fetch_emovoxceleb_imdb.m:160-172,
compute_visual_feats.m:130-143) -- parse, Huffman, dequantisation, libjpeg's ISLOW integer IDCT, fancy chroma
upsampling, 16-bit fixed-point YCbCr -> RGB -- equal to PIL's pixels on every fixture of tests/golden/jpeg_small.npz
(and, with PIL at hand, on regenerated fixtures and random sizes); xm_jpeg_plan through ctypes without a device against
the restatement's parse and tables; the ABI of the two new entries.  The GPU tests import the restatement from here."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_small.npz")
NEW_ABI = ["xm_jpeg_plan", "xm_jpeg_decode_batch"]
DESC, LANE, QT_BYTES, HT_BYTES = 24, 4, 128, 1024                 # the layout documented in include/xmodal.h

# jpeg_natural_order: zigzag position -> row-major position in the 8 x 8 block
NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7,
                    14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39,
                    46, 53, 60, 61, 54, 47, 55, 62, 63])


class Unsupported(Exception):
    pass


class Malformed(Exception):
    pass


# ------------------------------------------------------------------------------------------------ parse
def parse(data):
    """the headers of one file: H, W, components [(hs, vs, tq, td, ta)], qt {id: 64 natural-order ints}, dht {(class,
    id): (counts 16, values)}, ri, the byte range [scan0, scan1) of the entropy data and the restart intervals' ranges"""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[:2] != b"\xff\xd8":
        raise Malformed("no SOI")
    pos, qt, dht, ri, frame, adobe = 2, {}, {}, 0, None, None

    def need(k):
        if pos + k > n:
            raise Malformed("cut inside the headers")

    while True:
        need(2)
        if data[pos] != 0xFF:
            raise Malformed("marker expected")
        while pos < n and data[pos] == 0xFF:
            pos += 1
        need(1)
        m = data[pos]
        pos += 1
        if m == 0xD9:
            raise Malformed("EOI before SOS")
        need(2)
        L = int.from_bytes(data[pos:pos + 2], "big")
        if L < 2:
            raise Malformed("segment length")
        need(L)
        seg = data[pos + 2:pos + L]
        if m == 0xDB:
            q = 0
            while q < len(seg):
                pq, tq = seg[q] >> 4, seg[q] & 15
                if pq:
                    raise Unsupported("16-bit quantiser table")
                if tq > 3 or q + 65 > len(seg):
                    raise Malformed("DQT")
                t = np.zeros(64, np.int64)
                t[NATURAL] = np.frombuffer(seg[q + 1:q + 65], np.uint8)
                qt[tq] = t
                q += 65
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                if q + 17 > len(seg):
                    raise Malformed("DHT")
                tc, th = seg[q] >> 4, seg[q] & 15
                counts = list(seg[q + 1:q + 17])
                tot = sum(counts)
                if tc > 1 or th > 3 or tot > 256 or q + 17 + tot > len(seg):
                    raise Malformed("DHT")
                dht[(tc, th)] = (counts, list(seg[q + 17:q + 17 + tot]))
                q += 17 + tot
        elif m == 0xC0:
            if len(seg) < 6:
                raise Malformed("SOF")
            P, H, W, nf = seg[0], int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big"), seg[5]
            if P != 8:
                raise Unsupported("%d-bit samples" % P)
            if len(seg) < 6 + 3 * nf or H == 0 or W == 0:
                raise Malformed("SOF")
            if nf not in (1, 3):
                raise Unsupported("%d components" % nf)
            frame = (H, W, [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nf)])
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise Unsupported("SOF%d (progressive, arithmetic, lossless or 12-bit)" % (m - 0xC0))
        elif m == 0xCC:
            raise Unsupported("arithmetic coding")
        elif m == 0xDD:
            if len(seg) < 2:
                raise Malformed("DRI")
            ri = int.from_bytes(seg[:2], "big")
        elif m == 0xEE and len(seg) >= 12 and seg[:5] == b"Adobe":
            adobe = seg[11]
        elif m == 0xDA:
            if frame is None:
                raise Malformed("SOS before SOF")
            H, W, fc = frame
            ns = seg[0] if seg else 0
            if len(seg) < 1 + 2 * ns + 3:
                raise Malformed("SOS")
            if ns != len(fc):
                raise Unsupported("multi-scan")
            comps = []
            for i in range(ns):
                cs, tdta = seg[1 + 2 * i], seg[2 + 2 * i]
                if cs != fc[i][0]:
                    raise Unsupported("scan component order")
                comps.append((fc[i][1], fc[i][2], fc[i][3], tdta >> 4, tdta & 15))
            pos += L
            break
        pos += L
    if len(comps) == 3:
        if adobe == 0:
            raise Unsupported("Adobe transform 0")
        if (comps[0][:2] not in ((1, 1), (2, 1), (2, 2))) or comps[1][:2] != (1, 1) or comps[2][:2] != (1, 1):
            raise Unsupported("sampling factors")
    else:
        comps = [(1, 1) + comps[0][2:]]            # a single component is never interleaved: its factors do not matter
    for hs, vs, tq, td, ta in comps:
        if tq not in qt or (0, td) not in dht or (1, ta) not in dht:
            raise Malformed("missing table")
    # the entropy data ends at the first marker that is neither a stuffed zero nor RSTn; restart intervals split at RSTn
    scan0, i, cuts = pos, pos, []
    while True:
        j = data.find(b"\xff", i)
        if j < 0 or j + 1 >= n:
            scan1 = n
            break
        b = data[j + 1]
        if b == 0:
            i = j + 2
        elif b == 0xFF:
            i = j + 1
        elif 0xD0 <= b <= 0xD7:
            cuts.append(j)
            i = j + 2
        else:
            scan1 = j
            break
    hs, vs = comps[0][0], comps[0][1]
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    begins = [scan0] + [c + 2 for c in cuts]
    ends = cuts + [scan1]
    if not ri:
        begins, ends = [scan0], [scan1]
    lanes = [(b, e, k * ri) for k, (b, e) in enumerate(zip(begins, ends)) if k * max(ri, 1) < mx * my]
    if not lanes:
        lanes = [(scan0, scan1, 0)]
    return dict(H=H, W=W, comps=comps, qt=qt, dht=dht, ri=ri, scan0=scan0, scan1=scan1, mx=mx, my=my, lanes=lanes)


# ------------------------------------------------------------------------------------------------ Huffman
def derived_table(counts, values):
    """jpeg_make_d_derived_tbl: (lut 256 of nbits << 8 | symbol, maxcode[0..16], valoff[0..16], huffval 256)"""
    sizes = [l for l in range(1, 17) for _ in range(counts[l - 1])]
    codes, code, si = [], 0, sizes[0] if sizes else 0
    p = 0
    while p < len(sizes):
        while p < len(sizes) and sizes[p] == si:
            codes.append(code)
            code += 1
            p += 1
        if code > (1 << si):
            raise Malformed("bad Huffman code lengths")
        code <<= 1
        si += 1
    maxcode, valoff = np.full(17, -1, np.int32), np.zeros(17, np.int32)
    p = 0
    for l in range(1, 17):
        if counts[l - 1]:
            valoff[l] = p - codes[p]
            p += counts[l - 1]
            maxcode[l] = codes[p - 1]
    lut = np.zeros(256, np.uint16)
    p = 0
    for l in range(1, 9):
        for _ in range(counts[l - 1]):
            look = codes[p] << (8 - l)
            lut[look:look + (1 << (8 - l))] = (l << 8) | values[p]
            p += 1
    hv = np.zeros(256, np.uint8)
    hv[:len(values)] = values
    return lut, maxcode, valoff, hv


def table_bytes(counts, values):
    """the 1024-byte device form of one Huffman table (include/xmodal.h)"""
    lut, maxcode, valoff, hv = derived_table(counts, values)
    raw = lut.tobytes() + hv.tobytes() + maxcode.tobytes() + valoff.tobytes()
    return raw + bytes(HT_BYTES - len(raw))


class Bits:
    """the entropy bytes of one restart interval, unstuffed, as 16-bit windows; zeros past the end"""

    def __init__(self, data, b, e):
        seg = np.frombuffer(data, np.uint8)[b:e]
        stuffed = np.zeros(seg.size, bool)
        ff = np.nonzero(seg[:-1] == 0xFF)[0] if seg.size else np.zeros(0, int)
        last = -2
        for i in ff:                                  # FF 00 pairs, left to right
            if i > last and seg[i + 1] == 0:
                stuffed[i + 1] = True
                last = i + 1
        self.src = np.nonzero(~stuffed)[0] + b        # file offset of every unstuffed byte
        bits = np.unpackbits(np.concatenate([seg[~stuffed], np.zeros(8, np.uint8)])).astype(np.int64)
        self.real = 8 * int((~stuffed).sum())
        bits = np.concatenate([bits, np.zeros(1 << 16, np.int64)])
        w = np.zeros(bits.size - 16, np.int64)
        for j in range(16):
            w += bits[j:j + w.size] << (15 - j)
        self.w, self.pos = w, 0

    def peek16(self):
        return int(self.w[min(self.pos, self.w.size - 1)])

    def take(self, s):
        v = self.peek16() >> (16 - s) if s else 0
        self.pos += s
        return v

    def file_pos(self):
        """file offset just past the last byte a bit has been taken from"""
        k = (self.pos + 7) // 8
        return int(self.src[k - 1]) + 1 if 0 < k <= self.src.size else (int(self.src[0]) if k == 0 and self.src.size else 1 << 62)


def huff_decode(br, tbl):
    lut, maxcode, valoff, hv = tbl
    w = br.peek16()
    e = int(lut[w >> 8])
    if e >> 8:
        br.pos += e >> 8
        return e & 255
    for l in range(9, 17):
        code = w >> (16 - l)
        if maxcode[l] >= 0 and code <= maxcode[l]:
            br.pos += l
            return int(hv[(code + valoff[l]) & 255])
    return None


def extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


OK, TRUNCATED, BADCODE = 0, 1, 2


def decode_coefs(data, P):
    """-> (coefs per component [by, bx, 64] natural order, status, file position after every MCU)"""
    data = bytes(data)
    comps, mx, my = P["comps"], P["mx"], P["my"]
    tabs = [(derived_table(*P["dht"][(0, td)]), derived_table(*P["dht"][(1, ta)])) for _, _, _, td, ta in comps]
    coefs = [np.zeros((my * vs, mx * hs, 64), np.int32) for hs, vs, _, _, _ in comps]
    status, mcu_end = OK, np.full(mx * my, 1 << 62, np.int64)
    for b, e, mcu0 in P["lanes"]:
        br, pred, bad = Bits(data, b, e), [0] * len(comps), False
        stop = min(mcu0 + P["ri"], mx * my) if P["ri"] else mx * my
        for mcu in range(mcu0, stop):
            ym, xm = divmod(mcu, mx)
            for c, (hs, vs, _, _, _) in enumerate(comps):
                for blk in range(hs * vs):
                    out = coefs[c][ym * vs + blk // hs, xm * hs + blk % hs]
                    s = huff_decode(br, tabs[c][0])
                    if s is None or s > 15:
                        bad = True
                        break
                    pred[c] += extend(br.take(s), s)
                    out[0] = ((pred[c] & 0xFFFF) ^ 0x8000) - 0x8000              # the coefficient is a 16-bit value
                    k = 1
                    while k < 64:
                        rs = huff_decode(br, tabs[c][1])
                        if rs is None:
                            bad = True
                            break
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            k += 16
                            continue
                        k += r
                        if k > 63:
                            bad = True
                            break
                        out[NATURAL[k]] = extend(br.take(s), s)
                        k += 1
                    if bad:
                        break
                if bad:
                    break
            if bad:
                status |= BADCODE
                break
            mcu_end[mcu] = br.file_pos() if br.pos <= br.real else 1 << 62
        if br.pos > br.real:
            status |= TRUNCATED
    return coefs, status, mcu_end


# ------------------------------------------------------------------------------------------------ ISLOW IDCT
def _idct_1d(x, first):
    """one pass of jpeg_idct_islow over eight int64 arrays (CONST_BITS 13, PASS1_BITS 2)"""
    z2, z3 = x[2], x[6]
    z1 = (z2 + z3) * 4433
    tmp2, tmp3 = z1 - z3 * 15137, z1 + z2 * 6270
    tmp0, tmp1 = (x[0] + x[4]) << 13, (x[0] - x[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    n = 11 if first else 18
    d = lambda v: (v + (1 << (n - 1))) >> n
    return [d(tmp10 + tmp3), d(tmp11 + tmp2), d(tmp12 + tmp1), d(tmp13 + tmp0), d(tmp13 - tmp0), d(tmp12 - tmp1),
            d(tmp11 - tmp2), d(tmp10 - tmp3)]


def idct_islow(coefs, q):
    """coefs [..., 64] natural order, q 64 natural order -> samples [..., 8, 8] uint8"""
    x = (coefs.astype(np.int64) * q).reshape(coefs.shape[:-1] + (8, 8))
    ws = np.stack(_idct_1d([x[..., r, :] for r in range(8)], True), -2)       # columns: over the row index
    out = np.stack(_idct_1d([ws[..., :, c] for c in range(8)], False), -1)    # rows: over the column index
    v = out & 1023
    v = np.where(v >= 512, v - 1024, v)
    return np.clip(v + 128, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ upsampling, colour
def upsample(plane, hs, vs, H, W):
    """a chroma plane of ceil(H / vs) x ceil(W / hs) real samples -> H x W, libjpeg's fancy (triangle) filters; a plane
    of one or two columns is replicated instead (jdsample.c: fancy only where downsampled_width > 2)"""
    dh, dw = -(-H // vs), -(-W // hs)
    p = plane[:dh, :dw].astype(np.int64)
    if hs == 1 and vs == 1:
        return p
    if dw <= 2:
        return np.repeat(np.repeat(p, vs, 0), hs, 1)[:H, :W]
    i = np.arange(dw)
    left, right = np.maximum(i - 1, 0), np.minimum(i + 1, dw - 1)
    if vs == 1:
        out = np.zeros((dh, 2 * dw), np.int64)
        out[:, 0::2] = (3 * p + p[:, left] + 1) >> 2
        out[:, 1::2] = (3 * p + p[:, right] + 2) >> 2
        return out[:H, :W]
    y = np.arange(2 * dh)
    near = y >> 1
    far = np.clip(np.where(y & 1, near + 1, near - 1), 0, dh - 1)
    cs = 3 * p[near] + p[far]
    out = np.zeros((2 * dh, 2 * dw), np.int64)
    out[:, 0::2] = (3 * cs + cs[:, left] + 8) >> 4
    out[:, 1::2] = (3 * cs + cs[:, right] + 7) >> 4
    return out[:H, :W]


def ycc_to_rgb(y, cb, cr):
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def np_decode(data, with_status=False):
    """H x W x 3 uint8, what PIL gives for the file"""
    P = parse(data)
    coefs, status, mcu_end = decode_coefs(data, P)
    H, W = P["H"], P["W"]
    planes = []
    for c, (hs, vs, tq, _, _) in enumerate(P["comps"]):
        s = idct_islow(coefs[c], P["qt"][tq])                                  # [by, bx, 8, 8]
        planes.append(s.transpose(0, 2, 1, 3).reshape(s.shape[0] * 8, s.shape[1] * 8))
    if len(planes) == 1:
        out = np.repeat(planes[0][:H, :W, None], 3, 2)
    else:
        hs, vs = P["comps"][0][:2]
        out = ycc_to_rgb(planes[0][:H, :W].astype(np.int64), upsample(planes[1], hs, vs, H, W),
                         upsample(planes[2], hs, vs, H, W))
    return (out, status, mcu_end, P) if with_status else out


def complete_rows(data, whole):
    """pixel rows of a truncated file that a decoder has in full: the MCU rows whose last bit lies before the cut, minus
    the last row of the last one when the chroma is upsampled vertically (it blends in the next, missing, chroma row)"""
    P = parse(whole)
    _, _, mcu_end = decode_coefs(whole, P)
    rows_done = 0
    for j in range(P["my"]):
        if mcu_end[(j + 1) * P["mx"] - 1] > len(data):
            break
        rows_done = j + 1
    vs = P["comps"][0][1]
    return max(0, min(P["H"], rows_done * 8 * vs - (1 if vs == 2 else 0)))


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _maker():
    spec = importlib.util.spec_from_file_location("make_golden_jpeg", os.path.join(ROOT, "tests", "golden", "make_golden_jpeg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def have_pil():
    try:
        import PIL  # noqa: F401
        return True
    except ImportError:
        return False


def test_restatement_equals_pil_on_every_fixture(golden):
    names = [str(n) for n in golden["names"]]
    assert len(names) == 11
    for name in names:
        got, status, _, P = np_decode(golden["bytes_" + name].tobytes(), with_status=True)
        assert status == OK, name
        assert got.shape == golden["pix_" + name].shape and np.array_equal(got, golden["pix_" + name]), name
    # the cases really are what their names say
    kinds = {n: [c[:2] for c in parse(golden["bytes_" + n].tobytes())["comps"]] for n in names}
    assert kinds["grey_8x8"] == [(1, 1)] and kinds["s444_16x16"][0] == (1, 1) and kinds["s422_33x47"][0] == (2, 1)
    assert kinds["s420_1x1"][0] == (2, 2)
    rst = parse(golden["bytes_s420_64x64_rst"].tobytes())
    assert rst["ri"] == 3 and len(rst["lanes"]) == 6 and rst["lanes"][1][2] == rst["ri"]     # 5 RST markers
    assert b"\xff\x00" in golden["bytes_s420_50x50_q100"].tobytes()[parse(golden["bytes_s420_50x50_q100"].tobytes())["scan0"]:]
    assert int(parse(golden["bytes_s420_50x50_q100"].tobytes())["qt"][0].max()) == 1
    assert sum(v.size for k, v in golden.items() if k.startswith("bytes_")) < 100000


def test_restatement_rejects_and_flags(golden):
    with pytest.raises(Unsupported, match="SOF2"):
        parse(golden["bytes_progressive"].tobytes())
    whole = golden["bytes_s420_96x80_q50"].tobytes()
    with pytest.raises(Malformed):
        parse(whole[:parse(whole)["scan0"] - 5])
    with pytest.raises(Malformed):
        parse(b"\x00\x01\x02\x03")
    cut = golden["bytes_truncated"].tobytes()
    got, status, _, P = np_decode(cut, with_status=True)
    assert status == TRUNCATED and P["scan1"] == len(cut)
    rows = complete_rows(cut, whole)
    assert 16 <= rows < 96 and np.array_equal(got[:rows], golden["pix_truncated"][:rows])
    assert not np.array_equal(got, golden["pix_truncated"])


@pytest.mark.skipif(not have_pil(), reason="PIL regenerates the fixtures; the stored ones are checked above")
def test_fixtures_regenerate_and_random_sizes_equal_pil(golden):
    import PIL
    mk = _maker()
    if PIL.__version__ == str(golden["pil_version"]):       # another PIL may encode differently; decoding is checked below
        fresh = mk.cases()
        assert sorted(fresh) == sorted(golden)
        for k in fresh:
            assert np.array_equal(fresh[k], golden[k]), k
    rng = np.random.default_rng(2024)
    for mode, ss in (("L", None), ("RGB", 0), ("RGB", 1), ("RGB", 2)):
        for t in range(20):
            H, W = int(rng.integers(1, 41)), int(rng.integers(1, 41))
            opts = {"quality": int(rng.integers(30, 101)), "optimize": bool(t & 1)}
            if t % 5 == 0:
                opts["restart_marker_blocks"] = int(rng.integers(1, 5))
            data = mk.encode(1000 + t, H, W, mode, ss, opts)
            assert np.array_equal(np_decode(data), mk.pil_decode(data)), (mode, ss, H, W, opts)


# ------------------------------------------------------------------------------------------------ xm_jpeg_plan, no device
def _supported(golden):
    return [str(n) for n in golden["names"]]


def test_plan_equals_the_restatements_parse(golden):
    from mcncrossmodalemotions_amd import vl
    names = _supported(golden) + ["truncated"]
    files = [golden["bytes_" + n].tobytes() for n in names]
    buf, plan = vl.jpeg_plan(files)
    N, sizes = len(files), plan["sizes"]
    desc = buf[plan["desc"][0]:plan["desc"][0] + plan["desc"][1]].view(np.int64).reshape(N, DESC)
    lanes = buf[plan["lanes"][0]:plan["lanes"][0] + plan["lanes"][1]].view(np.int64).reshape(-1, LANE)
    tables = buf[plan["tables"][0]:plan["tables"][0] + plan["tables"][1]]
    nq, nh = int(sizes[1]), int(sizes[2])
    assert tables.size == nq * QT_BYTES + nh * HT_BYTES == sizes[0] and sizes[7] == N
    qt = tables[:nq * QT_BYTES].view(np.uint16).reshape(nq, 64)
    ht = tables[nq * QT_BYTES:].reshape(nh, HT_BYTES)
    assert nh < 6 * N and nq < 3 * N                                   # equal tables share a slot
    base, coef, pix, lane0 = 0, 0, 0, 0
    for i, f in enumerate(files):
        P, d = parse(f), desc[i]
        assert (d[0], d[1]) == (base + P["scan0"], base + P["scan1"]), names[i]
        assert (d[2], d[3], d[4], d[7], d[8], d[9]) == (P["H"], P["W"], len(P["comps"]), P["ri"], P["mx"], P["my"]), names[i]
        assert (d[5], d[6]) == P["comps"][0][:2], names[i]
        for c in range(3):
            hs, vs, tq, td, ta = P["comps"][c if c < len(P["comps"]) else 0]
            assert np.array_equal(qt[d[10 + c]], P["qt"][tq]), (names[i], c)
            assert ht[d[13 + c]].tobytes() == table_bytes(*P["dht"][(0, td)]), (names[i], c)
            assert ht[d[16 + c]].tobytes() == table_bytes(*P["dht"][(1, ta)]), (names[i], c)
        nblocks = sum(P["mx"] * P["my"] * c[0] * c[1] for c in P["comps"])
        assert (d[19], d[20], d[21], d[22], d[23]) == (coef, coef, pix, lane0, len(P["lanes"])), names[i]
        for k, (b, e, m0) in enumerate(P["lanes"]):
            assert tuple(lanes[lane0 + k]) == (i, base + b, base + e, m0), (names[i], k)
        base, coef, pix, lane0 = base + len(f), coef + 64 * nblocks, pix + 3 * P["H"] * P["W"], lane0 + len(P["lanes"])
    assert (sizes[3], sizes[4], sizes[5], sizes[6]) == (coef, coef, pix, lane0) and lanes.shape[0] == lane0
    assert desc[names.index("s420_64x64_rst")][23] == 6


def test_plan_rejects_with_the_index_of_the_file(golden):
    from mcncrossmodalemotions_amd import _lib, vl
    ok = golden["bytes_s420_16x16"].tobytes()
    with pytest.raises(_lib.XmError, match=r"file 2: SOF2") as e:
        vl.jpeg_plan([ok, ok, golden["bytes_progressive"].tobytes()])
    assert e.value.code == 5                                           # XM_ENOTSUP
    whole = golden["bytes_s420_96x80_q50"].tobytes()
    with pytest.raises(_lib.XmError, match=r"file 1: cut inside its headers") as e:
        vl.jpeg_plan([ok, whole[:parse(whole)["scan0"] - 5]])
    assert e.value.code == 1                                           # XM_EINVAL
    with pytest.raises(_lib.XmError, match=r"file 0: no SOI") as e:
        vl.jpeg_plan([b"not a jpeg file", ok])
    assert e.value.code == 1
    # 16-bit quantiser table, 12-bit samples, four components, odd sampling: valid files this build does not decode
    i = ok.index(b"\xff\xdb")
    assert vl.jpeg_plan([ok])[1]["sizes"][7] == 1
    for patch, msg in [((i + 4, ok[i + 4] | 0x10), "16-bit quantiser"), ((ok.index(b"\xff\xc0") + 4, 12), "12-bit"),
                       ((ok.index(b"\xff\xc0") + 9, 4), "4 components"), ((ok.index(b"\xff\xc0") + 11, 0x12), "luma sampling 1 x 2"),
                       ((ok.index(b"\xff\xc0") + 14, 0x21), "chroma sampling")]:
        bad = bytearray(ok)
        bad[patch[0]] = patch[1]
        with pytest.raises(_lib.XmError, match="file 0: .*" + msg) as e:
            vl.jpeg_plan([bytes(bad)])
        assert e.value.code == 5, msg


def test_plan_arguments_are_rejected_without_a_device(golden):
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    ok = golden["bytes_grey_8x8"].tobytes()
    data = np.frombuffer(ok, np.uint8).copy()
    offs = np.array([0, len(ok)], np.int64)
    desc, lanes, tabs, sizes = np.zeros(DESC, np.int64), np.zeros(4 * LANE, np.int64), np.zeros(8192, np.uint8), np.zeros(8, np.int64)
    p = lambda a: C.c_void_p(a.ctypes.data)
    g = lambda **k: [k.get("bytes", p(data)), k.get("offsets", p(offs)), k.get("N", 1), k.get("desc", p(desc)),
                     k.get("lanes", p(lanes)), k.get("lanes_cap", 4), k.get("tables", p(tabs)), k.get("tables_cap", 8192),
                     k.get("sizes", p(sizes))]
    assert L.xm_jpeg_plan(*g()) == 0 and sizes[6] == 1 and desc[2] == 8
    for bad, msg in [(dict(N=-1), b"N >= 0"), (dict(lanes_cap=-1), b"lanes_cap >= 0"), (dict(tables_cap=-1), b"tables_cap >= 0"),
                     (dict(bytes=None), b"NULL"), (dict(offsets=None), b"NULL"), (dict(desc=None), b"NULL"),
                     (dict(lanes=None), b"NULL"), (dict(tables=None), b"NULL"), (dict(sizes=None), b"NULL")]:
        assert L.xm_jpeg_plan(*g(**bad)) == 1 and msg in L.xm_last_error(), bad
    assert L.xm_jpeg_plan(*g(lanes_cap=0)) == 2 and sizes[6] == 1            # XM_ENOMEM, the need is reported
    assert L.xm_jpeg_plan(*g(tables_cap=16)) == 2 and sizes[0] == QT_BYTES + 2 * HT_BYTES
    assert L.xm_jpeg_plan(*g(N=0, bytes=None)) == 0
    bad_offs = np.array([5, 2], np.int64)
    assert L.xm_jpeg_plan(*g(offsets=p(bad_offs))) == 1 and b"ascend" in L.xm_last_error()
    # the device entry rejects its arguments before it touches a device
    one = C.c_void_p(4096)
    d = lambda **k: [k.get("bytes", one), k.get("nbytes", 100), one, k.get("N", 1), one, k.get("nlanes", 1), k.get("tables", one),
                     1, 2, k.get("coef", 64), k.get("plane", 64), 192, None, k.get("faces", None), k.get("crop", 0.5),
                     k.get("Ho", 8), 8, None, k.get("status", one), None]
    for bad, msg in [(dict(N=-1), b"negative"), (dict(bytes=None), b"NULL"), (dict(status=None), b"NULL"),
                     (dict(coef=65), b"xm_jpeg_plan reports"), (dict(nlanes=0), b"xm_jpeg_plan reports"),
                     (dict(bytes=C.c_void_p(4100)), b"aligned"), (dict(faces=one, Ho=0), b"Ho > 0"),
                     (dict(faces=one, crop=1.5), b"crop")]:
        assert L.xm_jpeg_decode_batch(*d(**bad)) == 1 and msg in L.xm_last_error(), bad
    assert L.xm_jpeg_decode_batch(*d(N=0)) == 0


def test_imreadjpeg_options_raise_before_anything_else():
    from mcncrossmodalemotions_amd import vl
    with pytest.raises(ValueError, match="Prefetch"):
        vl.imreadjpeg([b""], prefetch=True)
    with pytest.raises(ValueError, match="center"):
        vl.imreadjpeg([b""], crop_location="random")
    with pytest.raises(ValueError, match="bilinear"):
        vl.imreadjpeg([b""], interpolation="bicubic")


def test_jpeg_abi_declared_typed_and_exported():
    from mcncrossmodalemotions_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "xmodal.h")).read()
    L = _lib.load()
    assert L.xm_version() >= 113
    assert "jpeg.hip" in build.SOURCES
    for name in NEW_ABI:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name]
        proto = re.search(r"\bint %s\(([^;]*)\);" % name, hdr).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name]), name
    for cite in ("fetch_emovoxceleb_imdb.m:160-172", "compute_visual_feats.m:130-143"):
        assert cite in hdr, cite
    for k, v in (("XM_JPEG_DESC", DESC), ("XM_JPEG_LANE", LANE), ("XM_JPEG_QT_BYTES", QT_BYTES), ("XM_JPEG_HT_BYTES", HT_BYTES)):
        assert re.search(r"%s = %d\b" % (k, v), hdr), k

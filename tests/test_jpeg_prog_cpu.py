"""CPU: a numpy restatement of the progressive JPEG decode behind vl.imreadjpeg(progressive=True) -- the scan script
parse with its levels and rasters, DC first / refinement and AC first / refinement as T.81 G.1.2 on top of the bit
reader, Huffman tables, IDCT, upsampling and colour conversion of tests/test_jpeg_cpu.py -- equal to PIL's pixels on
every fixture of tests/golden/jpeg_progressive.npz, the partial files included; xm_jpeg_plan_prog through ctypes without
a device against the restatement's parse; hand-edited scan headers refused with the file's index and the scan's number;
baseline batches planned as xm_jpeg_plan plans them; the plan header alone, every truncation and byte mutation of a
file, under the host sanitizers (tests/jpeg_scan_plan_check.cpp); the ABI of the two new entries.  The GPU tests import from here."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_jpeg_cpu import (BADCODE, GOLDEN, HT_BYTES, NATURAL, OK, QT_BYTES, TRUNCATED, Bits, Malformed, Unsupported,
                           derived_table, extend, huff_decode, idct_islow, parse, table_bytes, upsample, ycc_to_rgb)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_PROG = os.path.join(ROOT, "tests", "golden", "jpeg_progressive.npz")
NEW_ABI = ["xm_jpeg_plan_prog", "xm_jpeg_decode_batch_prog"]
DESC, LANE, SCAN = 24, 4, 24                                       # the layout documented in include/xmodal.h
SEQ, DC_FIRST, DC_REFINE, AC_FIRST, AC_REFINE = range(5)           # XM_JPEG_SCAN_*
PARTIAL = ["partial_1", "partial_5", "partial_9"]


# ------------------------------------------------------------------------------------------------ parse
def scan_end(data, pos):
    """(end of the entropy data that starts at pos, offsets of the RSTn markers inside it)"""
    n, i, cuts = len(data), pos, []
    while True:
        j = data.find(b"\xff", i)
        if j < 0 or j + 1 >= n:
            return n, cuts
        b = data[j + 1]
        if b == 0:
            i = j + 2
        elif b == 0xFF:
            i = j + 1
        elif 0xD0 <= b <= 0xD7:
            cuts.append(j)
            i = j + 2
        else:
            return j, cuts


def parse_prog(data):
    """the frame and the scan script of a progressive or baseline file: H, W, comps [(hs, vs, tq)], qt as it stood at
    the first scan, mx, my and scans [dict(comps, Ss, Se, Ah, Al, kind, dc, ac: (counts, values) per scan component as DHT
    stood at the scan, b0, b1, bw, bh, level, ri, lanes [(begin, end, first MCU)])].  A file may end after any scan."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[:2] != b"\xff\xd8":
        raise Malformed("no SOI")
    pos, qt, dht, ri, frame, scans = 2, {}, {}, 0, None, []
    bits, level_of, qt0 = {}, {}, None
    while True:
        if pos + 2 > n or data[pos] != 0xFF:
            if scans:
                break
            raise Malformed("cut inside the headers")
        while pos < n and data[pos] == 0xFF:
            pos += 1
        if pos >= n:
            if scans:
                break
            raise Malformed("cut inside the headers")
        m = data[pos]
        pos += 1
        if m == 0xD9:
            if scans:
                break
            raise Malformed("EOI before SOS")
        if pos + 2 > n:
            if scans:
                break
            raise Malformed("cut inside the headers")
        L = int.from_bytes(data[pos:pos + 2], "big")
        if L < 2:
            raise Malformed("segment length")
        if pos + L > n:
            if scans:
                break
            raise Malformed("cut inside the headers")
        seg = data[pos + 2:pos + L]
        if m == 0xDB:
            q = 0
            while q < len(seg):
                if seg[q] >> 4:
                    raise Unsupported("16-bit quantiser table")
                t = np.zeros(64, np.int64)
                t[NATURAL] = np.frombuffer(seg[q + 1:q + 65], np.uint8)
                qt[seg[q] & 15] = t
                q += 65
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                counts = list(seg[q + 1:q + 17])
                tot = sum(counts)
                dht[(seg[q] >> 4, seg[q] & 15)] = (counts, list(seg[q + 17:q + 17 + tot]))
                q += 17 + tot
        elif m in (0xC0, 0xC2):
            P, H, W, nf = seg[0], int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big"), seg[5]
            if P != 8:
                raise Unsupported("%d-bit samples" % P)
            if nf not in (1, 3):
                raise Unsupported("%d components" % nf)
            frame = (m == 0xC2, H, W, [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nf)])
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8):
            raise Unsupported("SOF%d" % (m - 0xC0))
        elif m == 0xDD:
            ri = int.from_bytes(seg[:2], "big")
        elif m == 0xDA:
            prog, H, W, fc = frame
            ids = [c[0] for c in fc]
            ns = seg[0]
            comps = [ids.index(seg[1 + 2 * i]) for i in range(ns)]
            td = [seg[2 + 2 * i] >> 4 for i in range(ns)]
            ta = [seg[2 + 2 * i] & 15 for i in range(ns)]
            Ss, Se, Ah, Al = (seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns] >> 4, seg[3 + 2 * ns] & 15) if prog else (0, 63, 0, 0)
            hs, vs = (fc[0][1], fc[0][2]) if len(fc) == 3 else (1, 1)
            mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
            kind, level = SEQ, 0
            if prog:
                if Ss > Se or Se > 63 or (Ss == 0 and Se != 0) or (Ss > 0 and ns != 1) or Al > 13 or (Ah and Ah != Al + 1):
                    raise Malformed("scan %d" % len(scans))
                touched = [(c, k) for c in comps for k in range(Ss, Se + 1)]
                for t in touched:
                    if (Ah == 0 and t in bits) or (Ah and bits.get(t) != Ah):
                        raise Malformed("scan %d" % len(scans))
                level = max([level_of[t] + 1 for t in touched if t in level_of] + [0])
                for t in touched:
                    bits[t], level_of[t] = Al, level
                kind = (DC_FIRST if Ah == 0 else DC_REFINE) if Ss == 0 else (AC_FIRST if Ah == 0 else AC_REFINE)
            if qt0 is None:
                qt0 = {k: v.copy() for k, v in qt.items()}
            pos += L
            end, cuts = scan_end(data, pos)
            bw, bh = mx, my
            if ns == 1 and len(fc) == 3:
                hc, vc = (hs, vs) if comps[0] == 0 else (1, 1)
                bw, bh = -(-(-(-W * hc // hs)) // 8), -(-(-(-H * vc // vs)) // 8)
            begins, ends = ([pos] + [c + 2 for c in cuts], cuts + [end]) if ri else ([pos], [end])
            lanes = [(b, e, k * ri) for k, (b, e) in enumerate(zip(begins, ends)) if k == 0 or k * ri < bw * bh]
            lanes[-1] = (lanes[-1][0], end, lanes[-1][2])
            scans.append(dict(comps=comps, Ss=Ss, Se=Se, Ah=Ah, Al=Al, kind=kind, b0=pos, b1=end, bw=bw, bh=bh, level=level, ri=ri,
                              dc=[dht.get((0, t)) if kind in (SEQ, DC_FIRST) else None for t in td],
                              ac=[dht.get((1, t)) if kind in (SEQ, AC_FIRST, AC_REFINE) else None for t in ta], lanes=lanes))
            if not prog:
                break
            pos = end
            continue
        pos += L
    prog, H, W, fc = frame
    comps = [(c[1], c[2], c[3]) for c in fc] if len(fc) == 3 else [(1, 1, fc[0][3])]
    hs, vs = comps[0][:2]
    coef_bits = [[bits.get((c, k), -1) for k in range(10)] for c in range(len(comps))]
    rasters = [(-(-(-(-W * h // hs)) // 8), -(-(-(-H * v // vs)) // 8)) for h, v, _ in comps]
    return dict(progressive=prog, H=H, W=W, comps=comps, qt=qt0, mx=-(-W // (8 * hs)), my=-(-H // (8 * vs)), scans=scans,
                coef_bits=coef_bits, rasters=rasters)


# ------------------------------------------------------------------------------------------------ entropy decode
def wrap16(v):
    return ((int(v) & 0xFFFF) ^ 0x8000) - 0x8000


def decode_scan(data, P, S, coefs):
    """one scan into coefs (per component [by, bx, 64], natural order) -> status"""
    hs, vs = P["comps"][0][:2]
    ns, kind, Ss, Se, Al = len(S["comps"]), S["kind"], S["Ss"], S["Se"], S["Al"]
    dc = [derived_table(*t) if t else None for t in S["dc"]]
    ac = [derived_table(*t) if t else None for t in S["ac"]]
    total, status = S["bw"] * S["bh"], OK
    p1, m1 = 1 << Al, -(1 << Al)
    for b, e, mcu0 in S["lanes"]:
        br, pred, eob, bad = Bits(data, b, e), [0] * ns, 0, False
        stop = min(mcu0 + S["ri"], total) if S["ri"] else total
        for mcu in range(mcu0, stop):
            ym, xm = divmod(mcu, S["bw"])
            for i, c in enumerate(S["comps"]):
                hc, vc = (hs, vs) if ns > 1 and c == 0 else (1, 1)
                for blk in range(hc * vc):
                    out = coefs[c][ym * vc + blk // hc, xm * hc + blk % hc]
                    if kind in (SEQ, DC_FIRST):
                        s = huff_decode(br, dc[i])
                        if s is None or s > 15:
                            bad = True
                            break
                        pred[i] += extend(br.take(s), s)
                        out[0] = wrap16(pred[i] * p1)
                    if kind == DC_REFINE:
                        if br.take(1):
                            out[0] |= p1
                    elif kind == SEQ:
                        k = 1
                        while k < 64:
                            rs = huff_decode(br, ac[i])
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
                    elif kind == AC_FIRST:
                        if eob > 0:
                            eob -= 1
                            continue
                        k = Ss
                        while k <= Se:
                            rs = huff_decode(br, ac[i])
                            if rs is None:
                                bad = True
                                break
                            r, s = rs >> 4, rs & 15
                            if s:
                                k += r
                                if k > Se:
                                    bad = True
                                    break
                                out[NATURAL[k]] = wrap16(extend(br.take(s), s) * p1)
                            elif r == 15:
                                k += 15
                            else:
                                eob = (1 << r) + br.take(r) - 1
                                break
                            k += 1
                    elif kind == AC_REFINE:
                        def correct(j):
                            cur = int(out[NATURAL[j]])
                            if cur != 0 and br.take(1) and (cur & p1) == 0:
                                out[NATURAL[j]] = cur + (p1 if cur >= 0 else m1)
                            return cur != 0
                        k = Ss
                        if eob == 0:
                            while k <= Se:
                                rs = huff_decode(br, ac[i])
                                if rs is None:
                                    bad = True
                                    break
                                r, s = rs >> 4, rs & 15
                                val = 0
                                if s:
                                    if s != 1:
                                        bad = True
                                        break
                                    val = p1 if br.take(1) else m1
                                elif r != 15:
                                    eob = (1 << r) + br.take(r)
                                    break
                                while k <= Se:
                                    if not correct(k):
                                        r -= 1
                                        if r < 0:
                                            break
                                    k += 1
                                if s:
                                    if k > Se:
                                        bad = True
                                        break
                                    out[NATURAL[k]] = val
                                k += 1
                        if eob > 0 and not bad:
                            while k <= Se:
                                correct(k)
                                k += 1
                            eob -= 1
                    if bad:
                        break
                if bad:
                    break
            if bad:
                status |= BADCODE
                break
            if br.pos > br.real:
                break
        if br.pos > br.real:
            status |= TRUNCATED
        elif eob > 0 and not bad:
            status |= BADCODE
    return status


# ------------------------------------------------------------------------------------------------ block smoothing
# natural-order positions of the coefficients libjpeg estimates, in the zigzag order its coef_bits are kept in
SMOOTH_POS = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24]
# 5 x 5 kernels over the DC values around a block (rows top to bottom); [0]: while no AC bit of the component has
# arrived ("change_dc": the DC itself is smoothed too), [1]: afterwards
SMOOTH_K = {
    1: ([[-1, -1, 0, 1, 1], [-3, 13, 0, -13, 3], [-3, 38, 0, -38, 3], [-3, 13, 0, -13, 3], [-1, -1, 0, 1, 1]],
        [[0] * 5, [0] * 5, [-7, 50, 0, -50, 7], [0] * 5, [0] * 5]),
    3: ([[0, 0, 1, 0, 0], [0, 2, 7, 2, 0], [0, -5, -14, -5, 0], [0, 2, 7, 2, 0], [0, 0, 1, 0, 0]],
        [[0, 0, -1, 0, 0], [0, 0, 13, 0, 0], [0, 0, -24, 0, 0], [0, 0, 13, 0, 0], [0, 0, -1, 0, 0]]),
    4: ([[-1, 0, 0, 0, 1], [0, 9, 0, -9, 0], [0] * 5, [0, -9, 0, 9, 0], [1, 0, 0, 0, -1]],
        [[0, -1, 0, 1, 0], [-1, 10, 0, -10, 1], [0] * 5, [1, -10, 0, 10, -1], [0, 1, 0, -1, 0]]),
    6: ([[0] * 5, [0, 1, 0, -1, 0], [0, 2, 0, -2, 0], [0, 1, 0, -1, 0], [0] * 5], None),
    7: ([[0] * 5, [0, 1, -3, 1, 0], [0] * 5, [0, -1, 3, -1, 0], [0] * 5], None),
    0: ([[-2, -6, -8, -6, -2], [-6, 6, 42, 6, -6], [-8, 42, 152, 42, -8], [-6, 6, 42, 6, -6], [-2, -6, -8, -6, -2]], None),
}
SMOOTH_K[2] = tuple(None if k is None else [list(r) for r in zip(*k)] for k in SMOOTH_K[1])     # AC10 from AC01
SMOOTH_K[5] = tuple(None if k is None else [list(r) for r in zip(*k)] for k in SMOOTH_K[3])     # AC02 from AC20
SMOOTH_K[8] = tuple(None if k is None else [list(r) for r in zip(*k)] for k in SMOOTH_K[7])     # AC21 from AC12
SMOOTH_K[9] = tuple(None if k is None else [list(r) for r in zip(*k)] for k in SMOOTH_K[6])     # AC30 from AC03


def smooth(P, coefs):
    """libjpeg's block smoothing (jdcoefct.c decompress_smooth_data, the 5 x 5 version of libjpeg-turbo 2.1 and later),
    which a decoder applies to a progressive file whose first ten coefficients have not all arrived in full: a
    coefficient that is still zero and not known exactly is estimated from the DC values of the 5 x 5 blocks around
    its block (edges replicated inside the component's own raster) and clamped below 1 << Al."""
    bits = P["coef_bits"]
    if not P["progressive"] or any(b[0] < 0 for b in bits) or not any(v != 0 for b in bits for v in b[1:]):
        return coefs
    out = []
    for c, (_, _, tq) in enumerate(P["comps"]):
        q, (bw, bh), cb = P["qt"][tq], P["rasters"][c], bits[c]
        src, dst = coefs[c], coefs[c].copy()
        change_dc = all(v == -1 for v in cb[1:])
        dc = src[:bh, :bw, 0].astype(np.int64)
        pad = np.pad(dc, 2, mode="edge")
        for z in range(10):
            kern = SMOOTH_K[z][0 if change_dc else 1]
            if kern is None or (z > 0 and cb[z] == 0):
                continue
            num = sum(int(kern[i][j]) * pad[i:i + bh, j:j + bw] for i in range(5) for j in range(5)) * int(q[0])
            Q = int(q[SMOOTH_POS[z]])
            pred = ((Q << 7) + np.abs(num)) // (Q << 8)
            if z > 0 and cb[z] > 0:
                pred = np.minimum(pred, (1 << cb[z]) - 1)
            pred = np.where(num >= 0, pred, -pred)
            cur = src[:bh, :bw, SMOOTH_POS[z]]
            dst[:bh, :bw, SMOOTH_POS[z]] = pred if z == 0 else np.where(cur == 0, pred, cur)
        out.append(dst)
    return out


def np_decode_prog(data, with_status=False):
    """H x W x 3 uint8, what PIL gives for the file (progressive or baseline)"""
    data = bytes(data)
    P = parse_prog(data)
    coefs = [np.zeros((P["my"] * v, P["mx"] * h, 64), np.int32) for h, v, _ in P["comps"]]
    status = OK
    for S in P["scans"]:
        status |= decode_scan(data, P, S, coefs)
    coefs = smooth(P, coefs)
    H, W = P["H"], P["W"]
    planes = []
    for c, (_, _, tq) in enumerate(P["comps"]):
        s = idct_islow(coefs[c], P["qt"][tq])
        planes.append(s.transpose(0, 2, 1, 3).reshape(s.shape[0] * 8, s.shape[1] * 8))
    if len(planes) == 1:
        out = np.repeat(planes[0][:H, :W, None], 3, 2)
    else:
        hs, vs = P["comps"][0][:2]
        out = ycc_to_rgb(planes[0][:H, :W].astype(np.int64), upsample(planes[1], hs, vs, H, W), upsample(planes[2], hs, vs, H, W))
    return (out, status, P) if with_status else out


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def prog():
    return dict(np.load(GOLDEN_PROG))


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def names_of(prog):
    return [str(n) for n in prog["names"]]


def test_restatement_equals_pil_on_every_fixture(prog):
    names = names_of(prog)
    assert names == ["grey_8x8", "grey_17x23", "s444_16x16", "s422_33x47_opt", "s420_16x16", "s420_41x35", "s420_96x80_q10",
                     "s420_50x50_q100", "s420_64x64_rst3", "s420_1x1", "flat_64x64"]
    for name in names:
        got, status, P = np_decode_prog(prog["bytes_" + name].tobytes(), with_status=True)
        assert status == OK and P["progressive"], name
        assert got.shape == prog["pix_" + name].shape and np.array_equal(got, prog["pix_" + name]), name
    # the cases really are what their names say: PIL's script has 10 scans in 3 levels for colour, 6 for grey
    for name in names:
        P = parse_prog(prog["bytes_" + name].tobytes())
        assert len(P["scans"]) == (6 if name.startswith("grey") else 10), name
        assert sorted({S["level"] for S in P["scans"]}) == [0, 1, 2], name
        assert {S["kind"] for S in P["scans"]} == {DC_FIRST, DC_REFINE, AC_FIRST, AC_REFINE}, name
    assert [len(parse_prog(prog["bytes_" + n].tobytes())["scans"]) for n in PARTIAL] == [1, 5, 9]
    whole = prog["pix_s420_41x35"].astype(int)
    assert [int(np.abs(prog["pix_" + n].astype(int) - whole).max()) for n in PARTIAL] == [76, 30, 27]
    luma = [S for S in parse_prog(prog["bytes_s420_41x35"].tobytes())["scans"] if S["comps"] == [0]]
    assert all((S["bw"], S["bh"]) == (5, 6) for S in luma) and len(luma) == 4       # not the MCU-padded 6 x 6
    rst = parse_prog(prog["bytes_s420_64x64_rst3"].tobytes())
    assert all(S["ri"] == 3 for S in rst["scans"]) and [len(S["lanes"]) for S in rst["scans"]][:2] == [6, 22]
    cut, status, _ = np_decode_prog(prog["bytes_truncated"].tobytes(), with_status=True)
    assert status & TRUNCATED and len(parse_prog(prog["bytes_truncated"].tobytes())["scans"]) == 6
    assert sum(v.size for k, v in prog.items() if k.startswith("bytes_")) < 100000


def test_restatement_equals_pil_on_the_partial_files(prog):
    for name in PARTIAL:
        got, status, P = np_decode_prog(prog["bytes_" + name].tobytes(), with_status=True)
        assert status == OK and P["progressive"], name
        want = prog["pix_" + name]
        print(name, "largest difference from PIL", int(np.abs(got.astype(int) - want).max()))
        assert got.shape == want.shape and np.array_equal(got, want), name


def test_restatement_decodes_the_baseline_fixtures_too(golden):
    for name in [str(n) for n in golden["names"]]:
        got, status, P = np_decode_prog(golden["bytes_" + name].tobytes(), with_status=True)
        assert status == OK and not P["progressive"] and len(P["scans"]) == 1 and np.array_equal(got, golden["pix_" + name]), name


# ------------------------------------------------------------------------------------------------ xm_jpeg_plan_prog, no device
def plan_parts(buf, plan):
    N, sizes = plan["N"], plan["sizes"]
    part = lambda k: buf[plan[k][0]:plan[k][0] + plan[k][1]]
    desc = part("desc").view(np.int64).reshape(N, DESC)
    scans = part("scans").view(np.int64).reshape(-1, SCAN)
    lanes = part("lanes").view(np.int64).reshape(-1, LANE)
    tables = part("tables")
    nq, nh = int(sizes[1]), int(sizes[2])
    assert tables.size == nq * QT_BYTES + nh * HT_BYTES == sizes[0]
    return desc, scans, lanes, tables[:nq * QT_BYTES].view(np.uint16).reshape(nq, 64), tables[nq * QT_BYTES:].reshape(nh, HT_BYTES)


def test_plan_equals_the_restatements_parse(prog, golden):
    from mcncrossmodalemotions_amd import vl
    names = names_of(prog) + PARTIAL + ["truncated"]
    files = [prog["bytes_" + n].tobytes() for n in names] + [golden["bytes_s420_64x64_rst"].tobytes()]
    names = names + ["baseline"]
    buf, plan = vl.jpeg_plan(files, progressive=True)
    desc, scans, lanes, qt, ht = plan_parts(buf, plan)
    sizes = plan["sizes"]
    assert sizes[7] == len(files) and sizes[8] == scans.shape[0] and sizes[6] == lanes.shape[0] and tuple(sizes[9:]) == (3, 1)
    base, coef, pix, row, lane = 0, 0, 0, 0, 0
    for i, f in enumerate(files):
        P, d = parse_prog(f), desc[i]
        first, last = P["scans"][0], P["scans"][-1]
        assert (d[0], d[1]) == (base + first["b0"], base + last["b1"]), names[i]
        assert (d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9]) == (P["H"], P["W"], len(P["comps"])) + P["comps"][0][:2] + (
            first["ri"], P["mx"], P["my"]), names[i]
        for c in range(3):
            assert np.array_equal(qt[d[10 + c]], P["qt"][P["comps"][c if c < len(P["comps"]) else 0][2]]), (names[i], c)
        smoothed = P["progressive"] and any(v != 0 for b in P["coef_bits"] for v in b[1:])     # libjpeg's smoothing_ok
        assert smoothed == (names[i] in PARTIAL + ["truncated"]), names[i]
        for c in range(len(P["comps"]) if P["progressive"] else 0):
            want = (1 << 40) + sum((b + 1) << (4 * z) for z, b in enumerate(P["coef_bits"][c])) if smoothed else 0
            assert d[13 + c] == want, (names[i], c)
        nblocks = sum(P["mx"] * P["my"] * c[0] * c[1] for c in P["comps"])
        assert (d[19], d[20], d[21], d[22], d[23]) == (coef, coef, pix, lane, sum(len(S["lanes"]) for S in P["scans"])), names[i]
        for k, S in enumerate(P["scans"]):
            s, ns, tag = scans[row], len(S["comps"]), (names[i], k)
            assert (s[0], s[1]) == (i, ns) and list(s[2:5]) == S["comps"] + [-1] * (3 - ns), tag
            assert tuple(s[5:9]) == (S["Ss"], S["Se"], S["Ah"], S["Al"]) and s[23] == S["kind"], tag
            assert (s[15], s[16]) == (base + S["b0"], base + S["b1"]) and (s[17], s[18]) == (S["bw"], S["bh"]), tag
            assert (s[19], s[20], s[21], s[22]) == (S["level"], lane, len(S["lanes"]), S["ri"]), tag
            for j in range(ns):                                         # table slots by content, as DHT stood at the scan
                if S["dc"][j] is not None:
                    assert ht[s[9 + j]].tobytes() == table_bytes(*S["dc"][j]), tag
                if S["ac"][j] is not None:
                    assert ht[s[12 + j]].tobytes() == table_bytes(*S["ac"][j]), tag
            for b, e, m0 in S["lanes"]:
                assert tuple(lanes[lane]) == (row, base + b, base + e, m0), tag
                lane += 1
            row += 1
        base, coef, pix = base + len(f), coef + 64 * nblocks, pix + 3 * P["H"] * P["W"]
    assert (sizes[3], sizes[4], sizes[5]) == (coef, coef, pix) and row == scans.shape[0] and lane == lanes.shape[0]
    assert ht.shape[0] < scans.shape[0]                                 # equal tables share a slot
    k = names.index("s420_41x35")
    luma = [s for s in scans if s[0] == k and s[1] == 1 and s[2] == 0]
    assert len(luma) == 4 and all((s[17], s[18]) == (5, 6) for s in luma) and (desc[k][8] * 2, desc[k][9] * 2) == (6, 6)


def sos_at(data, k):
    """offset of the FF of SOS number k"""
    pos, seen = 2, 0
    while True:
        m = data[pos + 1]
        end = pos + 2 + int.from_bytes(data[pos + 2:pos + 4], "big")
        if m == 0xDA:
            if seen == k:
                return pos
            seen += 1
            end = scan_end(data, end)[0]
        pos = end


def test_bad_scan_scripts_are_refused_with_file_and_scan(prog):
    from mcncrossmodalemotions_amd import _lib, vl
    ok = prog["bytes_s420_16x16"].tobytes()
    P = parse_prog(ok)
    assert [(S["Ss"], S["Se"], S["Ah"], S["Al"]) for S in P["scans"]][:6] == [(0, 0, 0, 1), (1, 5, 0, 2), (1, 63, 0, 1), (1, 63, 0, 1),
                                                                             (6, 63, 0, 2), (1, 63, 2, 1)]

    def patched(k, **kw):
        """scan k's SOS with Ss / Se / AhAl replaced (offsets past the component list)"""
        o = sos_at(ok, k)
        ns = ok[o + 4]
        bad = bytearray(ok)
        for name, rel in (("Ss", 0), ("Se", 1), ("AhAl", 2)):
            if name in kw:
                bad[o + 5 + 2 * ns + rel] = kw[name]
        return bytes(bad)

    o = sos_at(ok, 1)
    assert ok[o + 2:o + 5] == b"\x00\x08\x01"
    two = ok[:o + 2] + b"\x00\x0a\x02" + ok[o + 5:o + 7] + bytes([2, ok[o + 6]]) + ok[o + 7:]      # scan 1 with Y and Cb
    cases = [(patched(1, Ss=6), 1, "need Ss <= Se <= 63"), (patched(0, Se=5), 0, "mixes DC and AC"), (two, 1, "an AC scan of 2 components"),
             (patched(5, AhAl=0x31), 5, "Ah 3 is not Al \\+ 1"), (patched(1, AhAl=0x32), 1, "which no earlier scan sent"),
             (patched(2, AhAl=0x0E), 2, "Al 14"), (patched(4, Ss=5), 4, "sent twice")]
    for bad, k, msg in cases:
        with pytest.raises((Malformed, ValueError)):
            parse_prog(bad)
        with pytest.raises(_lib.XmError, match=r"file 1: scan %d: .*%s" % (k, msg)) as e:
            vl.jpeg_plan([ok, bad, ok], progressive=True)
        assert e.value.code == 1, msg                                                  # XM_EINVAL
    # valid files this build does not decode: XM_ENOTSUP with the file's index
    f = ok.index(b"\xff\xc2")
    for at, val, msg in [(f + 1, 0xC1, "file 2: SOF1 "), (f + 1, 0xC9, "file 2: SOF9 "), (f + 1, 0xC3, "file 2: SOF3 "),
                         (f + 4, 12, "file 2: 12-bit"), (f + 9, 4, "file 2: 4 components")]:
        bad = bytearray(ok)
        bad[at] = val
        with pytest.raises(_lib.XmError, match=msg) as e:
            vl.jpeg_plan([ok, ok, bytes(bad)], progressive=True)
        assert e.value.code == 5, msg                                                  # XM_ENOTSUP
    # a legal script of 312 scans (the plan reads no entropy data): chroma one coefficient at a time, twice; the cap is 256
    sos = lambda cid, k, ahal: b"\xff\xda\x00\x08\x01" + bytes([cid, 0, k, k, ahal])
    many = ok[:sos_at(ok, 2)] + b"".join(sos(cid, k, ahal) for cid in (2, 3) for ahal in (0x01, 0x10) for k in range(1, 64))
    many += b"".join(sos(1, k, 0x02) for k in range(6, 64)) + b"\xff\xd9"
    assert len(parse_prog(many[:many.index(sos(2, 63, 0x10))])["scans"]) == 2 + 63 + 62
    with pytest.raises(_lib.XmError, match="file 0: more than 256 scans") as e:
        vl.jpeg_plan([many], progressive=True)
    assert e.value.code == 5
    with pytest.raises(_lib.XmError, match=r"file 1: no SOI") as e:
        vl.jpeg_plan([ok, b"not a jpeg file"], progressive=True)
    assert e.value.code == 1
    # the default still refuses the file (tests/test_jpeg_cpu.py pins the message)
    with pytest.raises(_lib.XmError, match=r"file 0: SOF2") as e:
        vl.jpeg_plan([ok])
    assert e.value.code == 5


def test_baseline_batch_plans_as_xm_jpeg_plan(golden):
    from mcncrossmodalemotions_amd import vl
    names = [str(n) for n in golden["names"]] + ["truncated"]
    files = [golden["bytes_" + n].tobytes() for n in names]
    buf0, plan0 = vl.jpeg_plan(files)
    buf1, plan1 = vl.jpeg_plan(files, progressive=True)
    for k in ("desc", "lanes", "tables"):                               # one scan per image: scan row == image index
        assert plan0[k][1] == plan1[k][1], k
        assert np.array_equal(buf0[plan0[k][0]:plan0[k][0] + plan0[k][1]], buf1[plan1[k][0]:plan1[k][0] + plan1[k][1]]), k
    assert np.array_equal(plan0["sizes"], plan1["sizes"][:8]) and tuple(plan1["sizes"][8:]) == (len(files), 1, 0)
    _, scans, lanes, _, _ = plan_parts(buf1, plan1)
    assert np.array_equal(scans[:, 0], np.arange(len(files))) and (scans[:, 23] == SEQ).all() and (scans[:, 19] == 0).all()
    with pytest.raises(Exception, match="multi-scan SOF0"):             # a baseline frame whose first scan is partial
        ok = golden["bytes_s420_16x16"].tobytes()
        o = sos_at(ok, 0)
        vl.jpeg_plan([ok[:o + 2] + b"\x00\x08\x01" + ok[o + 5:o + 7] + ok[o + 11:]], progressive=True)


def test_plan_arguments_are_rejected_without_a_device(prog):
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    ok = prog["bytes_grey_8x8"].tobytes()
    data = np.frombuffer(ok, np.uint8).copy()
    offs = np.array([0, len(ok)], np.int64)
    desc, scans, lanes, tabs, sizes = (np.zeros(DESC, np.int64), np.zeros(8 * SCAN, np.int64), np.zeros(8 * LANE, np.int64),
                                       np.zeros(16384, np.uint8), np.zeros(11, np.int64))
    p = lambda a: C.c_void_p(a.ctypes.data)
    g = lambda **k: [k.get("bytes", p(data)), p(offs), k.get("N", 1), p(desc), k.get("scans", p(scans)), k.get("scans_cap", 8),
                     p(lanes), k.get("lanes_cap", 8), p(tabs), k.get("tables_cap", 16384), k.get("sizes", p(sizes))]
    assert L.xm_jpeg_plan_prog(*g()) == 0 and tuple(sizes[6:]) == (6, 1, 6, 3, 0) and desc[2] == 8
    for bad, msg in [(dict(N=-1), b"N >= 0"), (dict(scans_cap=-1), b"scans_cap >= 0"), (dict(bytes=None), b"NULL"),
                     (dict(scans=None), b"NULL"), (dict(sizes=None), b"NULL")]:
        assert L.xm_jpeg_plan_prog(*g(**bad)) == 1 and msg in L.xm_last_error(), bad
    assert L.xm_jpeg_plan_prog(*g(scans_cap=2)) == 2 and sizes[8] == 6            # XM_ENOMEM, the need is reported
    assert L.xm_jpeg_plan_prog(*g(lanes_cap=0)) == 2 and sizes[6] == 6
    assert L.xm_jpeg_plan_prog(*g(tables_cap=16)) == 2 and sizes[0] > 16
    assert L.xm_jpeg_plan_prog(*g(N=0, bytes=None)) == 0
    # the device entry rejects its arguments before it touches a device
    one = C.c_void_p(4096)
    d = lambda **k: [one, 100, one, k.get("N", 1), one, k.get("nlanes", 6), one, 1, 1, 64, 64, 192, None, None, 0.5, 8, 8, None, one,
                     k.get("scans", one), k.get("nscans", 6), k.get("levels", 3), 0, None]
    for bad, msg in [(dict(scans=None), b"scans"), (dict(scans=C.c_void_p(4100)), b"aligned"), (dict(levels=0), b"levels"),
                     (dict(levels=15), b"levels"), (dict(nscans=0), b"nscans"), (dict(nlanes=2), b"nscans"), (dict(N=-1), b"negative")]:
        assert L.xm_jpeg_decode_batch_prog(*d(**bad)) == 1 and msg in L.xm_last_error(), bad
    assert L.xm_jpeg_decode_batch_prog(*d(N=0)) == 0


def test_progressive_excludes_split_before_anything_else():
    from mcncrossmodalemotions_amd import external, fetch_emovoxceleb_imdb as fe, vl
    with pytest.raises(ValueError, match="progressive=True and split="):
        vl.imreadjpeg([b""], progressive=True, split=64, prefetch=True)
    with pytest.raises(ValueError, match="progressive=True and split="):
        fe.getImageBatch(["a.jpg"], None, read=lambda ps: [b""], split=64, progressive=True)
    with pytest.raises(ValueError, match="progressive=True and split="):
        fe.buildImdb(None, None, read=lambda ps: [b""], split=64, progressive=True)
    with pytest.raises(ValueError, match="progressive=True and split="):
        external.compute_visual_feats(None, [], read=lambda ps: [b""], split=64, progressive=True)


def test_jpeg_prog_abi_declared_typed_and_exported():
    from mcncrossmodalemotions_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "xmodal.h")).read()
    L = _lib.load()
    assert L.xm_version() >= 120
    assert "jpeg_prog.hip" in build.SOURCES and "jpeg_scan_plan.h" in build.HEADERS
    for name in NEW_ABI:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name]
        proto = re.search(r"\bint %s\(([^;]*)\);" % name, hdr).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name]), name
    for k, v in (("XM_JPEG_SCAN", SCAN), ("XM_JPEG_PROG_SIZES", 11), ("XM_JPEG_MAX_LEVELS", 14), ("XM_JPEG_SCAN_AC_REFINE", AC_REFINE)):
        assert re.search(r"%s = %d\b" % (k, v), hdr), k


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host compiler")
def test_the_plan_header_is_pure_host_code():
    src = os.path.join(ROOT, "mcncrossmodalemotions_amd", "csrc", "jpeg_scan_plan.h")
    unit = '#include "%s"\nint main() { return xm::jpeg_plan_prog(nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, nullptr, 0) != XM_EINVAL; }\n' % src
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-fsyntax-only", "-x", "c++", "-"],
                   input=unit.encode(), check=True)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host compiler")
def test_plan_survives_every_truncation_and_mutation_under_sanitizers(prog, tmp_path):
    exe, src = str(tmp_path / "jpeg_scan_plan_check"), os.path.join(ROOT, "tests", "jpeg_scan_plan_check.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", src, "-o", exe], check=True)
    for name in ("s420_16x16", "grey_8x8"):                             # DRI-free colour and grey; a few thousand plans each
        path = str(tmp_path / (name + ".jpg"))
        open(path, "wb").write(prog["bytes_" + name].tobytes())
        out = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout
        planned, refused = map(int, re.match(r"planned (\d+), refused (\d+)", out).groups())
        n = prog["bytes_" + name].size                                  # 2 n cuts, 2 n mutations and the whole file
        assert planned + refused == 4 * n + 1 and min(planned, refused) > n, out

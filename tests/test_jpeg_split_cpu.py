"""CPU: a numpy restatement of the segment-parallel entropy decode behind vl.imreadjpeg(split=) -- every lane cut into
segments of seg_bytes raw bytes, each decoded from a guessed state, exit states handed forward until nothing changes,
then a writing decode from block ordinals and DC predictors that an exclusive scan gives -- equal to the sequential
restatement of tests/test_jpeg_cpu.py on every fixture, on the truncated file and on corrupted ones; and the ABI of
xm_jpeg_decode_batch_split / xm_jpeg_split_geometry without a device.  The GPU tests import the helpers from here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_jpeg_cpu import (BADCODE, GOLDEN, NATURAL, OK, ROOT, TRUNCATED, Bits, decode_coefs, derived_table, extend,
                           huff_decode, np_decode, parse)

NEW_ABI = ["xm_jpeg_decode_batch_split", "xm_jpeg_split_geometry"]
ENDED = None                                                      # the state of a chain that has ended


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def corrupted(golden):
    """s444_37x29_opt with the byte at scan0 + 300 set to 0xFE: an invalid code some blocks into the image"""
    data = bytearray(golden["bytes_s444_37x29_opt"].tobytes())
    data[parse(bytes(data))["scan0"] + 300] = 0xFE
    return bytes(data)


# (fixture, seg_bytes, file offset, value): corruptions inside a segment that begins exactly where an MCU begins on a byte
# boundary, so that the thread's cold guess (first byte, block 0, k 0) IS the true state and no hand-forward ever replaces
# it.  grey_17x23: the chain stands at (8 * 360, 0, 0); s444_37x29_opt: at byte 1043.  A decode that recovered from the
# invalid symbol while guessing must not become final there.
ALIGNED = [("grey_17x23", 32, 362, 0x7F), ("grey_17x23", 32, 366, 0xFE), ("grey_17x23", 32, 368, 0x7F),
           ("grey_17x23", 16, 362, 0x7F), ("s444_37x29_opt", 16, 1045, 0x7F), ("s444_37x29_opt", 64, 1045, 0x7F),
           ("s444_37x29_opt", 176, 1046, 0xFE)]


def patched(golden, name, offset, value):
    data = bytearray(golden["bytes_" + name].tobytes())
    data[offset] = value
    return bytes(data)


def sweep(golden):
    """grey_17x23 with every fifth byte of its entropy data, in turn, set to 0x7F or 0xFE (never FF: no new marker)"""
    P = parse(golden["bytes_grey_17x23"].tobytes())
    return [patched(golden, "grey_17x23", o, 0x7F if (o // 5) & 1 else 0xFE) for o in range(P["scan0"], P["scan1"], 5)]


# ------------------------------------------------------------------------------------------------ the restatement
class Lane:
    """one restart interval: its unstuffed bits (test_jpeg_cpu.Bits) addressed by canonical positions -- 8 x the file
    offset of a delivered byte (never the 00 of an FF 00 pair) + 0 .. 7, counting on over zero bits past the end"""

    def __init__(self, data, b, e):
        self.b, self.e, self.br = b, e, Bits(data, b, e)
        self.src, self.real, self.data = self.br.src, self.br.real, data

    def to_u(self, p):
        raw = p >> 3
        if raw >= self.e:
            return self.real + p - 8 * self.e
        i = int(np.searchsorted(self.src, raw))
        assert i < self.src.size and self.src[i] == raw, "not a canonical position"
        return 8 * i + (p & 7)

    def to_p(self, u):
        return int(self.src[u >> 3]) * 8 + (u & 7) if u < self.real else 8 * self.e + u - self.real

    def guess(self, sb):
        """where a thread starts cold: the first byte of its segment, or the one after a stuffed 00"""
        if sb > self.b and sb < self.e and self.data[sb] == 0 and self.data[sb - 1] == 0xFF:
            sb += 1
        return 8 * sb


def run(L, geo, tabs, seg_end, state, guess, write=None):
    """decodes from `state` = (position, block inside the MCU, k) until a symbol starts at or past seg_end.
    write None: -> (exit state, blocks completed, DC differences summed per component, whether a guess skipped an
    invalid symbol); a chain that reaches the end of the data, or meets an invalid symbol while not guessing, exits ENDED.
    write (n, preds, store): the writing decode from block ordinal n; goes on in the tail to the end of the MCU;
    -> status bits"""
    bpm, hv, nlb = geo
    p, blk, k = state
    br = L.br
    br.pos = L.to_u(p)
    n, pred = (0, [0, 0, 0]) if write is None else (write[0], list(write[1]))
    recovered = False
    while True:
        if write is not None and n >= nlb:
            return OK
        tail = br.pos >= L.real
        if not tail and L.to_p(br.pos) >= 8 * seg_end:
            return ((L.to_p(br.pos), blk, k), n, pred, recovered) if write is None else OK
        if tail and write is None:
            return ENDED, n, pred, recovered
        c = 0 if blk < hv else blk - hv + 1
        bad = False
        if k == 0:
            s = huff_decode(br, tabs[c][0])
            if s is None or s > 15:
                bad = True
            else:
                pred[c] += extend(br.take(s), s)
                if write is not None:
                    write[2](n, 0, pred[c])
                k = 1
        else:
            rs = huff_decode(br, tabs[c][1])
            if rs is None:
                bad = True
            else:
                r, s = rs >> 4, rs & 15
                if s == 0:
                    k = 64 if r != 15 else k + 16
                else:
                    k += r
                    if k > 63:
                        bad = True
                    else:
                        v = extend(br.take(s), s)
                        if write is not None:
                            write[2](n, k, v)
                        k += 1
        if bad:
            if write is not None:
                return BADCODE | (TRUNCATED if br.pos > L.real else 0)
            if not guess:
                return ENDED, n, pred, False
            br.pos += 1                                   # a guess went wrong: one bit on, a DC symbol next
            k, recovered = 0, True
            continue
        if k >= 64:
            k, n, blk = 0, n + 1, (blk + 1) % bpm
            if write is not None and (n >= nlb or blk == 0) and br.pos > L.real:
                return TRUNCATED


def split_decode(data, P, seg_bytes, per_pass=64):
    """-> (coefs per component [by, bx, 64], status, rounds per lane, segments per lane)"""
    data = bytes(data)
    comps, mx, my = P["comps"], P["mx"], P["my"]
    tabs = [(derived_table(*P["dht"][(0, td)]), derived_table(*P["dht"][(1, ta)])) for _, _, _, td, ta in comps]
    coefs = [np.zeros((my * vs, mx * hs, 64), np.int32) for hs, vs, _, _, _ in comps]
    hs, vs = comps[0][:2]
    hv = hs * vs
    bpm = hv + (2 if len(comps) == 3 else 0)
    status, rounds, segments = OK, [], []
    for b, e, mcu0 in P["lanes"]:
        stop = min(mcu0 + P["ri"], mx * my) if P["ri"] else mx * my
        geo = (bpm, hv, (stop - mcu0) * bpm)
        L = Lane(data, b, e)

        def store(n, k, v, mcu0=mcu0):
            mcu, j = mcu0 + n // bpm, n % bpm
            ym, xm = divmod(mcu, mx)
            blk = coefs[0][ym * vs + j // hs, xm * hs + j % hs] if j < hv else coefs[j - hv + 1][ym, xm]
            blk[NATURAL[k]] = ((v & 0xFFFF) ^ 0x8000) - 0x8000 if k == 0 else v

        nseg = max(-(-(e - b) // seg_bytes), 1)
        confirmed, n0, preds, total_rounds = (8 * b, 0, 0), 0, [0, 0, 0], 0
        for seg0 in range(0, nseg, per_pass):
            if confirmed is ENDED:
                break
            nact = min(per_pass, nseg - seg0)
            ends = [min(b + (seg0 + t + 1) * seg_bytes, e) for t in range(nact)]
            entry = [confirmed] + [(L.guess(min(b + (seg0 + t) * seg_bytes, e)), 0, 0) for t in range(1, nact)]
            redo, guess = [True] * nact, [False] + [True] * (nact - 1)
            out = [None] * nact
            for r in range(nact):
                for t in range(nact):
                    if redo[t]:
                        out[t] = run(L, geo, tabs, ends[t], entry[t], guess[t])
                exits = [o[0] for o in out]
                redo, guess = [False] * nact, [False] * nact
                for t in range(1, nact):
                    if exits[t - 1] != entry[t]:
                        entry[t] = exits[t - 1]
                        redo[t] = entry[t] is not ENDED     # an ended entry: the thread keeps its result and is dead
                    elif out[t][3] and entry[t] is not ENDED:   # the guess was right, but its decode skipped an invalid
                        redo[t] = True                      # symbol: such a result never becomes final
                if not any(redo):
                    break
            assert not any(redo), "no fixed point within as many rounds as the pass has segments"
            total_rounds += r + 1
            dead = False
            for t in range(nact):                           # the scan, then every live thread writes
                dead = dead or entry[t] is ENDED
                if dead:
                    break
                status |= run(L, geo, tabs, ends[t], entry[t], False, write=(n0, preds, store))
                n0 += out[t][1]
                preds = [a + d for a, d in zip(preds, out[t][2])]
            confirmed = ENDED if dead else out[nact - 1][0]
        rounds.append(total_rounds)
        segments.append(nseg)
    return coefs, status, rounds, segments


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("seg_bytes", [16, 64, 4096])
def test_fixed_point_equals_the_sequential_decode(golden, seg_bytes):
    for name in [str(n) for n in golden["names"]]:
        data = golden["bytes_" + name].tobytes()
        P = parse(data)
        want, want_status, _ = decode_coefs(data, P)
        got, status, rounds, segments = split_decode(data, P, seg_bytes)
        assert status == want_status == OK, name
        assert same(got, want), name
        assert all(1 <= r <= s for r, s in zip(rounds, segments)), (name, rounds, segments)
        if seg_bytes == 4096:
            assert rounds == [1] * len(P["lanes"]), name
    if seg_bytes == 16:                                     # the lane the multi-pass carry is tested on
        data = golden["bytes_s420_50x50_q100"].tobytes()
        assert split_decode(data, parse(data), 16)[3] == [225]


def test_passes_of_any_length_carry_the_state(golden):
    for name in ("s420_41x35_opt", "s420_64x64_rst", "grey_8x8"):
        data = golden["bytes_" + name].tobytes()
        P = parse(data)
        want = decode_coefs(data, P)[0]
        for per_pass in (1, 2, 5):
            got, status, rounds, segments = split_decode(data, P, 16, per_pass=per_pass)
            assert status == OK and same(got, want), (name, per_pass)
            assert all(1 <= r <= s for r, s in zip(rounds, segments)), (name, per_pass)


@pytest.mark.parametrize("seg_bytes", [16, 64, 4096])
def test_truncated_file(golden, seg_bytes):
    """the decode goes on over zero bits to the end of the MCU the data ends in, sets TRUNCATED and stops; whatever
    seg_bytes is, that is what one segment (the sequential decode) gives, and the MCUs before it are the whole file's"""
    cut = golden["bytes_truncated"].tobytes()
    P = parse(cut)
    one, one_status, _, _ = split_decode(cut, P, 1 << 16)
    got, status, rounds, segments = split_decode(cut, P, seg_bytes)
    assert status == one_status == TRUNCATED == np_decode(cut, with_status=True)[1]
    assert same(got, one) and all(1 <= r <= s for r, s in zip(rounds, segments))
    ref, _, mcu_end = decode_coefs(cut, P)
    done = int(np.count_nonzero(mcu_end < (1 << 62)))       # MCUs whose last bit lies before the cut
    assert 0 < done < P["mx"] * P["my"]
    hs, vs = P["comps"][0][:2]
    for mcu in range(P["mx"] * P["my"]):
        ym, xm = divmod(mcu, P["mx"])
        luma = got[0][ym * vs:(ym + 1) * vs, xm * hs:(xm + 1) * hs]
        if mcu < done:
            assert np.array_equal(luma, ref[0][ym * vs:(ym + 1) * vs, xm * hs:(xm + 1) * hs]), mcu
            assert np.array_equal(got[1][ym, xm], ref[1][ym, xm]) and np.array_equal(got[2][ym, xm], ref[2][ym, xm]), mcu
        elif mcu > done:                                     # past the MCU the data ends in nothing is written
            assert not luma.any() and not got[1][ym, xm].any() and not got[2][ym, xm].any(), mcu


@pytest.mark.parametrize("seg_bytes", [16, 64, 4096])
def test_corrupted_file(golden, seg_bytes):
    data = corrupted(golden)
    assert np_decode(data, with_status=True)[1] == BADCODE
    P = parse(data)
    want, want_status, _ = decode_coefs(data, P)
    got, status, rounds, segments = split_decode(data, P, seg_bytes)
    assert status == want_status == BADCODE
    assert same(got, want) and any(c.any() for c in got)
    assert all(1 <= r <= s for r, s in zip(rounds, segments))


def test_corruption_where_a_cold_guess_is_the_true_state(golden):
    """against the sequential decode_coefs, which shares nothing with the rounds"""
    for name, seg_bytes, offset, value in ALIGNED:
        whole = golden["bytes_" + name].tobytes()
        P = parse(whole)
        # the premise: a segment boundary before the patched byte where the sequential decode ends an MCU byte-aligned
        sb = P["scan0"] + (offset - P["scan0"]) // seg_bytes * seg_bytes
        assert sb in decode_coefs(whole, P)[2].tolist(), (name, seg_bytes)
        data = patched(golden, name, offset, value)
        P = parse(data)
        want, want_status, _ = decode_coefs(data, P)
        got, status, rounds, segments = split_decode(data, P, seg_bytes)
        assert status == want_status == BADCODE, (name, seg_bytes, offset)
        assert same(got, want), (name, seg_bytes, offset)
        assert all(1 <= r <= s for r, s in zip(rounds, segments))


@pytest.mark.parametrize("seg_bytes", [16, 32])
def test_corruption_sweep(golden, seg_bytes):
    """every variant equals what one segment -- the sequential decode, which never guesses -- gives, and decode_coefs
    where that is comparable (it decodes on past a truncation, the kernels stop at the MCU)"""
    statuses = set()
    for data in sweep(golden):
        P = parse(data)
        one, one_status, _, _ = split_decode(data, P, 1 << 16)
        got, status, rounds, segments = split_decode(data, P, seg_bytes)
        assert status == one_status and same(got, one)
        assert all(1 <= r <= s for r, s in zip(rounds, segments))
        if not status & TRUNCATED:
            want, want_status, _ = decode_coefs(data, P)
            assert want_status == status and same(got, want)
        statuses.add(status)
    assert BADCODE in statuses


def test_split_abi_declared_typed_and_exported():
    from mcncrossmodalemotions_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "xmodal.h")).read()
    L = _lib.load()
    assert L.xm_version() >= 115
    for name in NEW_ABI:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name]
        proto = re.search(r"\bint %s\(([^;]*)\);" % name, hdr).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name]), name
    # the split entry takes every argument of xm_jpeg_decode_batch up to status, then seg_bytes, rounds, stream
    plain, split = _lib.SIGNATURES["xm_jpeg_decode_batch"], _lib.SIGNATURES["xm_jpeg_decode_batch_split"]
    assert split[:len(plain) - 1] == plain[:-1] and len(split) == len(plain) + 2


def test_geometry_answers_without_a_device():
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    spp, launches = C.c_int(0), C.c_int(0)
    assert L.xm_jpeg_split_geometry(C.byref(spp), C.byref(launches)) == 0
    assert 1 <= spp.value <= 111 and launches.value == 5    # the unsplit path's launch count (tests/test_gpu_jpeg.py)
    assert L.xm_jpeg_split_geometry(None, None) == 0


def test_seg_bytes_is_checked_before_any_device_call():
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    one = C.c_void_p(4096)
    args = lambda seg, **k: [one, 100, one, k.get("N", 1), one, 1, one, 1, 2, 64, 64, 192, None, None, 0.5, 8, 8, None,   # noqa: E731
                             k.get("status", one), seg, None, None]
    for seg in (0, 8, 24, 65552, -16):
        assert L.xm_jpeg_decode_batch_split(*args(seg)) == 1 and b"seg_bytes" in L.xm_last_error(), seg
    # a valid seg_bytes reaches the checks of xm_jpeg_decode_batch, still in front of the device
    assert L.xm_jpeg_decode_batch_split(*args(64, status=None)) == 1 and b"NULL" in L.xm_last_error()
    assert L.xm_jpeg_decode_batch_split(*args(65536, N=-1)) == 1 and b"negative" in L.xm_last_error()
    assert L.xm_jpeg_decode_batch_split(*args(16, N=0)) == 0

"""CPU: the host side of the FER2013 CSV path.  xm_pixcsv_plan against a restatement of its rules written here (py_plan)
for files with and without a header, reordered columns, quoted and plain pixel fields, LF and CRLF, a byte order mark,
blank lines, no final newline, missing `emotion` / `Usage` columns and unknown usage strings; every documented rejection
with its code and its line; counting with desc == NULL.  The vote-file reader and the keep rule of getFerPlusImdb on a
hand-written 12-row pair; benchmark_ferplus_models' cache / refresh logic with ferplus_baselines stubbed.  Nothing here
opens a device.  tests/pixcsv_plan_check.cpp -- csrc/pixcsv_plan.h alone, every truncation and single-byte mutation of
small valid files -- is built with the address and undefined-behaviour sanitizers and run as a program of its own."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
USAGES = ("Training", "PublicTest", "PrivateTest")


class Rejected(Exception):
    def __init__(self, line, what):
        super().__init__("line %d: %s" % (line, what))
        self.line, self.what = line, what


def split_fields(data, a, b):
    """byte ranges of the fields of data[a:b], split at commas outside double quotes; None if a quote stays open"""
    out, start, quoted = [], a, False
    for p in range(a, b):
        if data[p:p + 1] == b'"':
            quoted = not quoted
        elif data[p:p + 1] == b"," and not quoted:
            out.append((start, p))
            start = p + 1
    out.append((start, b))
    return None if quoted else out


def unquote(data, a, b, blanks):
    if b - a >= 2 and data[a:a + 1] == b'"' and data[b - 1:b] == b'"':
        a, b = a + 1, b - 1
    if blanks:
        while a < b and data[a:a + 1] in (b" ", b"\t"):
            a += 1
        while b > a and data[b - 1:b] in (b" ", b"\t"):
            b -= 1
    return a, b


def py_plan(data, max_rows=None):
    """the rules of include/xmodal.h restated: N x 8 int64 rows and [N, longest field]"""
    pos = 3 if data[:3] == b"\xef\xbb\xbf" else 0
    cols, ncols, first, rows, line = {"emotion": 0, "pixels": 1, "Usage": 2}, 3, True, [], 0
    while pos < len(data):
        eol = data.find(b"\n", pos)
        eol = len(data) if eol < 0 else eol
        a, b, pos = pos, eol, eol + 1
        line += 1
        if b > a and data[b - 1:b] == b"\r":
            b -= 1
        if a == b:
            continue
        f = split_fields(data, a, b)
        if f is None:
            raise Rejected(line, "unterminated quote")
        if first:
            first = False
            if not data[a:a + 1].isdigit():
                cols, ncols = {}, len(f)
                for k, (u, v) in enumerate(f):
                    name = data[slice(*unquote(data, u, v, True))].decode("latin-1")
                    if name in ("emotion", "pixels", "Usage") and name not in cols:
                        cols[name] = k
                if "pixels" not in cols:
                    raise Rejected(line, "no pixels column")
                continue
        if len(f) < ncols:
            raise Rejected(line, "fields")
        if max_rows is not None and len(rows) >= max_rows:
            raise Rejected(line, "max_rows")
        pa, pb = unquote(data, *f[cols["pixels"]], False)
        emotion, usage = -1, -1
        if "emotion" in cols:
            s = data[slice(*unquote(data, *f[cols["emotion"]], True))]
            if 0 < len(s) <= 9 and all(48 <= c <= 57 for c in s):
                emotion = int(s)
        if "Usage" in cols:
            s = data[slice(*unquote(data, *f[cols["Usage"]], True))].decode("latin-1")
            usage = USAGES.index(s) if s in USAGES else -1
        rows.append([pa, pb, emotion, usage, line, len(rows), 0, 0])
    rows = np.array(rows, np.int64).reshape(len(rows), 8)
    return rows, [len(rows), int((rows[:, 1] - rows[:, 0]).max()) if len(rows) else 0]


def c_plan(data, max_rows=None, count_only=False):
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    buf = np.frombuffer(data, np.uint8)
    sizes = np.full(2, -7, np.int64)
    p = C.c_void_p(buf.ctypes.data) if buf.size else None
    if count_only:
        return L.xm_pixcsv_plan(p, buf.size, None, 0, C.c_void_p(sizes.ctypes.data)), None, list(sizes), L.xm_last_error().decode()
    cap = max_rows if max_rows is not None else max(1, data.count(b"\n") + 1)
    desc = np.full((cap + 1, 8), -99, np.int64)                    # one guard row behind what the call may write
    rc = L.xm_pixcsv_plan(p, buf.size, C.c_void_p(desc.ctypes.data), cap, C.c_void_p(sizes.ctypes.data))
    assert (desc[cap] == -99).all()
    return rc, desc, list(sizes), L.xm_last_error().decode()


def fer_file(rng, n, header=True, order=("emotion", "pixels", "Usage"), quote=False, eol=b"\n", bom=False, blanks=(),
             final_newline=True, numbers=6, usages=USAGES + ("Other", "")):
    """a seeded FER-style file: n rows of `numbers` values with 1 .. 3 digits"""
    lines = [",".join(order).encode()] if header else []
    for i in range(n):
        px = " ".join(str(int(v)) for v in rng.integers(0, 256, numbers)).encode()
        if quote == "mixed":
            px = b'"' + px + b'"' if i % 2 else px
        elif quote:
            px = b'"' + px + b'"'
        fields = {"emotion": str(int(rng.integers(0, 7))).encode() if i % 5 != 4 else b"",   # (an empty first field would make line 1 a header)
                  "pixels": px, "Usage": usages[i % len(usages)].encode()}
        lines.append(b",".join(fields[c] for c in order))
        if i in blanks:
            lines.append(b"")
    body = eol.join(lines) + (eol if final_newline else b"")
    return (b"\xef\xbb\xbf" if bom else b"") + body


CASES = {
    "header_lf": dict(),
    "no_header": dict(header=False),
    "reordered": dict(order=("Usage", "emotion", "pixels")),
    "reordered_extra": dict(order=("pixels", "Usage", "emotion")),
    "quoted": dict(quote=True),
    "mixed_quotes": dict(quote="mixed"),
    "crlf": dict(eol=b"\r\n"),
    "bom": dict(bom=True),
    "bom_crlf_no_header": dict(bom=True, eol=b"\r\n", header=False),
    "blank_lines": dict(blanks=(0, 3, 4)),
    "blank_lines_crlf": dict(blanks=(1, 2), eol=b"\r\n"),
    "no_final_newline": dict(final_newline=False),
    "no_final_newline_crlf_quoted": dict(final_newline=False, eol=b"\r\n", quote=True),
    "no_emotion": dict(order=("pixels", "Usage")),
    "no_usage": dict(order=("emotion", "pixels")),
    "pixels_only": dict(order=("pixels",)),
    "unknown_usage": dict(usages=("training", "Test", "PublicTest ", " PrivateTest", "Training")),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_plan_equals_the_restatement(case):
    import torch
    before = torch.cuda.is_initialized()
    data = fer_file(np.random.default_rng(len(case)), 11, **CASES[case])
    want, wsizes = py_plan(data)
    assert len(want) == 11
    rc, desc, sizes, msg = c_plan(data)
    assert rc == 0, msg
    assert sizes == wsizes and np.array_equal(desc[:11], want), case
    for r in want:                                                    # the restatement itself: ranges hold the numbers
        assert len(data[r[0]:r[1]].split()) == 6 and b'"' not in data[r[0]:r[1]]
    rc, _, sizes, _ = c_plan(data, count_only=True)
    assert rc == 0 and sizes == wsizes
    assert torch.cuda.is_initialized() == before


def test_plan_columns_mean_what_the_header_says():
    data = b' Usage ,"pixels",emotion,note\nPrivateTest,1 2 3,5,"x,y"\n"PublicTest"," 7  8 ","",z\nTraining,\t9,12x,\n'
    rc, desc, sizes, msg = c_plan(data)
    assert rc == 0, msg
    assert sizes == [3, 6]
    assert [bytes(data[r[0]:r[1]]) for r in desc[:3]] == [b"1 2 3", b" 7  8 ", b"\t9"]
    assert desc[:3, 2].tolist() == [5, -1, -1] and desc[:3, 3].tolist() == [2, 1, 0]
    assert desc[:3, 4].tolist() == [2, 3, 4] and desc[:3, 5].tolist() == [0, 1, 2]
    assert np.array_equal(desc[:3], py_plan(data)[0])
    # an empty file, a header alone, a byte order mark alone
    for d in (b"", b"emotion,pixels,Usage\n", b"\xef\xbb\xbf", b"\n\r\n\n"):
        rc, _, sizes, _ = c_plan(d)
        assert rc == 0 and sizes == [0, 0]


REJECTIONS = [
    (b'emotion,pixels,Usage\n0,1 2,Training\n1,"3 4,Training\n', 3, "unterminated quote"),
    (b'0,1 2,Training\n\n1,3 4,"Training\n', 3, "unterminated quote"),
    (b'emotion,"pixels,Usage\n', 1, "unterminated quote"),
    (b"emotion,pixels,Usage\n0,1 2,Training\n\r\n1,3 4\n", 4, "fields"),
    (b"0,1 2,Training\n1\n", 2, "fields"),
    (b"\xef\xbb\xbfemotion,Usage\n0,Training\n", 1, "pixels column"),
    (b"Emotion,Pixels,usage\n0,1 2,Training\n", 1, "pixels column"),
]


@pytest.mark.parametrize("k", range(len(REJECTIONS)))
def test_every_rejection_gives_its_code_and_its_line(k):
    data, line, what = REJECTIONS[k]
    with pytest.raises(Rejected) as e:
        py_plan(data)
    assert e.value.line == line
    for count_only in (False, True):
        rc, _, sizes, msg = c_plan(data, count_only=count_only)
        assert rc == EINVAL and "line %d:" % line in msg and what in msg, msg
        assert sizes == [0, 0]


def test_more_rows_than_max_rows_and_bad_arguments():
    from mcncrossmodalemotions_amd import _lib, vl
    L = _lib.load()
    data = fer_file(np.random.default_rng(1), 5, blanks=(1,))
    want, _ = py_plan(data)
    rc, desc, _, msg = c_plan(data, max_rows=3)
    assert rc == EINVAL and "line %d:" % want[3, 4] in msg and "max_rows" in msg
    assert np.array_equal(desc[:3], want[:3])
    with pytest.raises(Rejected) as e:
        py_plan(data, max_rows=3)
    assert e.value.line == want[3, 4]
    rc, desc, sizes, _ = c_plan(data, max_rows=5)
    assert rc == 0 and sizes[0] == 5
    sizes = np.zeros(2, np.int64)
    assert L.xm_pixcsv_plan(None, 0, None, 0, None) == EINVAL and b"NULL sizes" in L.xm_last_error()
    assert L.xm_pixcsv_plan(None, 5, None, 0, C.c_void_p(sizes.ctypes.data)) == EINVAL
    assert L.xm_pixcsv_plan(None, -1, None, 0, C.c_void_p(sizes.ctypes.data)) == EINVAL
    # the decode entry point refuses before any device call
    assert L.xm_pixcsv_decode_batch(None, 0, None, 0, 48, 48, 1, None, 0, None, None) == 0
    assert L.xm_pixcsv_decode_batch(None, 0, None, -1, 48, 48, 1, None, 0, None, None) == EINVAL
    assert L.xm_pixcsv_decode_batch(None, 0, None, 0, 48, 48, 2, None, 0, None, None) == EINVAL
    assert L.xm_pixcsv_decode_batch(None, 16, None, 1, 48, 48, 1, None, 0, None, None) == EINVAL and b"NULL" in L.xm_last_error()
    assert L.xm_pixcsv_decode_batch(C.c_void_p(16), 16, C.c_void_p(8), 1, 0, 48, 1, C.c_void_p(4), 64, C.c_void_p(4), None) == EINVAL
    assert L.xm_pixcsv_decode_batch(C.c_void_p(24), 16, C.c_void_p(8), 1, 2, 2, 1, C.c_void_p(4), 64, C.c_void_p(4), None) == EINVAL
    assert b"aligned" in L.xm_last_error()
    assert L.xm_pixcsv_decode_batch(C.c_void_p(16), 16, C.c_void_p(8), 1, 2, 2, 1, C.c_void_p(4), 3, C.c_void_p(4), None) == EINVAL
    assert b"holds no image" in L.xm_last_error()
    bpp, launches = vl.pixcsv_geometry()
    assert bpp % 16 == 0 and bpp >= 256 and launches == 1
    # vl.pixcsv_plan: the same rows, and the chunk cutter keeps rows whole
    plan = vl.pixcsv_plan(data)
    assert plan["N"] == 5 and np.array_equal(plan["rows"], want) and plan["nbytes"] == len(data)
    cuts = vl._pix_chunks(plan["rows"], 40)
    assert cuts[0][0] == 0 and cuts[-1][1] == 5 and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:])) and len(cuts) >= 3
    assert vl._pix_chunks(plan["rows"], 1) == [(i, i + 1) for i in range(5)]
    assert vl._pix_chunks(plan["rows"], None) == [(0, 5)]


# ------------------------------------------------------------------------------------------------ the vote file
VOTE_HEADER = "Usage,Image name,neutral,happiness,surprise,sadness,anger,disgust,fear,contempt,unknown,NF"
# 12 rows: two removed by FER+ (no name), one with no vote among the eight emotions, one tie (first argmax)
VOTES = [
    ("Training", "fer0000000.png", [4, 0, 0, 1, 3, 2, 0, 0, 0, 0]),
    ("Training", "fer0000001.png", [0, 10, 0, 0, 0, 0, 0, 0, 0, 0]),
    ("Training", "", [0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ("Training", "fer0000003.png", [0, 0, 0, 0, 0, 0, 0, 0, 7, 3]),
    ("Training", "fer0000004.png", [0, 0, 5, 0, 5, 0, 0, 0, 0, 0]),
    ("Training", "fer0000005.png", [1, 1, 1, 1, 1, 1, 1, 3, 0, 0]),
    ("PublicTest", "fer0000006.png", [0, 0, 0, 8, 0, 0, 0, 0, 2, 0]),
    ("PublicTest", "", [0, 0, 0, 0, 0, 0, 0, 0, 0, 10]),
    ("PublicTest", "fer0000008.png", [2, 0, 0, 0, 0, 0, 8, 0, 0, 0]),
    ("PrivateTest", "fer0000009.png", [0, 0, 0, 0, 0, 9, 0, 0, 1, 0]),
    ("PrivateTest", "fer0000010.png", [3, 3, 0, 0, 0, 0, 0, 0, 4, 0]),
    ("PrivateTest", "fer0000011.png", [0, 0, 0, 0, 6, 0, 0, 0, 0, 4]),
]


def write_pair(d, votes=VOTES, pix_usage=None, pix_rows=None):
    rng = np.random.default_rng(4)
    n = len(votes) if pix_rows is None else pix_rows
    with open(os.path.join(d, "fer2013new.csv"), "w") as fh:
        fh.write(VOTE_HEADER + "\n" + "".join("%s,%s,%s\n" % (u, name, ",".join(map(str, v))) for u, name, v in votes))
    with open(os.path.join(d, "fer2013.csv"), "w") as fh:
        fh.write("emotion,pixels,Usage\n")
        for i in range(n):
            u = (pix_usage or {}).get(i, votes[i % len(votes)][0])
            fh.write("%d,%s,%s\n" % (i % 7, " ".join(str(int(v)) for v in rng.integers(0, 256, 4)), u))


def test_vote_reader_and_keep_rule(tmp_path):
    import torch
    from mcncrossmodalemotions_amd import batch
    before = torch.cuda.is_initialized()
    d = str(tmp_path)
    write_pair(d)
    usage, names, votes, lines = batch.readFerPlusVotes(os.path.join(d, "fer2013new.csv"))
    assert usage == [v[0] for v in VOTES] and names == [v[1] for v in VOTES]
    assert np.array_equal(votes, np.array([v[2] for v in VOTES], float)) and lines.tolist() == list(range(2, 14))
    full = batch.ferPlusPlan(d, "full")
    assert np.nonzero(~full["keep"])[0].tolist() == [2, 7]                                   # the two without a name
    assert full["plan"]["rows"][:, 5].tolist() == [0, 1, -1, 2, 3, 4, 5, -1, 6, 7, 8, 9]
    assert full["row"].tolist() == [2, 3, 5, 6, 7, 8, 10, 11, 12, 13]
    assert full["sets"].tolist() == [1, 1, 1, 1, 1, 2, 2, 3, 3, 3]
    assert full["ferLabels"].tolist() == [0, 1, 3, 4, 5, 6, 1, 2, 3, 4]
    assert np.array_equal(full["votes"][2], [0, 0, 0, 0, 0, 0, 0, 0, 7, 3])                 # zero first eight: kept
    for dt in ("CNTK", "clean"):
        h = batch.ferPlusPlan(d, dt)
        assert np.nonzero(~h["keep"])[0].tolist() == [2, 3, 7]                               # ... and dropped here
        assert h["plan"]["rows"][:, 5].tolist() == [0, 1, -1, -1, 2, 3, 4, -1, 5, 6, 7, 8]
        assert (h["votes"][:, :8].sum(1) > 0).all() and h["row"].tolist() == [2, 3, 6, 7, 8, 10, 11, 12, 13]
    with pytest.raises(ValueError, match="uknown number of classes"):
        batch.ferPlusPlan(d, "other")
    # the imdb object itself: hard labels are the first argmax over the eight emotions, 1-based
    imdb = batch.FerPlusImdb(None, h["votes"], h["sets"], h["ferLabels"], h["row"])
    assert imdb.images["hardLabels"].shape == (1, 9)
    assert imdb.images["hardLabels"].ravel().tolist() == [1, 2, 3, 8, 4, 7, 6, 1, 5]
    assert imdb.meta["classes"] == batch.FERPLUS_CLASSES and imdb.set is imdb.images["set"]
    assert torch.cuda.is_initialized() == before


def test_vote_file_must_match_the_pixel_file(tmp_path):
    from mcncrossmodalemotions_amd import batch
    d = str(tmp_path)
    write_pair(d, pix_usage={8: "PrivateTest"})
    with pytest.raises(ValueError, match=r"fer2013new.csv: line 10: Usage 'PublicTest'.*line 10") as e:
        batch.ferPlusPlan(d)
    assert "PrivateTest" in str(e.value)
    write_pair(d, pix_rows=11)
    with pytest.raises(ValueError, match="11 rows.*12"):
        batch.ferPlusPlan(d)
    write_pair(d, votes=VOTES[:5] + [("Validation", "x.png", [1] * 10)] + VOTES[6:], pix_usage={5: "Validation"})
    with pytest.raises(ValueError, match="line 7: Usage 'Validation'"):
        batch.ferPlusPlan(d)
    write_pair(d)
    p = os.path.join(d, "fer2013new.csv")
    txt = open(p).read()
    open(p, "w").write(txt.replace("Image name", "name"))
    with pytest.raises(ValueError, match="header"):
        batch.ferPlusPlan(d)
    open(p, "w").write(txt.replace("fer0000004.png,0,0,5", "fer0000004.png,0,zero,5"))
    with pytest.raises(ValueError, match="line 6: a vote is not a number"):
        batch.ferPlusPlan(d)


# ------------------------------------------------------------------------------------------------ benchmark_ferplus_models
def test_benchmark_cache_and_refresh(tmp_path, monkeypatch, capsys):
    from mcncrossmodalemotions_amd import benchmark_ferplus_models as bm
    calls = []

    def stub(**kw):
        calls.append(kw)
        err = {"val": 0.25, "test": 0.5}[kw["evaluateOnly"]["subset"]] + (0.125 if kw["modelName"].startswith("senet") else 0)
        return None, {"train": [{"num": 0}], "val": [{"classerror": err, "objective": 1.0}]}

    monkeypatch.setattr(bm, "ferplus_baselines", stub)
    cache = str(tmp_path / "cache" / "deep")
    res = bm.benchmark_ferplus_models(dataDir="somewhere", benchmarkCacheDir=cache, widthMult=0.125, blocks=(1, 1, 1, 1), seed=3)
    assert res == {"resnet50-ferplus": {"valAcc": 0.75, "testAcc": 0.5}, "senet50-ferplus": {"valAcc": 0.625, "testAcc": 0.375}}
    assert [(c["modelName"], c["lossType"], c["evaluateOnly"]["subset"]) for c in calls] == [
        ("resnet50-ferplus", "softmaxlog", "val"), ("resnet50-ferplus", "softmaxlog", "test"),
        ("senet50-ferplus", "distributions", "val"), ("senet50-ferplus", "distributions", "test")]
    assert all(c["batchSize"] == 32 and c["dataDir"] == "somewhere" and c["widthMult"] == 0.125 and c["seed"] == 3 for c in calls)
    assert sorted(os.listdir(cache)) == ["resnet50-ferplus.json", "senet50-ferplus.json"]
    assert json.load(open(os.path.join(cache, "senet50-ferplus.json"))) == {"valAcc": 0.625, "testAcc": 0.375}
    out = capsys.readouterr().out
    assert "evaluating resnet50-ferplus on FER+..." in out and "resnet50-ferplus: val (0.750), test: (0.500)" in out
    assert out.count("-----------------------------------------------------------\n") == 2
    # a second run reuses both caches; a changed cache file is what gets reported
    json.dump({"valAcc": 0.1, "testAcc": 0.2}, open(os.path.join(cache, "resnet50-ferplus.json"), "w"))
    res2 = bm.benchmark_ferplus_models(dataDir="somewhere", benchmarkCacheDir=cache)
    assert len(calls) == 4 and res2["resnet50-ferplus"] == {"valAcc": 0.1, "testAcc": 0.2} and res2["senet50-ferplus"] == res["senet50-ferplus"]
    out = capsys.readouterr().out
    assert out.count("loading cached results for") == 2 and "resnet50-ferplus: val (0.100), test: (0.200)" in out
    # one cache missing: only that model is evaluated
    os.remove(os.path.join(cache, "senet50-ferplus.json"))
    bm.benchmark_ferplus_models(dataDir="somewhere", benchmarkCacheDir=cache, verbose=False)
    assert len(calls) == 6 and {c["modelName"] for c in calls[4:]} == {"senet50-ferplus"}
    assert capsys.readouterr().out == ""
    # refresh: both again, the caches are rewritten
    res3 = bm.benchmark_ferplus_models(refresh=True, dataDir="somewhere", benchmarkCacheDir=cache, verbose=False)
    assert len(calls) == 10 and res3 == res
    assert json.load(open(os.path.join(cache, "resnet50-ferplus.json"))) == {"valAcc": 0.75, "testAcc": 0.5}


def test_default_data_dir_does_not_exist():
    """ferplus_baselines reads the CSVs only where both exist: its default dataDir does not, so every caller that names no
    dataDir keeps the synthetic imdb"""
    import inspect
    from mcncrossmodalemotions_amd import ferplus_baselines as fb
    default = inspect.signature(fb.ferplus_baselines).parameters["dataDir"].default
    assert not os.path.exists(default)
    assert fb.PRETRAINED == ("resnet50-ferplus", "senet50-ferplus")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_pixcsv_plan_header_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pixcsv_plan_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "pixcsv_plan_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout.strip())
    assert int(r.stdout.split()[0]) > 50000      # every truncation and mutation ran

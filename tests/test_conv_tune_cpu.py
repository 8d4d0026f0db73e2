"""csrc/conv_tune.h -- the tile configurations, the keys of the tuning table, the table and its file format -- needs
neither HIP nor a GPU: tests/conv_tune_check.cpp includes nothing else.  It loads the shipped tune_gfx950.txt, saves it
back byte for byte, feeds the loader files it has to refuse and lines it has to skip, and compares the key builders with
keys recorded in tests/golden/conv_dispatch_digest.json.  Built with the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "mcncrossmodalemotions_amd", "tune_gfx950.txt")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_conv_tune_header_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "conv_tune_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "conv_tune_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    with open(TABLE, "rb") as fh:
        before = fh.read()
    work = tmp_path / "work"
    work.mkdir()
    r = subprocess.run([exe, TABLE, str(work)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout.strip())
    words = r.stdout.split()
    assert int(words[0]) > 1000                                   # every section ran (two checks per shipped entry)
    assert int(words[2]) == before.count(b"\n") - 1               # one entry per line after the header
    with open(TABLE, "rb") as fh:
        assert fh.read() == before                                # the check writes to its scratch directory only
    assert sorted(os.listdir(work)) == ["case.txt", "copy.txt"]   # no .tmp file left behind

"""Pins what csrc/conv.hip's dispatch DOES, arm by arm, against a record taken before the dispatch code was reorganised
(tests/golden/conv_dispatch_digest.json; worker: tests/_dispatch_worker.py, one child process per pass because the
autotune switch is read once per process).

Pass 1 (XM_AUTOTUNE=0, no table): the tile configuration is the analytic model's or a forced one and a challenger runs
only when its force hook asks for it, so every launch is a function of the shape alone.  Per case: the kernels the
profiler hooks saw and the SHA-256 of every output tensor, both equal to the record (the reductions have a fixed order).
Pass 2 (find mode on, empty table, no force hook): one launch per tune kind just above its policy threshold; the KEYS
xm_tune_save writes (first nine integers of a line) equal the record -- they are the keys of the shipped
tune_gfx950.txt.  The chosen configuration is a measurement and is ignored.
"""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_dispatch_worker.py")
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_dispatch_digest.json")

# every ProfKind (csrc/prof.h) that csrc/conv.hip records has to occur in the record (and therefore in every later run)
KERNELS = ["conv_gemm_kernel<", "conv_gemm_dma_kernel<", "conv_gemm_multi_kernel<", "conv_wgrad_kernel<", "conv_halo_kernel<2, 2, 2, 2, 512>",
           "conv_halo_kernel<3, 1, 1, 4, 512>", "conv_halo_kernel<3, 1, 1, 4, 1024>", "conv_halo_multi_kernel<", "conv_stem_kernel<",
           "conv_stem_wgrad_kernel<", "conv_stem_wgrad_bnp_kernel<", "conv_wgrad_patch_kernel<", "conv_wgrad_patch_s2_kernel<",
           "conv_dgrad_s2_kernel<", "conv_stem3_kernel<", "stem_gram_kernel<", "conv_stem_wgrad_pool_kernel<2, true>",
           "conv_stem_wgrad_pool_kernel<2, false>", "conv_stem_bnpool_fwd_kernel"]
TUNE_KINDS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12]


def _run(tmp_path, what, env_extra):
    out = str(tmp_path / (what + ".json"))
    env = {k: v for k, v in os.environ.items() if not k.startswith("XM_") or k == "XM_LIB_PATH"}
    env["XM_TUNE_FILE"] = ""
    env.update(env_extra)
    t0 = time.time()
    r = subprocess.run([sys.executable, WORKER, what, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, "%s: %s" % (what, r.stderr.decode()[-3000:])
    print("%s pass: %.1f s" % (what, time.time() - t0))
    return json.load(open(out))


def test_golden_covers_every_kernel_family_and_tune_kind():
    gold = json.load(open(GOLDEN))
    seen = [k for c in gold["results"].values() for k in c["kernels"]]
    for prefix in KERNELS:
        assert any(k.startswith(prefix) for k in seen), prefix
    assert sorted({k[0] for k in gold["keys"]}) == TUNE_KINDS
    ci = {int(n[len("fwd_1x1_cfg"):]): c["kernels"] for n, c in gold["results"].items() if n.startswith("fwd_1x1_cfg")}
    assert len(ci) == 12 and all(("dma" in ci[i][0]) == (i >= 8) for i in ci), ci
    assert not any("dma" in k for n, c in gold["results"].items() if n.startswith("fwd_1x1_odd") for k in c["kernels"])


@pytest.mark.gpu
def test_every_dispatch_arm_runs_the_recorded_kernels_and_gives_the_recorded_bits(gpu, tmp_path):
    gold = json.load(open(GOLDEN))["results"]
    got = _run(tmp_path, "results", {"XM_AUTOTUNE": "0"})
    assert sorted(got) == sorted(gold)
    for name in sorted(gold):
        assert got[name]["kernels"] == gold[name]["kernels"], name
        assert got[name]["sha256"] == gold[name]["sha256"], name


@pytest.mark.gpu
def test_tune_table_keys_are_the_recorded_ones(gpu, tmp_path):
    gold = json.load(open(GOLDEN))["keys"]
    got = _run(tmp_path, "keys", {})
    assert got == gold, ([k for k in got if k not in gold], [k for k in gold if k not in got])

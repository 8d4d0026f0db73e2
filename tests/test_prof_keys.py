"""CPU (xm_prof_kernel_name needs no device): the profiler's key table (csrc/prof.cpp, conv_cfg_kernel_name in
csrc/conv.hip) decodes every key a launch site can record to the recorded name, a kernel the library holds, and refuses
every other key.  tests/golden/prof_kernel_names.json was written by `python tests/test_prof_keys.py` from the library of
the commit before the key table existed; run that again only when a kernel is renamed on purpose."""
import ctypes as C
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "prof_kernel_names.json")
XM_EINVAL = 1

# kind -> the sub-keys its launch sites produce (key = kind * 100 + sub)
SUBS = {
    0: [ci * 2 + mode for ci in range(12) for mode in (0, 1)],   # gemm
    1: [ci * 4 + v for ci in range(7) for v in (0, 1, 2)],       # wgrad
    2: [ci * 2 for ci in range(8)],                              # gemm-multi
    3: [0, 1, 2], 4: [0, 1, 2],                                  # halo, halo-multi
    5: [0], 6: [0, 1],                                           # stem, stem-wgrad
    9: [0], 10: [0], 11: [0],                                    # wgrad-patch, wgrad-patch-s2, dgrad-s2
    12: [0, 1], 13: [0], 14: [0, 1], 15: [0],                    # stem3, stem-gram, stem-wgrad-pool, stem-bnpool-fwd
    20: [0, 1, 2, 3], 21: [0, 1, 2, 3, 4, 5], 22: [0], 23: [0],  # spec, jpeg, wav, pixcsv
}
VALID = sorted(kind * 100 + s for kind, subs in SUBS.items() for s in subs)


def _name(L, key):
    buf = C.create_string_buffer(b"?" * 127, 128)
    return L.xm_prof_kernel_name(key, buf, 128), buf.value.decode()


def _golden():
    return {int(k): v for k, v in json.load(open(GOLDEN)).items()}


def test_launch_site_keys_give_the_recorded_names_and_every_other_key_is_refused():
    from mcncrossmodalemotions_amd import _lib
    L = _lib.load()
    gold = _golden()
    assert sorted(gold) == VALID and len(VALID) == 83 and len(set(gold.values())) == 79
    want = {k: (0, gold[k]) if k in gold else (XM_EINVAL, "") for k in range(2500)}
    wrong = {k: (_name(L, k), want[k]) for k in want if _name(L, k) != want[k]}
    assert not wrong, wrong


def test_names_are_kernels_of_the_library():
    from mcncrossmodalemotions_amd import _lib, build
    build.build()
    syms = subprocess.run(["nm", "-C", _lib.SO_PATH], check=True, capture_output=True, text=True).stdout
    missing = [n for n in sorted(set(_golden().values()))
               if "xm::%s(" % n not in syms and ("<" in n or "xm::%s<" % n not in syms)]
    assert not missing, missing


def test_no_numeric_kind_and_no_open_close_pair_is_left():
    csrc = os.path.join(ROOT, "mcncrossmodalemotions_amd", "csrc")
    for fn in sorted(os.listdir(csrc)):
        if os.path.isfile(os.path.join(csrc, fn)):
            txt = open(os.path.join(csrc, fn)).read()
            assert "prof_open" not in txt and "prof_close" not in txt, fn
            assert not re.search(r"ProfScope\s+\w+\s*[({]\s*\d", txt), fn


if __name__ == "__main__":   # regenerate the golden file from the library as built
    from mcncrossmodalemotions_amd import _lib
    names = {}
    for key in VALID:
        rc, names[str(key)] = _name(_lib.load(), key)
        assert rc == 0, key
    json.dump(names, open(GOLDEN, "w"), indent=0)

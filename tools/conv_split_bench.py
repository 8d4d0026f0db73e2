#!/usr/bin/env python
"""The bf16x3 arm of the frozen teachers' 1 x 1 layers (vl_nnconv precision='bf16x3', conv_split.hip) against the fp32
selection, in ONE process and one call.
usage: python tools/conv_split_bench.py [--faces 32 128] [--rounds 9] [--reps 5] [--teacher-reps 4] [--json FILE]
Prints
 (a) every distinct 1 x 1 layer call of resnet50-ferplus and senet50-ferplus at each face count, as the forward-only
     test-mode plan issues it (stride-2 stage openings, pruned stage ends with their strided shortcut, SE projections with
     their gate included): microseconds of the fp32 selection and of the split kernel -- medians of interleaved rounds, the
     same operands, each round a burst of `reps` calls between two events -- their ratio, and whether the split kernel
     clears the 4 % margin (the call-to-call spread of one kernel; XM_HALO_MARGIN's figure for a challenger);
 (b) whole-teacher img/s through zoo.FrozenTeacher at fp32, at bf16x3 under the shipped `want` rule, and at bf16x3 with
     every layer the kernel can run ("all": the test switch conv_split_want = 1), interleaved;
 (c) the drift of the logits at bf16x3 (rule / all) from the fp32 logits on the same faces, as a fraction of the largest
     fp32 logit (seeded synthetic weights and random faces: the fixture-based figures are those of
     tests/test_gpu_teacher_precision.py).
The last line is one JSON record of all of it."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mcncrossmodalemotions_amd import _lib, dagnn, vl, zoo  # noqa: E402

TEACHERS = ("resnet50-ferplus", "senet50-ferplus")
MARGIN = 1.04


def teacher_net(name, precision="fp32"):
    net = zoo.ferPlusZoo(name)
    zoo.strip_losses(net)
    net.mode = "test"
    net.move("gpu")
    net.convPrecision = precision
    return net


def burst(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3      # microseconds per call


def interleaved(fns, rounds, reps):
    """median microseconds per call of each of `fns`, measured round-robin"""
    for fn in fns:
        fn()
        fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            t[i].append(burst(fn, reps))
    return [statistics.median(x) for x in t]


def record_calls(name, faces):
    """the forward vl_nnconv calls of the teacher's forward-only plan that the split kernel can run: distinct
    (shapes, stride, epilogue) -> [count, a layer name]"""
    L = _lib.load()
    net = teacher_net(name, "bf16x3")
    L.xm_debug_set(b"conv_split_want", 0)          # every call stays fp32 but passes through the plan's one helper
    seen = {}
    real = dagnn._forward_conv

    def spy(step, x, f, b, **kw):
        g = vl.conv_split_geometry(x.shape, f.shape, stride=kw.get("stride", 1), pad=kw.get("pad", 0),
                                   relu=bool(kw.get("relu")), sigmoid=bool(kw.get("sigmoid")))
        if g["can"] and kw.get("out_lattice") is None:
            res = kw.get("residual")
            key = (tuple(int(v) for v in x.shape), tuple(int(v) for v in f.shape), tuple(vl._pair(kw.get("stride", 1), "S")),
                   b is not None, kw.get("scale") is not None, kw.get("gate") is not None,
                   None if res is None else tuple(int(v) for v in res.shape),
                   None if kw.get("residual_stride") is None else tuple(kw["residual_stride"]), bool(kw.get("relu")))
            seen.setdefault(key, [0, step.rec.name, g["want"]])[0] += 1
        return real(step, x, f, b, **kw)

    dagnn._forward_conv = spy
    try:
        x = vl.from_numpy(np.asfortranarray(np.random.default_rng(0).standard_normal((224, 224, 3, faces)).astype(np.float32)))
        net.eval(["data", x])
        torch.cuda.synchronize()
    finally:
        dagnn._forward_conv = real
        L.xm_debug_set(b"conv_split_want", -1)
    # `want` under the shipped rule, asked again with the switch back at its default
    for key, v in seen.items():
        v[2] = vl.conv_split_geometry(key[0], key[1], stride=key[2], relu=key[8])["want"]
    return seen


def layer_table(faces, rounds, reps):
    rows, done = [], {}
    rng = np.random.default_rng(1)
    dev = lambda *s: vl.from_numpy(np.asfortranarray(rng.standard_normal(s).astype(np.float32)))
    for name in TEACHERS:
        for key, (count, layer, want) in record_calls(name, faces).items():
            xs, fs, stride, has_b, has_s, has_g, rs, rstride, relu = key
            if key not in done:
                K, N = fs[3], xs[3]
                kw = dict(stride=stride, relu=relu, residual_stride=rstride)
                if has_s:
                    kw["scale"], kw["shift"] = dev(K, 1), dev(K, 1)
                if has_g:
                    kw["gate"] = vl.from_numpy(np.asfortranarray(rng.uniform(0, 1, (1, 1, K, N)).astype(np.float32)))
                if rs is not None:
                    kw["residual"] = dev(*rs)
                x, f, b = dev(*xs), dev(*fs), (dev(K, 1) if has_b else None)
                t32, t3 = interleaved([lambda: vl.vl_nnconv(x, f, b, **kw),
                                       lambda: vl.vl_nnconv(x, f, b, precision="bf16x3", **kw)], rounds, reps)
                done[key] = (t32, t3)
            t32, t3 = done[key]
            Ho, Wo = (xs[0] - 1) // stride[0] + 1, (xs[1] - 1) // stride[1] + 1
            rows.append(dict(teacher=name, faces=faces, layer=layer, count=count, H=xs[0], W=xs[1], C=xs[2], K=fs[3],
                             stride=list(stride), gate=has_g, residual=rs is not None, residual_stride=list(rstride) if rstride else None,
                             relu=relu, fp32_us=round(t32, 2), split_us=round(t3, 2), ratio=round(t32 / t3, 3),
                             clears=bool(t3 * MARGIN < t32), want=bool(want),
                             split_tflops=round(2.0 * Ho * Wo * xs[3] * xs[2] * fs[3] / t3 * 1e-6, 1)))
    return rows


def teacher_table(faces, rounds, reps):
    L = _lib.load()
    out = []
    for name in TEACHERS:
        x = vl.from_numpy(np.asfortranarray(np.random.default_rng(2).standard_normal((224, 224, 3, faces)).astype(np.float32)))
        teachers = {"fp32": zoo.FrozenTeacher(teacher_net(name), lanes=2, precision="fp32"),
                    "bf16x3": zoo.FrozenTeacher(teacher_net(name), lanes=2, precision="bf16x3"),
                    "bf16x3-all": zoo.FrozenTeacher(teacher_net(name), lanes=2, precision="bf16x3")}

        def run(tag):
            # the plan of a lane asks the library per shape on its first run and keeps the answer: "all" keeps the switch on
            # for its own calls only
            L.xm_debug_set(b"conv_split_want", 1 if tag == "bf16x3-all" else -1)
            try:
                return teachers[tag].logits(x)
            finally:
                L.xm_debug_set(b"conv_split_want", -1)

        tags = list(teachers)
        logits = {t: vl.to_numpy(run(t)).astype(np.float64) for t in tags}
        us = interleaved([lambda t=t: run(t) for t in tags], rounds, reps)
        big = float(np.abs(logits["fp32"]).max())
        rec = dict(teacher=name, faces=faces)
        for t, u in zip(tags, us):
            rec[t + "_img_s"] = round(faces / u * 1e6, 1)
            if t != "fp32":
                rec[t + "_drift"] = float(np.abs(logits[t] - logits["fp32"]).max() / big)
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--teacher-reps", type=int, default=4)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    layers, nets = [], []
    for faces in a.faces:
        layers += layer_table(faces, a.rounds, a.reps)
        nets += teacher_table(faces, a.rounds, a.teacher_reps)
    print("%-17s %5s %-18s %2s %4s %5s %5s %-6s %-10s %9s %9s %6s %7s %s" % (
        "teacher", "faces", "layer", "x", "HxW", "C", "K", "stride", "epilogue", "fp32 us", "split us", "ratio", "TFLOP/s", "clears/want"))
    for r in layers:
        epi = ("g" if r["gate"] else "") + ("r" if r["residual"] else "") + ("s" if r["residual_stride"] else "") + ("R" if r["relu"] else "")
        print("%-17s %5d %-18s %2d %4s %5d %5d %-6s %-10s %9.1f %9.1f %6.2f %7.1f %s/%s" % (
            r["teacher"], r["faces"], r["layer"], r["count"], "%dx%d" % (r["H"], r["W"]), r["C"], r["K"],
            "%dx%d" % tuple(r["stride"]), epi or "-", r["fp32_us"], r["split_us"], r["ratio"], r["split_tflops"],
            "yes" if r["clears"] else "no", "yes" if r["want"] else "no"))
    for r in nets:
        print("%-17s %4d faces: fp32 %8.1f img/s   bf16x3 (rule) %8.1f img/s, drift %.2e   bf16x3 (all) %8.1f img/s, drift %.2e" % (
            r["teacher"], r["faces"], r["fp32_img_s"], r["bf16x3_img_s"], r["bf16x3_drift"], r["bf16x3-all_img_s"],
            r["bf16x3-all_drift"]))
    rec = json.dumps(dict(layers=layers, teachers=nets))
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(rec + "\n")
    print(rec)


if __name__ == "__main__":
    main()

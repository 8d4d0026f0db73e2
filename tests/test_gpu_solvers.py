"""GPU: xm_solver_update (csrc/misc.hip solver_kernel) and its way up through vl.solver_update, train.accumulate_gradients,
cnn_train_dag's checkpoints and the two training drivers, against the numpy restatement of tests/test_solvers.py.

Allowance per output tensor (tests/test_solvers.py has the reasoning): |got - ref64| <= max(4 * max|ref32 - ref64|, one fp32
ulp of max|ref64|), after max|ref32 - ref64| <= 2.5e-7 has been asserted.  Every check prints both figures.

Launch arithmetic (ew_grid(items) = min(ceil(items / 256), 2048) blocks of 256; float4 arm when every non-NULL pointer is
16-byte aligned, scalar arm otherwise):
  n = 1, 3            the float4 arm with no quad: the scalar tail alone
  n = 4, 5            one quad, without / with a tail
  n = 255, 256, 257   the block edge in the tail / scalar arithmetic; n = 4,099: 1,024 quads = 4 full blocks + a 3-element tail
  n = 2,100,003       n / 4 = 525,000 quads > 2,048 * 256 = 524,288: blocks 0 .. 2 take a second grid-stride trip; tail of 3;
                      with ONE of w, s1, s2, der one float past a 16-byte boundary the scalar arm: grid 2,048, five trips"""
import numpy as np
import pytest

from test_gpu_misc_edges import guarded, guards_intact
from test_solvers import BATCH, KINDS, LR, TWO_STATE, WD, allowance, case, restate

pytestmark = pytest.mark.gpu

BIG_N = 2100003
SIZES = [1, 3, 4, 5, 255, 256, 257, 4099, BIG_N]


def check(what, got, ref32, ref64):
    tol, d = allowance(ref32, ref64, what)
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    print("%s: max|ref32 - ref64| %.3e, max|got - ref64| %.3e (allowed %.3e)" % (what, d, err, tol))
    assert err <= tol, "%s: max|got - ref64| %.3e > %.3e" % (what, err, tol)


def run_one_update(kind, n, warm, off, pass_s2=True):
    """one vl.solver_update on views of guarded buffers at the float offsets `off` (4: aligned, 1: one float off)"""
    from mcncrossmodalemotions_amd import vl
    (w, s1, s2, der), r32, r64 = case(kind, n, warm)
    two = kind in TWO_STATE
    fw, vw = guarded(w, off["w"])
    f1, v1 = guarded(s1, off["s1"])
    f2, v2 = guarded(s2, off["s2"])
    fd, vd = guarded(der, off["der"])
    vl.solver_update(kind, vw, v1, v2 if (two or pass_s2) else None, vd, LR, WD, BATCH)
    tag = "%s n=%d %s" % (kind, n, "warm" if warm else "cold")
    check(tag + " w", vw.cpu().numpy(), r32[0], r64[0])
    check(tag + " s1", v1.cpu().numpy(), r32[1], r64[1])
    if two:
        check(tag + " s2", v2.cpu().numpy(), r32[2], r64[2])
    else:
        assert np.array_equal(v2.cpu().numpy(), s2), tag + ": a one-state kind wrote s2"
    assert np.array_equal(vd.cpu().numpy(), der), tag + ": der changed"
    for f, k in ((fw, "w"), (f1, "s1"), (f2, "s2"), (fd, "der")):
        assert guards_intact(f, off[k], n), tag + ": wrote outside " + k


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("warm", [True, False], ids=["warm", "cold"])
@pytest.mark.parametrize("kind", KINDS)
def test_one_update_every_kind_and_size(gpu, kind, warm, n):
    """float4 arm at every size of the module docstring, warm states and the first step from zero states; der unchanged,
    the floats on both sides of every view unchanged; adagrad / rmsprop / nesterov leave a passed s2 untouched (warm) and
    accept None there (cold)"""
    run_one_update(kind, n, warm, {k: 4 for k in ("w", "s1", "s2", "der")}, pass_s2=warm)


@pytest.mark.parametrize("which", ["w", "s1", "s2", "der"])
@pytest.mark.parametrize("kind", KINDS)
def test_scalar_arm_when_one_operand_is_misaligned(gpu, kind, which):
    """n = 2,100,003 with one of the four operands one float past a 16-byte boundary, one at a time (for a one-state kind
    the misaligned s2 is passed too and stays untouched)"""
    off = {k: (1 if k == which else 4) for k in ("w", "s1", "s2", "der")}
    run_one_update(kind, BIG_N, True, off)


def test_adam_first_step_keeps_matlabs_coefficient_bits(gpu):
    """zero states, der = batch, w = 0: g = 1 exactly, so v = (1 - beta2) and m = (1 - beta1) as MATLAB rounds those double
    expressions -- float32(0.001), not 1 - float32(0.999) -- bit for bit"""
    import torch
    from mcncrossmodalemotions_amd import vl
    n = 1030
    w, m, v = (torch.zeros(n, dtype=torch.float32, device="cuda") for _ in range(3))
    der = torch.full((n,), BATCH, dtype=torch.float32, device="cuda")
    vl.solver_update("adam", w, m, v, der, LR, WD, BATCH)
    vv, mm = v.cpu().numpy(), m.cpu().numpy()
    assert (vv == np.float32(1.0 - 0.999)).all() and (vv != np.float32(1) - np.float32(0.999)).all()
    assert (mm == np.float32(1.0 - 0.9)).all()
    # lr_t * m / (sqrt(v) + epsilon) with t = 1 is lr * 1 / (1 + epsilon / sqrt(1 - beta2)): one step of lr
    assert np.abs(w.cpu().numpy() + LR).max() <= 1e-7


@pytest.mark.parametrize("kind", KINDS)
def test_twenty_consecutive_updates(gpu, kind):
    """n = 4,099, zero states, a fresh der per step (the sign of the float64 trajectory's current w, every 7th element --
    shifted by the step -- zero); adam's t counts 1 .. 20.  The allowance comes from the two restatements' trajectories.
    Twenty steps accumulate twenty steps' roundings, so the inputs are taken from the inner part of the one-step ranges,
    where an ulp is smaller: w0 in (-0.45, 0.45), |der| / batch in (0.05, 0.25) (adagrad's g_sqr, a plain sum of g.^2, stays
    below 1.25 and nesterov's momentum below 2.5; with |der| / batch up to 0.95 they reach 9.3 and 2.6 and the fp32
    restatement alone is 1.6e-6 and 3e-7 away from the fp64 one).  max|ref32 - ref64| over (w, s1[, s2]) with these inputs,
    on the CPU: adagrad 1.3e-7, rmsprop 2.1e-7, adadelta 1.2e-7, adam 1.1e-7, nesterov 2.3e-7 -- inside the 2.5e-7 that
    `allowance` asserts first"""
    import torch
    from mcncrossmodalemotions_amd import vl
    n, steps = 4099, 20
    rng = np.random.default_rng(20 + KINDS.index(kind))
    w0 = rng.uniform(-0.45, 0.45, n).astype(np.float32)
    two = kind in TWO_STATE
    z = np.zeros(n, np.float32)
    s64, s32 = (w0, z, z if two else None), (w0, z, z if two else None)
    dw, d1, d2 = (torch.from_numpy(a.copy()).cuda() for a in (w0, z, z))
    for t in range(1, steps + 1):
        der = (np.where(s64[0] < 0, -1.0, 1.0) * BATCH * rng.uniform(0.05, 0.25, n)).astype(np.float32)
        der[t % 7::7] = 0.0
        s64 = restate(kind, s64[0], s64[1], s64[2], der, LR, WD, BATCH, np.float64, t=t)
        s32 = restate(kind, s32[0], s32[1], s32[2], der, LR, WD, BATCH, np.float32, t=t)
        vl.solver_update(kind, dw, d1, d2 if two else None, torch.from_numpy(der).cuda(), LR, WD, BATCH, t=t)
    check(kind + " 20 steps w", dw.cpu().numpy(), s32[0], s64[0])
    check(kind + " 20 steps s1", d1.cpu().numpy(), s32[1], s64[1])
    if two:
        check(kind + " 20 steps s2", d2.cpu().numpy(), s32[2], s64[2])
    else:
        assert not d2.any().item()


# ---- train_step on the narrow student ----------------------------------------------------------------------------------------
STUDENT_LR = 1e-2
# The derivatives of a real network put no distance between g = der / batch + wd * w and zero, and w - lr * g / (|g| + e) has the
# slope lr * e / (|g| + e)^2 there: with the default epsilon (1e-10 for adagrad) a rounding of g near zero, ~3e-12, is amplified by
# up to lr / e = 1e8 and the restatements part -- on the CPU oracle's derivatives of this very step max|ref32 - ref64| is 9e-6
# (adagrad) and 1.3e-6 (rmsprop), and the conditioning assert would (rightly) fire.  With epsilon = 1e-3 the slope is at most
# lr / e = 10 (for adam the effective e is epsilon / sqrt(1 - beta2) on the first step, larger still) and the same figure is
# 6e-8 .. 7e-8 for every kind: one rounding of w.  adadelta's step is smooth at g = 0 with its default.
STUDENT_SOLVERS = [("adagrad", {"epsilon": 1e-3}), ("rmsprop", {"epsilon": 1e-3}), ("adadelta", {}),
                   ("adam", {"epsilon": 1e-3}), (None, {})]
FROZEN = "conv2b"       # given zero multipliers below: a segment of its own that every solver must skip


def _student(seed=11):
    from mcncrossmodalemotions_amd import zoo
    net = zoo.emoVoxZoo(numSeconds=1, seed=seed, width_mult=0.125)
    name = FROZEN if FROZEN in net.params else sorted(net.params)[0]
    net.params[name].learningRate = 0
    net.params[name].weightDecay = 0
    net.pack_params()
    return net, name


def _pairs(seed=5, N=4):
    from mcncrossmodalemotions_amd import vl
    from test_gpu_nets import _student_inputs
    data, lgo, lab = _student_inputs(np.random.default_rng(seed), 100, N)
    return ["data", vl.from_numpy(data), "logitTarget", vl.from_numpy(lgo), "maxLabel", vl.from_numpy(lab)]


@pytest.fixture(scope="module")
def sgd_step(gpu):
    """the default solver's step on the same net and inputs: flat values before, flat derivative, flat values after"""
    import torch
    from mcncrossmodalemotions_amd import train
    net, _ = _student()
    inputs = _pairs()
    val0 = net._flat.val.cpu().numpy().copy()
    net.mode = "normal"
    net.eval(inputs, ["objective", 1])
    der0 = net._flat.der.cpu().numpy().copy()
    train.train_step(net, inputs, train.TrainOpts(learningRate=[STUDENT_LR], batchSize=4), 0, None, 4)
    torch.cuda.synchronize()
    assert np.array_equal(net._flat.der.cpu().numpy(), der0), "the step's derivative is not that of the prior eval"
    return val0, der0, net._flat.val.cpu().numpy().copy()


@pytest.mark.parametrize("solver,sopts", STUDENT_SOLVERS, ids=[s or "nesterovUpdate" for s, _ in STUDENT_SOLVERS])
def test_train_step_applies_the_solver_per_segment(gpu, sgd_step, solver, sopts):
    """one train_step (width_mult 0.125, numSeconds 1, N = 4) from zero states: every 'gradient' segment equals the
    restatement with the segment's multipliers on the derivative of a prior net.eval of the same inputs; 'average' segments
    (the BN moments) equal the default solver's run; the segment with zero multipliers keeps values and state, and adam's t
    does not advance there; paramGeneration advances"""
    import torch
    from mcncrossmodalemotions_amd import train
    val0, der0, val_sgd = sgd_step
    net, frozen = _student()
    flat = net._flat
    assert np.array_equal(flat.val.cpu().numpy(), val0)
    opts = train.TrainOpts(learningRate=[STUDENT_LR], batchSize=4, solver=solver, solverOpts=sopts or None,
                           nesterovUpdate=solver is None)
    gen = net.paramGeneration
    train.train_step(net, _pairs(), opts, 0, None, 4)
    torch.cuda.synchronize()
    assert net.paramGeneration > gen
    assert np.array_equal(flat.der.cpu().numpy(), der0)
    val, s1 = flat.val.cpu().numpy(), flat.mom.cpu().numpy()
    kind = solver or "nesterov"
    two = kind in TWO_STATE
    assert (flat.state2 is not None) == two
    s2 = flat.state2.cpu().numpy() if two else None
    seen = set()
    for k, ((method, lr_mult, wd_mult), a, b) in enumerate(flat.segments):
        if b == a:
            continue
        seen.add((method, lr_mult > 0 or wd_mult > 0))
        tag = "%s segment %d (%s, lr x %g, wd x %g)" % (kind, k, method, lr_mult, wd_mult)
        if method == "average":
            assert np.array_equal(val[a:b], val_sgd[a:b]), tag
            assert not s1[a:b].any() and (s2 is None or not s2[a:b].any()), tag + ": state written"
            continue
        if not (lr_mult > 0 or wd_mult > 0):
            assert np.array_equal(val[a:b], val0[a:b]) and not s1[a:b].any(), tag + ": not skipped"
            assert s2 is None or not s2[a:b].any(), tag
            assert solver is None or flat.solver_t[k] == 0, tag
            continue
        z = np.zeros(b - a, np.float32)
        ko = {"momentum": opts.momentum} if solver is None else sopts
        args = (kind, val0[a:b], z, z if two else None, der0[a:b], STUDENT_LR * lr_mult, opts.weightDecay * wd_mult, 4.0)
        r64, r32 = restate(*args, np.float64, t=1, **ko), restate(*args, np.float32, t=1, **ko)
        check(tag + " w", val[a:b], r32[0], r64[0])
        check(tag + " s1", s1[a:b], r32[1], r64[1])
        if two:
            check(tag + " s2", s2[a:b], r32[2], r64[2])
        if solver == "adam":
            assert flat.solver_t[k] == 1, tag
    assert seen == {("average", True), ("gradient", True), ("gradient", False)}, seen
    off = net.params[frozen]._flat_off
    assert np.array_equal(val[off:off + 4], val0[off:off + 4])


# ---- cnn_train_dag: checkpoints -------------------------------------------------------------------------------------------------
class _TinyImdb:
    """eight fixed (spectrogram, teacher logits) pairs; samples 0 .. 5 train, 6 .. 7 validate"""

    def __init__(self):
        from test_gpu_nets import _student_inputs
        self.data, self.lgo, self.lab = _student_inputs(np.random.default_rng(31), 100, 8)

    def getBatch(self, imdb, batch):
        from mcncrossmodalemotions_amd import vl
        b = list(batch)
        return ["data", vl.from_numpy(np.ascontiguousarray(self.data[..., b])),
                "logitTarget", vl.from_numpy(np.ascontiguousarray(self.lgo[..., b])),
                "maxLabel", vl.from_numpy(np.ascontiguousarray(self.lab[..., b]))]


def _train(imdb, expDir, numEpochs, **kw):
    from mcncrossmodalemotions_amd import train, zoo
    net = zoo.emoVoxZoo(numSeconds=1, seed=3, width_mult=0.125)
    return train.cnn_train_dag(net, imdb, imdb.getBatch, learningRate=[1e-3, 5e-4], batchSize=4, numEpochs=numEpochs,
                               train=range(6), val=[6, 7], expDir=str(expDir), **kw)


def test_adam_resumes_bit_for_bit_and_checkpoints_name_their_solver(gpu, tmp_path):
    """two epochs in one run == one epoch + a resumed second epoch: flat values, both states and t bit-identical (six samples
    in batches of four: the ragged second batch runs too).  The checkpoint of an adam run does not resume under the default
    solver (CheckpointMismatch naming both, nothing copied); a default-solver checkpoint has no "solver" key and resumes under
    the default solver as before, and not under adam"""
    import torch
    from mcncrossmodalemotions_amd import train
    imdb = _TinyImdb()
    adam = dict(solver="adam", solverOpts={"beta2": 0.99})
    a, info_a = _train(imdb, tmp_path / "a", 2, **adam)
    _train(imdb, tmp_path / "b", 1, **adam)
    b, info_b = _train(imdb, tmp_path / "b", 2, **adam)
    assert len(info_b["train"]) == 2 and info_b["train"][0]["objective"] == info_a["train"][0]["objective"]
    assert info_b["train"][1]["objective"] == info_a["train"][1]["objective"]
    for what in ("val", "mom", "state2"):
        assert torch.equal(getattr(a._flat, what), getattr(b._flat, what)), what
    assert a._flat.state2.any().item() and a._flat.mom.any().item()
    assert a._flat.solver_t == b._flat.solver_t and max(a._flat.solver_t) == 4 and min(a._flat.solver_t) == 0
    ck = torch.load(str(tmp_path / "b" / "net-epoch-2.pt"), weights_only=True)
    assert ck["format"] == "xmodal-params-v2" and ck["solver"]["name"] == "adam"
    assert ck["solver"]["opts"] == {"beta1": 0.9, "beta2": 0.99, "epsilon": 1e-8}
    assert set(ck["solver"]["state2"]) == set(ck["momentum"]) == set(a.params)
    assert set(ck["solver"]["t"].values()) <= {0, 4}
    with pytest.raises(train.CheckpointMismatch, match=r"'adam'.*None"):
        _train(imdb, tmp_path / "b", 3)
    _train(imdb, tmp_path / "c", 1)
    ck = torch.load(str(tmp_path / "c" / "net-epoch-1.pt"), weights_only=True)
    assert "solver" not in ck and sorted(ck) == ["epoch", "format", "info", "momentum", "params", "rng"]
    c, info_c = _train(imdb, tmp_path / "c", 2)
    assert len(info_c["train"]) == 2 and c._flat.state2 is None
    with pytest.raises(train.CheckpointMismatch, match=r"None.*'adam'"):
        _train(imdb, tmp_path / "c", 3, **adam)


def test_fifteen_adam_steps_lower_the_objective(gpu):
    import torch
    from mcncrossmodalemotions_amd import train, vl, zoo
    net = zoo.emoVoxZoo(numSeconds=1, seed=11, width_mult=0.125)
    net.pack_params()
    inputs = _pairs(seed=8)
    opts = train.TrainOpts(learningRate=[1e-3], batchSize=4, solver="adam")
    obj = []
    for it in range(15):
        train.train_step(net, inputs, opts, 0, None, 4)
        obj.append(float(vl.to_numpy(net.vars["objective"].value).ravel()[0]))
    torch.cuda.synchronize()
    print("objective over 15 adam steps:", " ".join("%.4f" % o for o in obj))
    assert np.isfinite(obj).all() and obj[-1] < obj[0]
    assert [t for t, (_, a, b) in zip(net._flat.solver_t, net._flat.segments) if b > a and t] and \
        max(net._flat.solver_t) == 15


def test_drivers_pass_the_solver_options_through(gpu, tmp_path):
    """run_distillation and ferplus_baselines in the tiny configurations of tests/test_gpu_nets.py and
    tests/test_gpu_ferplus.py with the new keywords: finite statistics, and checkpoints that name the solver"""
    import os
    import torch
    from mcncrossmodalemotions_amd import batch
    from mcncrossmodalemotions_amd.ferplus_baselines import ferplus_baselines
    from mcncrossmodalemotions_amd.run_distillation import run_distillation
    net, info = run_distillation(gpus=[0], numSeconds=1, batchSize=4, miniEpochRatio=0.5, miniVal=0.5, numTracks=24,
                                 widthMult=0.125, dataDir=str(tmp_path / "rd"), learningRate=[1e-3], numEpochs=1,
                                 solver="adam", solverOpts={"beta1": 0.8}, nesterovUpdate=False, momentum=0.8,
                                 weightDecay=1e-4)
    assert np.isfinite(info["train"][0]["objective"]) and np.isfinite(info["val"][0]["objective"])
    assert net._flat.state2 is not None and max(net._flat.solver_t) == 3          # 9 samples in batches of 4
    exp = os.path.join(str(tmp_path / "rd"), os.listdir(str(tmp_path / "rd"))[0])
    ck = torch.load(os.path.join(exp, "net-epoch-1.pt"), weights_only=True)
    assert ck["solver"]["name"] == "adam" and ck["solver"]["opts"]["beta1"] == 0.8
    imdb = batch.SyntheticFerPlusImdb(num_images=24, seed=1)
    kw = dict(imdb=imdb, widthMult=0.125, blocks=(1, 1, 1, 1), batchSize=8, learningRate=[0.01], numEpochs=1)
    dag, info = ferplus_baselines(expRoot=str(tmp_path / "fb"), solver="rmsprop", solverOpts={"rho": 0.9},
                                  nesterovUpdate=True, momentum=0.8, weightDecay=1e-4, **kw)
    for st in info["train"] + info["val"]:
        assert np.isfinite(st["objective"]) and 0 <= st["classerror"] <= 1
    assert dag._flat.state2 is None and dag._flat.mom.any().item()
    dag, info = ferplus_baselines(expRoot=str(tmp_path / "fn"), nesterovUpdate=True, **kw)
    assert np.isfinite(info["train"][0]["objective"]) and dag._flat.solver_t is None

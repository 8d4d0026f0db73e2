"""CPU: cnn_train_dag's solvers (xm_solver_update, vl.solver_update, train.TrainOpts) as far as they answer without a device:
the symbol, its refusals, the option tables, the coefficient rounding -- and the numpy restatement of MatConvNet's +solver
updates that tests/test_gpu_solvers.py holds the kernel to, checked here for the conditioning the allowance relies on.

The restatement is written from the formulas in include/xmodal.h (MatConvNet's +solver package and the nesterovUpdate arm of
cnn_train_dag's default solver [EXT]), MATLAB's order of operations kept.  It is evaluated twice: in float64 (`ref64`) and in
float32 with every intermediate rounded (`ref32`).  Allowance per output tensor:

    |got - ref64| <= max(4 * max|ref32 - ref64|, one fp32 ulp of max|ref64|)

(the device may contract multiply-adds and rounds the scalar coefficients once where ref32 rounds them twice: roundings move,
their number does not).  max|ref32 - ref64| itself must stay <= 2.5e-7, so that a badly conditioned input fails as such and
cannot widen the allowance."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KINDS = ["adagrad", "rmsprop", "adadelta", "adam", "nesterov"]
TWO_STATE = ("adadelta", "adam")
DEFAULTS = {"adagrad": {"epsilon": 1e-10, "rho": 1.0}, "rmsprop": {"epsilon": 1e-8, "rho": 0.99},
            "adadelta": {"epsilon": 1e-6, "rho": 0.9}, "adam": {"beta1": 0.9, "beta2": 0.999, "epsilon": 1e-8},
            "nesterov": {"momentum": 0.9}}
BATCH, WD, LR = 64.0, 5e-4, 0.05
CONDITION = 2.5e-7


def restate(kind, w, s1, s2, der, lr, wd, batch, T, t=1, **opts):
    """one update in dtype T (np.float64 / np.float32), every intermediate rounded to T; scalars are formed in double (as
    MATLAB forms 1 - opts.beta2 or lr_t) and rounded to T once.  Returns new (w, s1, s2); s2 is passed through (None
    allowed) by the kinds that have one state."""
    o = dict(DEFAULTS[kind], **opts)
    c = T                                            # a double scalar as it meets an array of dtype T
    w, s1, der = w.astype(T), s1.astype(T), der.astype(T)
    s2 = None if s2 is None else s2.astype(T)
    g = der * c(1.0 / batch) + c(wd) * w             # vl_taccum(1 / batchSize, parDer, thisDecay, value)
    if kind == "adagrad":
        s1 = s1 * c(o["rho"]) + g * g
        w = w - c(lr) * g / (np.sqrt(s1) + c(o["epsilon"]))
    elif kind == "rmsprop":
        s1 = s1 * c(o["rho"]) + g * g * c(1.0 - o["rho"])
        w = w - c(lr) * g / (np.sqrt(s1) + c(o["epsilon"]))
    elif kind == "adadelta":
        s1 = s1 * c(o["rho"]) + g * g * c(1.0 - o["rho"])
        delta = -np.sqrt((s2 + c(o["epsilon"])) / (s1 + c(o["epsilon"]))) * g
        s2 = s2 * c(o["rho"]) + delta * delta * c(1.0 - o["rho"])
        w = w + c(lr) * delta
    elif kind == "adam":
        s1 = s1 + c(1.0 - o["beta1"]) * (g - s1)
        s2 = s2 + c(1.0 - o["beta2"]) * (g * g - s2)
        lr_t = lr * np.sqrt(1.0 - o["beta2"] ** t) / (1.0 - o["beta1"] ** t)
        w = w - c(lr_t) * s1 / (np.sqrt(s2) + c(o["epsilon"]))
    else:
        s1 = c(o["momentum"]) * s1 - g
        w = w + c(lr) * (c(o["momentum"]) * s1 - g)
    for a in (w, s1) + (() if s2 is None else (s2,)):
        assert a.dtype == T
    return w, s1, s2


def make_inputs(kind, n, warm, seed=0):
    """the issue's input conditions: w in (-0.95, 0.95); der zero at every 7th element, elsewhere with the sign of w and
    |der| / batch in (0.05, 0.95), so that g = der / batch + wd * w never cancels; warm second-moment states in (0.05, 0.5),
    adam's m in (-0.5, 0.5); nesterov's momentum state against the sign of w (a momentum of descent: mom * m - g does not
    cancel either); cold: all states zero"""
    rng = np.random.default_rng(1000 * KINDS.index(kind) + 7 * seed + int(warm))
    w = rng.uniform(-0.95, 0.95, n).astype(np.float32)
    sign = np.where(w < 0, -1.0, 1.0)
    der = (sign * BATCH * rng.uniform(0.05, 0.95, n)).astype(np.float32)
    der[::7] = 0.0
    s1 = np.zeros(n, np.float32)
    s2 = np.zeros(n, np.float32)
    if warm:
        if kind == "adam":
            s1 = rng.uniform(-0.5, 0.5, n).astype(np.float32)
        elif kind == "nesterov":
            s1 = (-sign * rng.uniform(0.05, 0.5, n)).astype(np.float32)
        else:
            s1 = rng.uniform(0.05, 0.5, n).astype(np.float32)
        s2 = rng.uniform(0.05, 0.5, n).astype(np.float32)
    return w, s1, s2, der


def allowance(ref32, ref64, what):
    """the bound for one output tensor; asserts the conditioning first"""
    d = float(np.abs(ref32.astype(np.float64) - ref64).max())
    assert d <= CONDITION, "%s: badly conditioned input, max|ref32 - ref64| = %.3e" % (what, d)
    return max(4 * d, float(np.spacing(np.float32(np.abs(ref64).max())))), d


@functools.lru_cache(maxsize=8)
def case(kind, n, warm):
    """inputs and both restatements of one update, computed once"""
    w, s1, s2, der = make_inputs(kind, n, warm)
    two = kind in TWO_STATE
    r64 = restate(kind, w, s1, s2 if two else None, der, LR, WD, BATCH, np.float64)
    r32 = restate(kind, w, s1, s2 if two else None, der, LR, WD, BATCH, np.float32)
    return (w, s1, s2, der), r32, r64


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warm", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_is_well_conditioned(kind, warm):
    """on the issue's inputs ref32 stays within 2.5e-7 of ref64 on every output of every kind, the tail length and the
    second grid trip of the GPU cases included (n = 2,100,003)"""
    _, r32, r64 = case(kind, 2100003, warm)
    for name, a, b in zip(("w", "s1", "s2"), r32, r64):
        if a is not None:
            allowance(a, b, "%s %s" % (kind, name))


def test_symbol_is_declared_and_exported():
    from mcncrossmodalemotions_amd import _lib
    txt = open(os.path.join(ROOT, "include", "xmodal.h")).read()
    assert re.search(r"\bint xm_solver_update\(int kind, float \*w, float \*s1, float \*s2, const float \*der, size_t n", txt)
    for k, name in enumerate(["ADAGRAD", "RMSPROP", "ADADELTA", "ADAM", "NESTEROV"]):
        assert re.search(r"XM_SOLVER_%s = %d\b" % (name, k), txt)
    L = _lib.load()
    assert "xm_solver_update" in _lib.SIGNATURES and hasattr(L, "xm_solver_update")
    assert L.xm_version() >= 118


def test_refusals_answer_without_a_device():
    """XM_EINVAL with a message for: NULL w, der, s1; NULL s2 where the kind needs it; batch <= 0; an unknown kind.
    n == 0 is XM_OK.  None of them launches (the test runs without a device; the pointers are never dereferenced)."""
    from mcncrossmodalemotions_amd import _lib, vl
    L = _lib.load()
    coef = (C.c_float * 4)(1e-8, 0.1, 0.001, 0.05)
    p = C.c_void_p(4096)          # a non-NULL address that a refused call never reads

    def call(kind, w=p, s1=p, s2=p, der=p, n=8, batch=64.0):
        return L.xm_solver_update(kind, w, s1, s2, der, n, 0.05, 5e-4, batch, coef, None)
    for name in KINDS:
        kind = vl.SOLVERS[name][0]
        for null in ("w", "s1", "der"):
            assert call(kind, **{null: None}) == 1, (name, null)
            assert b"NULL" in L.xm_last_error() and name.encode() in L.xm_last_error()
        for batch in (0.0, -1.0, float("nan")):
            assert call(kind, batch=batch) == 1 and b"batch" in L.xm_last_error()
        if name in TWO_STATE:
            assert call(kind, s2=None) == 1 and b"s2" in L.xm_last_error()
        assert call(kind, n=0) == 0
        assert call(kind, w=None, s1=None, s2=None, der=None, n=0) == 0
    for kind in (-1, 5, 99):
        assert call(kind) == 1 and b"unknown kind" in L.xm_last_error()
    assert L.xm_solver_update(3, p, p, p, p, 8, 0.05, 5e-4, 64.0, None, None) == 1
    with pytest.raises(_lib.XmError):
        _lib.check(call(7))


def test_option_tables_match_the_issue():
    from mcncrossmodalemotions_amd import vl
    assert sorted(vl.SOLVERS) == sorted(KINDS)
    for k, name in enumerate(KINDS):
        kind, defaults, two = vl.SOLVERS[name]
        assert kind == k and defaults == DEFAULTS[name] and two == (name in TWO_STATE)


def test_unknown_solver_and_option_names_are_refused():
    import torch
    from mcncrossmodalemotions_amd import train, vl
    with pytest.raises(ValueError, match="unknown solver"):
        train.TrainOpts(solver="sgd")
    with pytest.raises(ValueError, match="unknown solver"):
        train.TrainOpts(solver="nesterov")            # an arm of the default solver, not a solver
    with pytest.raises(ValueError, match=r"beta1.*beta2.*epsilon"):
        train.TrainOpts(solver="adam", solverOpts={"rho": 0.9})
    with pytest.raises(ValueError, match="solverOpts without a solver"):
        train.TrainOpts(solverOpts={"rho": 0.9})
    o = train.TrainOpts(solver="adam", solverOpts={"beta2": 0.99})
    assert o.solverOpts == {"beta1": 0.9, "beta2": 0.99, "epsilon": 1e-8} and o.nesterovUpdate is False
    o = train.TrainOpts()
    assert o.solver is None and o.solverOpts == {} and o.nesterovUpdate is False
    z = torch.zeros(4)
    with pytest.raises(ValueError, match="unknown solver"):
        vl.solver_update("lbfgs", z, z, None, z, 0.1, 0.0, 1.0)
    with pytest.raises(ValueError, match=r"no option 'momentum'.*epsilon, rho"):
        vl.solver_update("rmsprop", z, z, None, z, 0.1, 0.0, 1.0, momentum=0.9)
    with pytest.raises(ValueError, match="momentum"):
        vl.solver_update("nesterov", z, z, None, z, 0.1, 0.0, 1.0, rho=0.9)


def test_coefficients_are_rounded_once_from_double():
    """MATLAB evaluates (1 - opts.beta2) in double and then multiplies the single array"""
    from mcncrossmodalemotions_amd import vl
    c = vl.solver_coef("adam", 0.05, t=1)
    assert c.dtype == np.float32 and c.shape == (4,)
    assert c[2] == np.float32(0.001) and c[2] != np.float32(1) - np.float32(0.999)
    assert c[1] == np.float32(1.0 - 0.9) and c[0] == np.float32(1e-8)
    for t in (1, 2, 17, 1000):
        lr_t = 0.05 * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)
        assert vl.solver_coef("adam", 0.05, t=t)[3] == np.float32(lr_t)
    assert list(vl.solver_coef("rmsprop", 0.05)) == [np.float32(1e-8), np.float32(0.99), np.float32(1.0 - 0.99), 0]
    assert vl.solver_coef("rmsprop", 0.05)[2] != np.float32(1) - np.float32(0.99)
    assert list(vl.solver_coef("adadelta", 0.05, rho=0.95))[:3] == [np.float32(1e-6), np.float32(0.95), np.float32(1.0 - 0.95)]
    assert list(vl.solver_coef("adagrad", 0.05))[:2] == [np.float32(1e-10), np.float32(1)]
    assert vl.solver_coef("nesterov", 0.05, momentum=0.8)[0] == np.float32(0.8)
    with pytest.raises(ValueError):
        vl.solver_coef("adam", 0.05, t=0)


def test_drivers_take_the_solver_options():
    import inspect
    from mcncrossmodalemotions_amd import ferplus_baselines, run_distillation, train
    for fn in (run_distillation.run_distillation, ferplus_baselines.ferplus_baselines):
        sig = inspect.signature(fn)
        for name, default in (("solver", None), ("solverOpts", None), ("nesterovUpdate", False), ("momentum", 0.9),
                              ("weightDecay", 5e-4)):
            prm = sig.parameters[name]
            assert prm.kind is inspect.Parameter.KEYWORD_ONLY and prm.default == default, (fn.__name__, name)
    sig = inspect.signature(train.cnn_train_dag)
    assert sig.parameters["solver"].default is None and sig.parameters["nesterovUpdate"].default is False

"""dagnn.DagNN.loadobj / saveobj: MatConvNet DagNN model files (.mat, v5 ... v7) in and out.

The reference starts every entry point from such a file (emoVoxCeleb/emoVoxZoo.m:36-46,199; teacher/ferPlusZoo.m:93-101,
145; misc/ensure_compatibility.m:13-31; teacher/ferplus_baselines.m:124-126).  The layout is the one MatConvNet
v1.0-beta25's DagNN.saveobj writes: a struct with the struct arrays `vars` {name, precious}, `params` {name,
value, learningRate, weightDecay [, trainMethod]} and `layers` {name, type, inputs, outputs, params, block}, and `meta`;
either at the top level of the file or inside a field `net`.

    s   = saveobj(net)            the struct, as nested dicts / numpy arrays that scipy.io.savemat takes
    net = loadobj(s)              s: what scipy.io.loadmat returned (the file or its `net` field) or what saveobj made
    net = load_mat(path)          refuses v7.3 (HDF5) files
    save_mat(net, path, wrap)     temporary file renamed into place; wrap='net' is the checkpoint form

Nothing here touches the device except saveobj's download of parameters that live there.  Parameters come back as
float32 Fortran-order host arrays, the form DagNN.initParams produces; DagNN.move('gpu') uploads them.

A file lists its layers in insertion order, DagNN.layers is the execution order: loadobj sorts (execution_order).  No
name of the file is significant: blocks are recognised by `type`, the fused plans by wiring (dagnn.build_plan).
"""
import os

import numpy as np

from . import dagnn

V73_HEADER = b"MATLAB 7.3 MAT-file"
# the 116 text bytes of a v5 header; savemat puts the time of day there, which would make two saves of one net differ
HEADER_TEXT = b"MATLAB 5.0 MAT-file, dagnn.DagNN.saveobj (mcncrossmodalemotions_amd)"

LOSSES = ("softmaxlog", "classerror")       # vl.vl_nnloss

# type string -> (class, fields of `block` that are read and written)
BLOCKS = {
    "dagnn.Conv": (dagnn.Conv, ("size", "hasBias", "pad", "stride", "dilate")),
    "dagnn.BatchNorm": (dagnn.BatchNorm, ("numChannels", "epsilon")),
    "dagnn.ReLU": (dagnn.ReLU, ("leak",)),
    "dagnn.LRN": (dagnn.LRN, ("param",)),
    "dagnn.Sigmoid": (dagnn.Sigmoid, ()),
    "dagnn.SoftMax": (dagnn.SoftMax, ()),
    "dagnn.Sum": (dagnn.Sum, ()),
    "dagnn.Axpy": (dagnn.Axpy, ()),
    "dagnn.Scale": (dagnn.Scale, ()),
    "dagnn.Pooling": (dagnn.Pooling, ("poolSize", "method", "pad", "stride")),
    "dagnn.GlobalPooling": (dagnn.GlobalPooling, ("method",)),
    "dagnn.DropOut": (dagnn.DropOut, ("rate",)),
    "dagnn.Loss": (dagnn.Loss, ("loss",)),
    "dagnn.VerboseLoss": (dagnn.VerboseLoss, ("loss",)),      # a dagnn.Loss subclass (mcnExtraLayers), same fields
    "dagnn.SoftmaxCELoss": (dagnn.SoftmaxCELoss, ("temperature", "logitTargets")),
    "dagnn.EuclideanLoss": (dagnn.EuclideanLoss, ()),
    "dagnn.HuberLoss": (dagnn.HuberLoss, ("sigma",)),
    "dagnn.ErrorStats": (dagnn.ErrorStats, ("numClasses",)),
}
_TYPE_OF = {cls: t for t, (cls, _) in BLOCKS.items()}


# ---------------------------------------------------------------------------------------------
# what scipy.io.loadmat returns -> plain Python
# ---------------------------------------------------------------------------------------------
def _string(x):
    if isinstance(x, str):
        return x
    a = np.asarray(x)
    if a.dtype == object and a.size == 1:
        return _string(a.ravel()[0])
    if a.size == 0:
        return ""
    if a.dtype.kind not in "US":
        raise ValueError("expected a string, found %s %s" % (a.dtype, a.shape))
    return "".join(str(v) for v in a.ravel(order="F"))      # a column of characters reads as one string each


def _cellstr(x):
    """a cell of strings of any shape (1 x n, n x 1, 0 x 0) or a bare string -> list of str"""
    if x is None:
        return []
    if isinstance(x, str):
        return [x]
    if isinstance(x, (list, tuple)):
        return [_string(v) for v in x]
    a = np.asarray(x)
    if a.size == 0:
        return []
    if a.dtype == object:
        return [_string(v) for v in a.ravel(order="F")]
    return [_string(a)]


def _structs(x):
    """a struct array of any shape (0 x 0 included), a dict or a list of dicts -> list of dicts"""
    if x is None:
        return []
    if isinstance(x, dict):
        return [x]
    if isinstance(x, (list, tuple)):
        return [s for v in x for s in _structs(v)]
    a = np.asarray(x)
    if a.size == 0:
        return []
    if a.dtype.names is None:
        if a.dtype == object:       # a struct without fields comes back as [[None]]; a cell of structs is unwrapped
            return [s for v in a.ravel(order="F") for s in ([{}] if v is None else _structs(v))]
        raise ValueError("expected a struct, found %s %s" % (a.dtype, a.shape))
    return [{f: rec[f] for f in a.dtype.names} for rec in a.ravel(order="F")]


def _struct(x, what):
    s = _structs(x)
    if len(s) != 1:
        raise ValueError("%s: expected one struct, found %d" % (what, len(s)))
    return s[0]


def _numbers(x):
    return [float(v) for v in np.asarray(x, np.float64).ravel(order="F")]


def _number(x, what):
    v = _numbers(x)
    if len(v) != 1:
        raise ValueError("%s: expected a scalar, found %d values" % (what, len(v)))
    return v[0]


def _py_number(v):
    v = float(v)
    return int(v) if v.is_integer() and abs(v) < 2 ** 53 else v


def _to_python(x):
    """meta: structs -> dicts, struct arrays and cells -> lists, char -> str, numeric vectors -> lists of numbers
    (whole-valued ones as int), numeric scalars -> numbers, other numeric arrays -> nested lists"""
    if x is None or isinstance(x, (str, bool, int, float)):
        return x
    if isinstance(x, dict):
        return {k: _to_python(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_to_python(v) for v in x]
    a = np.asarray(x)
    if a.dtype.names is not None:
        recs = [{f: _to_python(r[f]) for f in a.dtype.names} for r in a.ravel(order="F")]
        return recs[0] if a.size == 1 else recs
    if a.dtype == object:
        if a.size == 1 and a.ravel()[0] is None:
            return {}
        return [_to_python(v) for v in a.ravel(order="F")]
    if a.dtype.kind in "US":
        return _string(a)
    if a.size == 0:
        return []
    if a.dtype == bool:
        return bool(a.ravel()[0]) if a.size == 1 else [bool(v) for v in a.ravel(order="F")]
    if a.size == 1:
        return _py_number(a.ravel()[0])
    if a.ndim <= 2 and min(a.shape) == 1:
        return [_py_number(v) for v in a.ravel()]
    return [[_py_number(v) for v in row] for row in a] if a.ndim == 2 else a.astype(np.float64).tolist()


# ---------------------------------------------------------------------------------------------
# plain Python -> what scipy.io.savemat takes
# ---------------------------------------------------------------------------------------------
def _cell(items):
    a = np.empty((1, len(items)) if items else (0, 0), object)
    for i, v in enumerate(items):
        a[0, i] = v
    return a


def _struct_array(recs, fields):
    a = np.empty((1, len(recs)) if recs else (0, 0), dtype=[(f, object) for f in fields])
    for i, r in enumerate(recs):
        a[0, i] = tuple(r[f] for f in fields)
    return a


def _row(v):
    return np.asarray(list(v), np.float64).reshape(1, -1)


def _from_python(x):
    if isinstance(x, dict):
        return {k: _from_python(v) for k, v in x.items()}
    if isinstance(x, str):
        return x
    if isinstance(x, (bool, np.bool_)):
        return bool(x)
    if isinstance(x, (int, float, np.integer, np.floating)):
        return float(x)
    if isinstance(x, np.ndarray):
        return x.astype(np.float64) if x.dtype.kind in "iub" else x
    if isinstance(x, (list, tuple)):
        if len(x) == 0:
            return np.zeros((0, 0))
        if all(isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) for v in x):
            return _row(x)
        if all(isinstance(v, dict) for v in x) and all(list(v) == list(x[0]) for v in x):
            return _struct_array([{k: _from_python(w) for k, w in v.items()} for v in x], list(x[0]))
        if all(isinstance(v, (list, tuple)) and len(v) == len(x[0]) and
               all(isinstance(w, (int, float)) for w in v) for v in x):
            return np.asarray(x, np.float64)
        return _cell([_from_python(v) for v in x])
    if x is None:
        return np.zeros((0, 0))
    raise TypeError("meta: cannot write a %s to a model file" % type(x).__name__)


# ---------------------------------------------------------------------------------------------
# blocks
# ---------------------------------------------------------------------------------------------
def _ints(x):
    return [int(round(v)) for v in _numbers(x)]


def _make_block(lname, ltype, b, nparams):
    """the block of layer `lname` from the struct `b` of its public properties; every field not listed in BLOCKS is
    ignored (opts, useShortCircuit, numInputs, exBackprop, average, numAveraged, ...)"""
    def err(msg):
        return ValueError("layer '%s' (%s): %s" % (lname, ltype, msg))

    def has(f):
        return f in b and np.asarray(b[f]).size > 0

    if ltype == "dagnn.Conv":
        if not has("size"):
            raise err("the block has no `size`")
        size = _ints(b["size"])
        size += [1] * (4 - len(size))                 # MATLAB drops trailing singleton dimensions here as well
        if len(size) != 4:
            raise err("`size` has %d values" % len(size))
        hasBias = bool(_number(b["hasBias"], "hasBias")) if has("hasBias") else nparams > 1
        if nparams != (2 if hasBias else 1):
            raise err("hasBias = %d but %d parameters" % (hasBias, nparams))
        pad = _ints(b["pad"]) if has("pad") else [0]
        stride = _ints(b["stride"]) if has("stride") else [1]
        dilate = _ints(b["dilate"]) if has("dilate") else [1]
        if len(pad) not in (1, 2, 4) or len(stride) not in (1, 2) or len(dilate) not in (1, 2):
            raise err("pad / stride / dilate of %d / %d / %d values" % (len(pad), len(stride), len(dilate)))
        pad = {1: pad * 4, 2: [pad[0], pad[0], pad[-1], pad[-1]], 4: pad}[len(pad)]
        return dagnn.Conv(size, hasBias, tuple((stride * 2)[:2]), tuple(pad), tuple((dilate * 2)[:2]))
    if ltype == "dagnn.BatchNorm":
        if nparams < 3:
            raise err("a BatchNorm needs three parameters (multiplier, bias, moments), the file gives %d" % nparams)
        if not has("numChannels"):
            raise err("the block has no `numChannels`")
        kw = {"epsilon": _number(b["epsilon"], "epsilon")} if has("epsilon") else {}
        return dagnn.BatchNorm(int(_number(b["numChannels"], "numChannels")), **kw)
    if ltype == "dagnn.ReLU":
        return dagnn.ReLU(_number(b["leak"], "leak") if has("leak") else 0.0)
    if ltype == "dagnn.LRN":
        if not has("param"):
            return dagnn.LRN()
        param = _numbers(b["param"])                  # 1 x 4 or 4 x 1
        if len(param) != 4:
            raise err("`param` has %d values, [N KAPPA ALPHA BETA] are four" % len(param))
        return dagnn.LRN(param)
    if ltype == "dagnn.Scale":
        if nparams:
            raise err("only the two-input form without parameters (SE blocks) is built")
        return dagnn.Scale()
    if ltype == "dagnn.Pooling":
        if not has("poolSize"):
            raise err("the block has no `poolSize`")
        ps = _ints(b["poolSize"])
        pad = _ints(b["pad"]) if has("pad") else [0]
        stride = _ints(b["stride"]) if has("stride") else [1]
        if len(ps) not in (1, 2) or len(pad) not in (1, 2, 4) or len(stride) not in (1, 2):
            raise err("poolSize / pad / stride of %d / %d / %d values" % (len(ps), len(pad), len(stride)))
        pad = {1: pad * 4, 2: [pad[0], pad[0], pad[-1], pad[-1]], 4: pad}[len(pad)]
        return dagnn.Pooling((ps * 2)[:2], tuple((stride * 2)[:2]), tuple(pad), _string(b["method"]) if has("method") else "max")
    if ltype == "dagnn.GlobalPooling":
        return dagnn.GlobalPooling(_string(b["method"]) if has("method") else "avg")
    if ltype == "dagnn.DropOut":
        return dagnn.DropOut(rate=_number(b["rate"], "rate")) if has("rate") else dagnn.DropOut()
    if ltype in ("dagnn.Loss", "dagnn.VerboseLoss"):
        loss = _string(b["loss"]) if has("loss") else "softmaxlog"
        if loss not in LOSSES:
            raise err("loss '%s' is not built (%s are)" % (loss, ", ".join(LOSSES)))
        return BLOCKS[ltype][0](loss)
    if ltype == "dagnn.SoftmaxCELoss":
        kw = {}
        if has("temperature"):
            kw["temperature"] = _py_number(_number(b["temperature"], "temperature"))
        if has("logitTargets"):
            kw["logitTargets"] = bool(_number(b["logitTargets"], "logitTargets"))
        return dagnn.SoftmaxCELoss(**kw)
    if ltype == "dagnn.HuberLoss":
        return dagnn.HuberLoss(_number(b["sigma"], "sigma")) if has("sigma") else dagnn.HuberLoss()
    if ltype == "dagnn.ErrorStats":
        return dagnn.ErrorStats(int(_number(b["numClasses"], "numClasses"))) if has("numClasses") else dagnn.ErrorStats()
    return BLOCKS[ltype][0]()        # Sigmoid, SoftMax, Sum, Axpy, EuclideanLoss: no fields


def _block_struct(block):
    """the struct saveobj writes for a block: exactly the fields _make_block reads"""
    t = _TYPE_OF.get(type(block))
    if t is None:
        raise ValueError("saveobj: no MatConvNet type for a %s block" % type(block).__name__)
    out = {}
    for f in BLOCKS[t][1]:
        v = getattr(block, f)
        if f == "pad":
            from . import vl
            v = _row(vl._pad4(v))
        elif f in ("stride", "dilate"):
            from . import vl
            v = _row(vl._pair(v, f))
        elif f in ("size", "poolSize", "param"):
            v = _row(v)
        elif isinstance(v, (bool, np.bool_)):
            v = bool(v)
        elif not isinstance(v, str):
            v = float(v)
        out[f] = v
    return t, out


# ---------------------------------------------------------------------------------------------
# execution order
# ---------------------------------------------------------------------------------------------
def execution_order(names, inputs, outputs):
    """Indices of the layers in an order in which every layer runs after the producers of its inputs.

    A file order that is executable already is kept as it is (the sort is stable in that sense: nothing moves).  Any
    other order is rebuilt from the wiring alone, so that the result does not depend on the order the file happened to
    have: depth first from the layers nobody consumes, and at a layer with several inputs the input with the fewest
    layers behind it first.  In a residual / SE bottleneck that is the shortcut, then the main branch, then the gate --
    the order in which dagnn.build_plan can fold the Sum / Axpy into the producing convolution's epilogue, because the
    shortcut operand exists when that convolution runs.  Only layers nothing tells apart by wiring (two loss heads on
    the same inputs) keep their file order.  Raises for a variable produced twice and for a cycle."""
    L = len(names)
    producer = {}
    for i in range(L):
        for v in outputs[i]:
            if v in producer:
                raise ValueError("variable '%s' is produced twice, by layer '%s' and by layer '%s'"
                                 % (v, names[producer[v]], names[i]))
            producer[v] = i
    preds = [sorted({producer[v] for v in inputs[i] if v in producer}) for i in range(L)]
    # Kahn, lowest file index first: the identity for an executable file, and the cycle check
    succs = [[] for _ in range(L)]
    for i in range(L):
        for p in preds[i]:
            succs[p].append(i)
    import heapq
    missing = [len(p) for p in preds]
    ready = [i for i in range(L) if missing[i] == 0]
    heapq.heapify(ready)
    kahn = []
    while ready:
        i = heapq.heappop(ready)
        kahn.append(i)
        for s in succs[i]:
            missing[s] -= 1
            if missing[s] == 0:
                heapq.heappush(ready, s)
    if len(kahn) != L:
        stuck = [names[i] for i in range(L) if missing[i] > 0]
        raise ValueError("the layers form a cycle: %s" % ", ".join("'%s'" % n for n in stuck[:8]))
    if kahn == list(range(L)):
        return kahn
    anc = [0] * L                                        # bit sets of the layers behind each layer
    for i in kahn:
        a = 0
        for p in preds[i]:
            a |= anc[p] | (1 << p)
        anc[i] = a
    weight = [bin(a).count("1") for a in anc]

    def children(i):
        seen, out = set(), []
        for pos, v in enumerate(inputs[i]):
            p = producer.get(v)
            if p is not None and p not in seen:
                seen.add(p)
                out.append((weight[p], pos, p))
        return [p for _, _, p in sorted(out)]

    sinks = sorted((i for i in range(L) if not succs[i]), key=lambda i: (weight[i], i))
    order, done = [], [False] * L
    for s in sinks:
        if done[s]:
            continue
        done[s] = True
        stack = [(s, iter(children(s)))]
        while stack:
            i, it = stack[-1]
            for c in it:
                if not done[c]:
                    done[c] = True
                    stack.append((c, iter(children(c))))
                    break
            else:
                order.append(i)
                stack.pop()
    return order


# ---------------------------------------------------------------------------------------------
# loadobj
# ---------------------------------------------------------------------------------------------
def _param_value(pname, value, shape, exact=False):
    a = np.asarray(value)
    if a.dtype.kind not in "fiub":
        raise ValueError("parameter '%s': the value is %s, not numeric" % (pname, a.dtype))
    want = tuple(int(s) for s in shape)
    if exact and tuple(a.shape) != want or a.size != int(np.prod(want)):
        raise ValueError("parameter '%s': the file holds %s, the layer needs %s"
                         % (pname, " x ".join(str(s) for s in a.shape), " x ".join(str(s) for s in want)))
    return np.asfortranarray(a.astype(np.float32).reshape(want, order="F"))


def _average_image(meta):
    norm = meta.get("normalization") if isinstance(meta, dict) else None
    if not isinstance(norm, dict) or "averageImage" not in norm:
        return
    a = np.asarray(norm["averageImage"], np.float64)
    if a.size != 3:
        # the reference reshapes it to 1 x 1 x 3 (fetch_emovoxceleb_imdb.m getImageBatch) and fails there otherwise
        raise ValueError("meta.normalization.averageImage holds %s values, three (one per colour plane) are needed"
                         % " x ".join(str(s) for s in a.shape))
    norm["averageImage"] = [float(v) for v in a.ravel(order="F")]


def loadobj(s):
    """net = dagnn.DagNN.loadobj(s).  `s`: the struct of a model file as scipy.io.loadmat returns it (the whole file, a
    file with the struct in `net`, or that struct), or what saveobj returned.  Everything is checked before anything is
    built: an unknown block type, an unsupported dagnn.Loss, a parametrised dagnn.Scale, a BatchNorm short of
    parameters and a parameter of the wrong size raise a ValueError that names the layer / parameter."""
    s = s if isinstance(s, dict) else _struct(s, "loadobj")
    if "net" in s and "layers" not in s:
        s = _struct(s["net"], "net")                                  # if isfield(net, 'net'), net = net.net ; end
    if "layers" not in s:
        raise ValueError("loadobj: the struct has no `layers` (fields: %s)" % ", ".join(k for k in s if not k.startswith("__")))
    layers = []
    for l in _structs(s["layers"]):
        name, ltype = _string(l["name"]), _string(l["type"])
        if ltype not in BLOCKS:
            raise ValueError("layer '%s': block type '%s' is not built (%s are)"
                             % (name, ltype, ", ".join(sorted(BLOCKS))))
        blk = l.get("block")
        layers.append({"name": name, "type": ltype, "inputs": _cellstr(l.get("inputs")),
                       "outputs": _cellstr(l.get("outputs")), "params": _cellstr(l.get("params")),
                       "block": _structs(blk)[0] if len(_structs(blk)) else {}})
    names = [l["name"] for l in layers]
    if len(set(names)) != len(names):
        dup = sorted(n for n in set(names) if names.count(n) > 1)
        raise ValueError("There is already a layer with name '%s'." % dup[0])
    filep = {}                                                        # file order (getParamIndex follows it)
    for p in _structs(s.get("params")):
        pname = _string(p["name"])
        filep[pname] = {"value": p.get("value"),
                        "learningRate": _number(p["learningRate"], pname) if "learningRate" in p else 1.0,
                        "weightDecay": _number(p["weightDecay"], pname) if "weightDecay" in p else 1.0,
                        "trainMethod": _string(p["trainMethod"]) if "trainMethod" in p and
                        np.asarray(p["trainMethod"]).size else None}
    blocks = [_make_block(l["name"], l["type"], l["block"], len(l["params"])) for l in layers]
    values = {}
    for l, b in zip(layers, blocks):
        for k, pname in enumerate(l["params"]):
            if pname not in filep:
                raise ValueError("layer '%s' (%s): the file has no parameter '%s'" % (l["name"], l["type"], pname))
            if pname in values:
                continue                                              # shared parameter: the first user's shape
            val = filep[pname]["value"]
            if val is None or np.asarray(val).size == 0:
                raise ValueError("parameter '%s' (layer '%s') has no value" % (pname, l["name"]))
            if isinstance(b, dagnn.Conv):
                values[pname] = _param_value(pname, val, b.size if k == 0 else (b.size[3], 1))
            elif isinstance(b, dagnn.BatchNorm):
                C = b.numChannels
                values[pname] = _param_value(pname, val, (C, 2) if k == 2 else (C, 1), exact=k == 2)
                if k == 2 and filep[pname]["trainMethod"] is None:
                    filep[pname]["trainMethod"] = "average"
            else:
                raise ValueError("layer '%s' (%s) takes no parameters, the file gives it '%s'" % (l["name"], l["type"], pname))
    meta = _to_python(_struct(s["meta"], "meta")) if "meta" in s and len(_structs(s["meta"])) else {}
    _average_image(meta)
    order = execution_order(names, [l["inputs"] for l in layers], [l["outputs"] for l in layers])
    precious = {_string(v["name"]) for v in _structs(s.get("vars"))
                if "precious" in v and np.asarray(v["precious"]).size and bool(np.asarray(v["precious"]).ravel()[0])}

    net = dagnn.DagNN()
    for pname, p in filep.items():
        net.params[pname] = dagnn.Param(pname, values.get(pname), p["learningRate"], p["weightDecay"],
                                        p["trainMethod"] or "gradient")
    for pos, i in enumerate(order):
        l = layers[i]
        if isinstance(blocks[i], dagnn.DropOut):
            blocks[i].seed = pos                  # the mask stream zoo.insert_dropout gives: the layer's position
        blocks[i].net = net
        net.layers.append(dagnn._LayerRec(l["name"], blocks[i], l["inputs"], l["outputs"], l["params"]))
    net.rebuild()
    for v in precious:
        if v in net.vars:
            net.vars[v].precious = True
    net.meta = meta
    return net


# ---------------------------------------------------------------------------------------------
# saveobj
# ---------------------------------------------------------------------------------------------
def saveobj(net):
    """s = net.saveobj(): the struct MatConvNet's DagNN.saveobj writes, as scipy.io.savemat takes it.  Parameters that
    live on the device are downloaded; `single` values."""
    import torch
    from . import vl
    layers = []
    for l in net.layers:
        t, b = _block_struct(l.block)
        layers.append({"name": l.name, "type": t, "inputs": _cell(list(l.inputs)), "outputs": _cell(list(l.outputs)),
                       "params": _cell(list(l.params)), "block": b})
    params = []
    for p in net.params.values():
        v = p.value
        if isinstance(v, torch.Tensor):
            v = vl.to_numpy(v)
        v = np.zeros((0, 0), np.float32) if v is None else np.asfortranarray(np.asarray(v, np.float32))
        params.append({"name": p.name, "value": v, "learningRate": float(p.learningRate),
                       "weightDecay": float(p.weightDecay), "trainMethod": str(p.trainMethod)})
    vars_ = [{"name": v.name, "precious": bool(v.precious)} for v in net.vars.values()]
    return {"vars": _struct_array(vars_, ["name", "precious"]),
            "params": _struct_array(params, ["name", "value", "learningRate", "weightDecay", "trainMethod"]),
            "layers": _struct_array(layers, ["name", "type", "inputs", "outputs", "params", "block"]),
            "meta": _from_python(net.meta)}


# ---------------------------------------------------------------------------------------------
# files
# ---------------------------------------------------------------------------------------------
def read_mat(path):
    """the variables of a v5 ... v7 MAT-file (scipy.io.loadmat); a v7.3 file is HDF5 and is refused"""
    import scipy.io as sio
    path = os.fspath(path)
    if not os.path.isfile(path):
        raise FileNotFoundError("no model file at %s" % path)
    with open(path, "rb") as f:
        head = f.read(len(V73_HEADER))
    if head == V73_HEADER:
        raise ValueError("%s is a MATLAB 7.3 (HDF5) file, which is not read here: re-save it in MATLAB with "
                         "save(path, '-struct', 'net', '-v7')" % path)
    # mat_dtype: every array in the class MATLAB would give it (logical stays logical, compactly stored doubles are doubles)
    return {k: v for k, v in sio.loadmat(path, mat_dtype=True).items() if not k.startswith("__")}


def rewritable(x):
    """what read_mat returned, in the form scipy.io.savemat writes back unchanged: a struct without fields is read as a
    1 x 1 cell holding None, which savemat would refuse"""
    if isinstance(x, dict):
        return {k: rewritable(v) for k, v in x.items()}
    if not isinstance(x, np.ndarray) or (x.dtype.names is None and x.dtype != object):
        return x
    if x.dtype.names is None and x.size == 1 and x.ravel()[0] is None:
        return {}
    out = np.empty(x.shape, x.dtype)
    for idx in np.ndindex(*x.shape):
        if x.dtype.names is None:
            out[idx] = rewritable(x[idx])
        else:
            out[idx] = tuple(rewritable(x[idx][f]) for f in x.dtype.names)
    return out


def write_mat(path, variables):
    """scipy.io.savemat into a temporary file that is renamed into place (as train.save_checkpoint does); the header
    text is a fixed one, so that saving the same net twice gives the same bytes"""
    import io
    import scipy.io as sio
    path = os.fspath(path)
    buf = io.BytesIO()
    sio.savemat(buf, variables)
    raw = bytearray(buf.getvalue())
    raw[:116] = HEADER_TEXT.ljust(116, b" ")
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(raw)
    os.replace(tmp, path)


def load_mat(path):
    """net = dagnn.load_mat(path): load(path), `if isfield(net, 'net'), net = net.net`, dagnn.DagNN.loadobj(net)"""
    return loadobj(read_mat(path))


def save_mat(net, path, wrap=None):
    """dagnn.save_mat(net, path): save(path, '-struct', 'net'); with wrap='net' the struct goes into that field, the
    form of a cnn_train_dag checkpoint (net next to stats / state)"""
    s = saveobj(net)
    write_mat(path, {wrap: s} if wrap else s)

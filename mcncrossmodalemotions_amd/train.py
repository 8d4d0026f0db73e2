"""cnn_train_dag step mirror: forward + backward + ParameterServer + accumulateGradients.

Reference call: cnn_train_dag(net, imdb, getBatchFn, 'learningRate', logspace(-4,-5,300),
'batchSize', 64, 'gpus', ..., 'parameterServer', struct('method','tmove'), ...)
(emoVoxCeleb/run_distillation.m:170-182).  The loop itself stays on the host; per minibatch it is
    net.eval(inputs, {'objective', 1})          -> HIP kernels
    parserv.push / sync / pull                  -> one RCCL sum-all-reduce of the flat der buffer
    accumulateGradients (momentum 0.9, wd 5e-4) -> fused HIP SGD / moving-average kernels
                                                   ('solver' / 'nesterovUpdate': fused HIP solver kernel)
Data parallelism follows MatConvNet: each worker takes a shard of the minibatch, BN statistics
are per worker, gradients are summed and divided by the GLOBAL batch size.
"""
import ctypes as C
import pickle

import numpy as np
import torch

from . import _lib, vl

# @solver.<name> of MatConvNet's +solver package [EXT] (vl.SOLVERS also lists the default solver's nesterovUpdate arm)
SOLVER_NAMES = tuple(k for k in vl.SOLVERS if k != "nesterov")


class TrainOpts:
    def __init__(self, learningRate=None, momentum=0.9, weightDecay=5e-4, batchSize=64,
                 derOutputs=("objective", 1), solver=None, solverOpts=None, nesterovUpdate=False):
        # run_distillation.m:76,87: 300 mini-epochs, logspace(-4, -5, 300)
        self.learningRate = np.logspace(-4, -5, 300) if learningRate is None else np.atleast_1d(learningRate)
        self.momentum = momentum
        self.weightDecay = weightDecay
        self.batchSize = batchSize
        self.derOutputs = list(derOutputs)
        # cnn_train_dag's 'solver' (None = its default, SGD with momentum), 'solverOpts' and 'nesterovUpdate' [EXT]
        if solver is not None and solver not in SOLVER_NAMES:
            raise ValueError("unknown solver %r (None or one of %s)" % (solver, ", ".join(SOLVER_NAMES)))
        if solver is None and solverOpts:
            raise ValueError("solverOpts without a solver (the default solver takes momentum / nesterovUpdate)")
        self.solver = solver
        self.solverOpts = vl.solver_opts(solver, solverOpts) if solver is not None else {}
        self.nesterovUpdate = bool(nesterovUpdate)     # as in MatConvNet: read by the default solver only


class ParameterServer:
    """ParameterServer.{start, push, sync, pull, stop} of MatConvNet [EXT] (selected with
    'parameterServer', struct('method','tmove') at run_distillation.m:88,181) as a sum-all-reduce over RCCL.

        push(flat[a:b])   start summing that range over all workers as soon as the kernels already enqueued on the
                          current stream have produced it; returns at once
        sync()            the current stream waits (on the device) for every push since the last sync; the sums are
                          then in place ("pull" is the identity: the reduction is in place)

    backend 'rccl-capi' : the library's own communicator behind the C ABI (xm_comm_init + xm_parserv_push /
                          xm_parserv_sync) -- what a MATLAB spmd host would bind; the 128-byte unique id travels
                          through torch.distributed's store here (labBroadcast there);
    backend 'torch'     : torch.distributed.all_reduce(async_op=True) (nccl == RCCL on ROCm, gloo on the CPU tests)."""

    def __init__(self, backend="torch"):
        self.backend = backend
        self.world = 1
        self.rank = 0
        self._started = False
        self._handles = []
        self.group = None     # backend 'torch': the process group the exchange runs on (None = the default group)

    _generation = 0      # id exchanges of this process so far (store keys; every worker makes the same calls)
    _agreement = 0       # start_agreed() rounds of this process so far (its own counter: see start_agreed)
    store_timeout_s = 120.0   # how long a worker waits for another worker's key before it counts it as failed

    @staticmethod
    def _store():
        from torch.distributed.distributed_c10d import _get_default_store
        return _get_default_store()

    @classmethod
    def _wait_keys(cls, store, keys):
        """True when every key is there within store_timeout_s (a worker that died never writes its own)"""
        import datetime
        import sys
        try:
            store.wait(list(keys), datetime.timedelta(seconds=cls.store_timeout_s))
            return True
        except Exception as e:   # noqa: BLE001 -- torch raises RuntimeError / DistStoreError depending on the store
            # a timeout is an answer ("that worker is gone"); anything else (broken store, lost connection) is reported
            # as what it is before it is treated the same way
            if "timeout" not in str(e).lower() and "timed out" not in str(e).lower():
                print("ParameterServer: store.wait failed: %s: %s" % (type(e).__name__, e), file=sys.stderr, flush=True)
            return False

    def start(self):
        if self._started:
            return
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            self.world, self.rank = dist.get_world_size(), dist.get_rank()
        if (self.world > 1 or self.force) and self.backend == "rccl-capi":
            buf = (C.c_char * 128)()
            raw = None
            if self.world > 1:
                # the 128-byte id travels through the process group's key-value store (labBroadcast in a MATLAB host):
                # host memory only -- no device allocation and no collective may precede xm_comm_init (xmodal.h "CALL
                # ORDER").  The key's generation is taken BEFORE anything can fail (library load included), so that
                # every worker uses the same key whatever happens to it, and a worker 0 that cannot produce the id
                # says so under that key instead of leaving the others waiting for it.
                ParameterServer._generation += 1
                gen = ParameterServer._generation
                key = "xm_comm_id/%d" % gen
                store = self._store()
                err, L = None, None
                try:
                    if self.rank == 0:
                        try:
                            rc = _lib.load().xm_comm_unique_id(buf)
                        except Exception:
                            store.set(key, b"no")
                            raise
                        store.set(key, b"ok" + bytes(buf) if rc == 0 else b"no")
                        _lib.check(rc)
                    if not self._wait_keys(store, [key]):
                        raise RuntimeError("ParameterServer: no communicator id from worker 0 within %.0f s"
                                           % self.store_timeout_s)
                    got = bytes(store.get(key))
                    if not got.startswith(b"ok"):
                        raise RuntimeError("ParameterServer: worker 0 could not create the communicator id")
                    raw = got[2:130]
                    L = _lib.load()
                except Exception as e:   # noqa: BLE001 -- posted below, re-raised after the ready round
                    err = e
                # READY round (round-5 advisor): xm_comm_init is ncclCommInitRank, which blocks in the RCCL bootstrap
                # until EVERY rank has called it.  A worker that failed above (no library, no id) never will, so the
                # healthy ones must not enter it: each worker posts whether it holds the library and the id, and the
                # communicator is created only when all of them do.
                ready = ["xm_comm_ready/%d/%d" % (gen, r) for r in range(self.world)]
                store.set(ready[self.rank], b"0" if err is not None else b"1")
                all_ready = self._wait_keys(store, ready) and all(bytes(store.get(k)) == b"1" for k in ready)
                if err is not None:
                    raise err
                if not all_ready:
                    raise RuntimeError("ParameterServer: another worker cannot create the communicator (it holds no "
                                       "library or no id); xm_comm_init not entered")
            else:
                L = _lib.load()
                _lib.check(L.xm_debug_comm_force_single(1))
                _lib.check(L.xm_comm_unique_id(buf))
                raw = bytes(buf)
            _lib.check(L.xm_comm_init(C.c_char_p(raw), self.rank, self.world))
        self._started = True

    _choice = 0          # choose_backend() rounds of this process so far

    @classmethod
    def choose_backend(cls):
        """'rccl-capi' or 'torch' for parameterServer = 'tmove', decided ONCE FOR ALL workers from what they post to the
        process group's store (round-5 advisor: each worker used to infer it locally from device_count() and
        LOCAL_WORLD_SIZE; workers that disagreed -- heterogeneous nodes, several workers on one device -- left some of
        them in the agreement round's store timeouts): every worker posts (host name, its current device); the library's
        communicator carries the exchange only when every worker sits on its OWN device of its host, because RCCL refuses
        two ranks on one device.  Same inputs on every worker => same answer on every worker."""
        import os
        import socket
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() < 2:
            return "torch"
        cls._choice += 1
        store, world, rank = cls._store(), dist.get_world_size(), dist.get_rank()
        dev = torch.cuda.current_device() if torch.cuda.is_available() else -1
        if os.environ.get("XM_DEBUG_DIST") == "gloo0":
            dev = -1                       # all workers share cuda:0 on purpose (functional runs over gloo)
        keys = ["xm_ps_where/%d/%d" % (cls._choice, r) for r in range(world)]
        store.set(keys[rank], ("%s|%d" % (socket.gethostname(), dev)).encode())
        if not cls._wait_keys(store, keys):
            return "torch"
        where = [bytes(store.get(k)).decode() for k in keys]
        distinct = len(set(where)) == world and all(not w.endswith("|-1") for w in where)
        return "rccl-capi" if distinct else "torch"

    @classmethod
    def start_agreed(cls, backend="rccl-capi", force=False):
        """Start the `backend` ParameterServer on every worker, or -- if ANY worker failed to -- torch.distributed
        on all of them: the outcome is agreed through the process group's store (host side, nothing on the device),
        so that no worker is left inside a collective the others never enter.  Returns the started instance.

        The agreement has its OWN round counter, advanced unconditionally before anything else: a worker that fails
        early in start() (it cannot even load the library) still writes its outcome under the key the others read.
        Two rounds: every worker posts its own outcome, then its VERDICT (all outcomes seen and good); the result is
        the AND of the verdicts.  A key that does not arrive within store_timeout_s counts as a failure on the
        worker that waited, and its verdict carries that to the others."""
        import sys
        import torch.distributed as dist
        cls._agreement += 1
        gen = cls._agreement
        ps = cls(backend)
        ps.force = force
        ok = 1
        try:
            ps.start()
        except Exception as e:   # noqa: BLE001 -- reported, then agreed on with the other workers
            print("ParameterServer(%s) failed to start: %s" % (backend, e), file=sys.stderr, flush=True)
            ok = 0
        # (the round runs whatever the backend: workers that were asked for different backends still meet here)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            store, world, rank = cls._store(), dist.get_world_size(), dist.get_rank()
            for phase in ("ok", "verdict"):
                keys = ["xm_ps_%s/%d/%d" % (phase, gen, r) for r in range(world)]
                store.set(keys[rank], b"1" if ok else b"0")
                ok = int(cls._wait_keys(store, keys) and all(bytes(store.get(k)) == b"1" for k in keys))
        if not ok:
            try:
                ps.stop()
            except Exception:    # noqa: BLE001
                pass
            ps = cls("torch")
            ps.force = force
            ps.start()
        return ps

    force = False  # debugging: run the collectives even with a single worker
    overlap = True  # bucketed exchange overlapped with the backward pass (GradBuckets); False: one exchange after it

    @property
    def active(self):
        return self.world > 1 or self.force

    def push(self, part):
        if not self.active or part.numel() == 0:
            return
        if self.backend == "rccl-capi":
            _lib.check(_lib.load().xm_parserv_push(C.c_void_p(part.data_ptr()), part.numel(),
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        else:
            import torch.distributed as dist
            self._handles.append(dist.all_reduce(part, op=dist.ReduceOp.SUM, group=self.group, async_op=True))

    def sync(self):
        if self.backend == "rccl-capi":
            if self.active:
                _lib.check(_lib.load().xm_parserv_sync(C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        else:
            for h in self._handles:
                h.wait()
            self._handles = []

    def allreduce_(self, flat):
        """one exchange of a whole buffer (push + sync)"""
        self.push(flat)
        self.sync()

    def comm_count(self):
        """worker count as the communicator itself reports it (ncclCommCount / the process group)"""
        if self.backend == "rccl-capi":
            n = C.c_int(0)
            _lib.check(_lib.load().xm_comm_count(C.byref(n)))
            return int(n.value)
        import torch.distributed as dist
        return dist.get_world_size(self.group) if dist.is_initialized() else 1

    def rccl_count(self):
        """ranks of the RCCL communicator the exchange runs on, or None when it does not run over RCCL: the
        library's own communicator (ncclCommCount), or torch's process group when that group's backend is nccl"""
        if not self.active:
            return None
        if self.backend == "rccl-capi":
            return self.comm_count()
        import torch.distributed as dist
        if dist.is_initialized() and dist.get_backend(self.group) == "nccl":
            return dist.get_world_size(self.group)
        return None

    def stop(self):
        if not self._started:
            if self.backend == "rccl-capi":
                _lib.load().xm_comm_destroy()     # a half-initialised communicator (failed start)
            return
        self.sync()
        if self.backend == "rccl-capi" and self.active:
            _lib.check(_lib.load().xm_comm_destroy())
        self._started = False


class GradBuckets:
    """Bucket plan of the overlapped gradient exchange.

    The derivatives of a network become ready from its LAST layer to its first.  The flat derivative buffer holds
    the filters of one (trainMethod, lr, wd) group contiguously in layer order, so the tail of that segment is
    complete first.  The plan cuts the filter segments, from the back, into buckets of >= `target_bytes` at
    parameter boundaries; a bucket is pushed as soon as the earliest of its layers has enqueued its filter
    derivative (dagnn calls gradHook(layer name) right there, on the stream the derivative was enqueued on), the
    rest of the backward pass hides the exchange.  Whatever is not covered (biases, bnorm multipliers / biases /
    moments -- small) goes out as one or two ranges after the pass.  Every element is pushed exactly once.

    student (66.6 MB):  [fc6f fc7f fc8f] 54.5 MB on fc6  |  [conv1f..conv5f] 12 MB on conv1 ... | rest
    SE-ResNet-50 (config 5, 104 MB): ~4 buckets of 24-32 MB along res5 / res4 / res3-2 | rest."""

    def __init__(self, net, target_bytes=24 << 20):
        from . import dagnn
        flat = net._flat
        self.flat = flat
        total = int(flat.der.numel())
        order = {l.name: i for i, l in enumerate(net.layers)}
        # filter parameters written by exactly one conv layer, with their flat ranges
        items = []
        for l in net.layers:
            if isinstance(l.block, dagnn.Conv):
                p = net.params[l.params[0]]
                if p.fanout == 1 and hasattr(p, "_flat_off"):
                    n = (int(p.value.numel()) + 3) // 4 * 4
                    items.append((p._flat_off, p._flat_off + n, l.name))
        items.sort()
        # maximal runs of adjacent filters (one run per (trainMethod, lr, wd) segment in practice)
        runs, cur = [], []
        for it in items:
            if cur and it[0] != cur[-1][1]:
                runs.append(cur)
                cur = []
            cur.append(it)
        if cur:
            runs.append(cur)
        self.buckets = []      # (a, b, trigger layer)
        for run in runs:
            acc = []
            for it in reversed(run):           # from the back: those derivatives are ready first
                acc.append(it)
                if 4 * (acc[0][1] - acc[-1][0]) >= target_bytes:
                    self.buckets.append((acc[-1][0], acc[0][1], min((x[2] for x in acc), key=lambda n: order[n])))
                    acc = []
            if acc:
                self.buckets.append((acc[-1][0], acc[0][1], min((x[2] for x in acc), key=lambda n: order[n])))
        # canonical push order = the order the backward pass reaches the trigger layers (last layer first); every
        # worker -- also one whose shard is empty and that runs no backward pass -- issues its collectives in it
        self.buckets.sort(key=lambda x: -order[x[2]])
        self.by_trigger = {}
        for a, b, t in self.buckets:
            self.by_trigger.setdefault(t, []).append((a, b))
        covered = sorted((a, b) for a, b, _ in self.buckets)
        self.rest, pos = [], 0
        for a, b in covered:
            if a > pos:
                self.rest.append((pos, a))
            pos = b
        if pos < total:
            self.rest.append((pos, total))
        self._sent = set()
        self.log = None        # tests: list that receives every pushed (a, b)

    def ranges(self):
        return [(a, b) for a, b, _ in self.buckets] + self.rest

    def begin(self):
        self._sent = set()

    def _push(self, parserv, a, b):
        if self.log is not None:
            self.log.append((a, b))
        parserv.push(self.flat.der[a:b])

    def on_layer(self, parserv, name):
        for a, b in self.by_trigger.get(name, ()):
            self._sent.add((a, b))
            self._push(parserv, a, b)

    def finish(self, parserv):
        for a, b, _ in self.buckets:           # trigger layer absent from this pass (frozen / idle worker)
            if (a, b) not in self._sent:
                self._push(parserv, a, b)
        for a, b in self.rest:
            self._push(parserv, a, b)
        parserv.sync()


def _in_buckets(buckets, a, b):
    """does an early bucket overlap the flat range [a, b)?  (the moments segment is re-weighted after the backward
    pass, so it must not have been pushed during it -- filters never share a bucket with it, this is a guard)"""
    return any(x < b and a < y for x, y, _ in buckets.buckets)


def shard_batch(batch, rank, world):
    """cnn_train_dag: batch(labindex:numlabs:end) -- interleaved shards."""
    return list(batch)[rank::world]


def solver_state(flat, solver):
    """the solver's state beyond flat.mom (state slot 1), made on first use: adam's update count per segment on the host
    and, for adadelta and adam only, a second flat buffer; all zero, MatConvNet's empty state"""
    if flat.solver_t is None:
        flat.solver_t = [0] * len(flat.segments)
    if vl.SOLVERS[solver][2] and flat.state2 is None:
        flat.state2 = torch.zeros_like(flat.mom)


def accumulate_gradients(net, opts, lr, global_batch, moments_denom=1.0):
    """accumulateGradients of cnn_train_dag: per flat segment one fused launch -- xm_sgd_update for the default solver
    (solver = []), xm_solver_update for opts.solver (@solver.adagrad / rmsprop / adadelta / adam) and for the default
    solver's nesterovUpdate arm.
    `moments_denom`: 1 for a single worker (der = the batch moments); the global batch size when the exchanged der
    is sum_w moments_w * batch_w (train_step does that weighting)."""
    flat = net._flat
    kind = opts.solver if opts.solver is not None else ("nesterov" if opts.nesterovUpdate else None)
    if opts.solver is not None:
        solver_state(flat, opts.solver)
    for k, ((method, lr_mult, wd_mult), a, b) in enumerate(flat.segments):
        if b == a:
            continue
        if method == "average":
            vl.average_update(flat.val[a:b], flat.der[a:b], lr_mult, moments_denom)
        elif kind is None:
            vl.sgd_update(flat.val[a:b], flat.mom[a:b], flat.der[a:b], lr * lr_mult, opts.momentum,
                          opts.weightDecay * wd_mult, global_batch)
        else:
            this_lr, this_decay = lr * lr_mult, opts.weightDecay * wd_mult
            if not (this_lr > 0 or this_decay > 0):      # cnn_train_dag: if thisLR > 0 || thisDecay > 0
                continue
            if kind == "nesterov":
                vl.solver_update(kind, flat.val[a:b], flat.mom[a:b], None, flat.der[a:b], this_lr, this_decay,
                                 global_batch, momentum=opts.momentum)
                continue
            if kind == "adam":
                flat.solver_t[k] += 1
            s2 = flat.state2[a:b] if vl.SOLVERS[kind][2] else None
            vl.solver_update(kind, flat.val[a:b], flat.mom[a:b], s2, flat.der[a:b], this_lr, this_decay,
                             global_batch, t=max(flat.solver_t[k], 1), **opts.solverOpts)
    net.paramGeneration = getattr(net, "paramGeneration", 0) + 1   # folded / cached views of the parameters are stale


def train_step(net, inputs, opts, epoch=0, parserv=None, global_batch=None, input_events=None, local_batch=None):
    """One minibatch of cnn_train_dag's processEpoch in training mode.

    `inputs` None: this worker's interleaved shard of the minibatch is EMPTY (ragged tail smaller than the worker
    count): it contributes zero derivatives / zero-weight moments but still joins the exchange -- every collective
    is entered by every worker.  `local_batch`: samples of this worker's shard (default: global_batch / workers)."""
    if net._flat is None:
        net.pack_params()
    net.mode = "normal"
    world = parserv.world if parserv is not None else 1
    exchange = parserv is not None and parserv.active
    global_batch = global_batch or opts.batchSize
    if local_batch is None:
        local_batch = 0 if inputs is None else global_batch / world
    buckets = None
    if exchange and parserv.overlap:
        buckets = net.__dict__.get("_grad_buckets")
        if buckets is None or buckets.flat is not net._flat:
            buckets = net.__dict__["_grad_buckets"] = GradBuckets(net)
        buckets.begin()
    net.gradHook = None
    if buckets is not None and inputs is not None and not any(m == "average" for (m, _, _), a, b in net._flat.segments
                                                              if b > a and _in_buckets(buckets, a, b)):
        net.gradHook = lambda name: buckets.on_layer(parserv, name)
    if inputs is None:
        net._flat.der.zero_()
    else:
        net.eval(inputs, opts.derOutputs, input_events=input_events)
    if exchange:
        # MatConvNet [EXT]: dagnn.BatchNorm returns moments * (worker batch size), accumulateGradients divides the
        # workers' sum by the global batch size -- ragged shards are weighted by their sample counts
        for (method, _, _), a, b in net._flat.segments:
            if method == "average" and b > a:
                vl.scale_(net._flat.der[a:b], float(local_batch))
        if buckets is not None:
            buckets.finish(parserv)
        else:
            parserv.allreduce_(net._flat.der)
    net.gradHook = None
    lr = float(opts.learningRate[min(epoch, len(opts.learningRate) - 1)])
    accumulate_gradients(net, opts, lr, global_batch, float(global_batch) if exchange else 1.0)
    if net.markHook is not None:
        net.markHook("upd")


def extractStats(stats, net):
    """stats = extractStats(stats, net) -- run_distillation.m:186-207: `.average` of every dagnn.Loss
    block under its output name; for dagnn.ErrorStats the per-class accuracies under the class names,
    their mean as `meanAcc`, and the class population as `<name>Pop`."""
    from . import dagnn
    stats = dict(stats or {})
    for l in net.layers:
        b = l.block
        if not isinstance(b, dagnn.LossBase):
            continue
        if isinstance(b, dagnn.ErrorStats):
            metrics, dist = b.average, b.classDist
            pop = dist / dist.sum() if dist.sum() > 0 else dist
            names = (net.meta.get("classes", {}).get("name") or
                     ["class%d" % (i + 1) for i in range(len(metrics))])
            stats["meanAcc"] = float(np.mean(metrics))
            for name, m in zip(names, metrics):
                stats[name] = float(m)
            for name, q in zip(names, pop):
                stats["%sPop" % name] = float(q)
        else:
            if b.ignoreAverage:
                continue
            stats[l.outputs[0]] = b.average
    return stats


def _reset_losses(net):
    from . import dagnn
    for l in net.layers:
        if isinstance(l.block, dagnn.LossBase):
            l.block.reset()


class _RunAhead:
    """bounded host run-ahead (two minibatches): a full HIP queue stalls launches for milliseconds"""

    def __init__(self, device):
        self.on = device is not None and device.type == "cuda"
        self.inflight = []

    def tick(self):
        if not self.on:
            return
        ev = torch.cuda.Event()
        ev.record()
        self.inflight.append(ev)
        if len(self.inflight) > 2:
            self.inflight.pop(0).synchronize()


def merge_loss_stats(net, parserv):
    """validation / training statistics are per-worker running sums (dagnn.Loss.average, ErrorStats counters):
    sum them over the workers before extractStats reads them, so that rank 0 reports -- and checkpoints -- the
    statistics of the whole subset, not of its own shard."""
    from . import dagnn
    if parserv is None or not parserv.active:
        return
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return
    dev = net.device if net.device is not None else torch.device("cpu")
    blocks = [l.block for l in net.layers if isinstance(l.block, dagnn.LossBase)]
    vals = []
    for b in blocks:
        if isinstance(b, dagnn.ErrorStats):
            C_ = b.numClasses
            vals.append(b._correct.reshape(-1).to(torch.float64) if b._correct is not None
                        else torch.zeros(C_, dtype=torch.float64, device=dev))
            vals.append(b._population.reshape(-1).to(torch.float64) if b._population is not None
                        else torch.zeros(C_, dtype=torch.float64, device=dev))
        else:
            b._fold()
            vals.append((b._sum.reshape(1).to(torch.float64) if b._sum is not None
                         else torch.zeros(1, dtype=torch.float64, device=dev)))
        vals.append(torch.tensor([float(b.numAveraged)], dtype=torch.float64, device=dev))
    if not vals:
        return
    t = torch.cat([v.to(dev) for v in vals])
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    pos = 0
    for b in blocks:
        if isinstance(b, dagnn.ErrorStats):
            C_ = b.numClasses
            if b._correct is None:
                b._correct = vl.mat_zeros(C_, 1, device=dev) if dev.type == "cuda" else torch.zeros(C_, 1).t().contiguous().t()
                b._population = b._correct.clone()
            b._correct.reshape(-1).copy_(t[pos:pos + C_].to(torch.float32))
            b._population.reshape(-1).copy_(t[pos + C_:pos + 2 * C_].to(torch.float32))
            pos += 2 * C_
        else:
            b._sum = t[pos].to(torch.float32).reshape(())
            pos += 1
        b.numAveraged = int(round(float(t[pos].item())))
        pos += 1


def process_epoch(net, imdb, getBatch, subset, opts, epoch, mode, parserv=None, extractStatsFn=extractStats):
    """processEpoch of cnn_train_dag [EXT]: one pass over `subset` in minibatches of opts.batchSize;
    each worker evaluates the interleaved shard batch(labindex:numlabs:end).  A ragged tail batch with fewer
    samples than workers leaves some shards empty: those workers still enter train_step (zero contribution) so
    that every collective is matched."""
    import time
    world = parserv.world if parserv is not None else 1
    rank = parserv.rank if parserv is not None else 0
    net.workerRank = rank          # dagnn.DropOut folds it into its seed: every shard draws its own masks
    _reset_losses(net)
    subset = list(subset)
    t0 = time.perf_counter()
    num = 0
    ahead = _RunAhead(net.device)
    for t in range(0, len(subset), opts.batchSize):
        batch = subset[t:t + opts.batchSize]
        shard = shard_batch(batch, rank, world)
        if mode == "train":
            inputs = getBatch(imdb, shard) if shard else None
            # (a getBatch whose targets are made on another stream says so: batch.BatchInputs.input_events)
            train_step(net, inputs, opts, epoch, parserv, len(batch), local_batch=len(shard),
                       input_events=getattr(inputs, "input_events", None))
        elif shard:
            net.mode = "test"
            inputs = getBatch(imdb, shard)
            net.eval(inputs, input_events=getattr(inputs, "input_events", None))
        num += len(batch)
        ahead.tick()
    merge_loss_stats(net, parserv)
    stats = extractStatsFn({}, net)   # the only host synchronisation of the pass
    stats["num"] = num
    stats["time"] = time.perf_counter() - t0
    return stats


def _segment_of(flat, off):
    """index of the flat segment that holds offset `off`"""
    return next(k for k, (_, a, b) in enumerate(flat.segments) if a <= off < b)


def save_checkpoint(net, path, info, epoch, opts=None):
    """net-epoch-<n>.pt: {parameter name: value / momentum} (self-describing: loadable into any net that has
    parameters of those names and shapes, e.g. emoVoxZoo(scratch=0) for inference), written to a temporary file and
    renamed into place so that a crash cannot leave a truncated file that `cont` would pick up.
    "momentum" is the first solver state whatever the solver.  With opts.solver set the file also carries "solver":
    {name, opts, state2: {parameter name: second state} (adadelta, adam), t: {parameter name: update count}}."""
    import os
    flat = net._flat
    solver = getattr(opts, "solver", None)
    vals, moms, st2, ts = {}, {}, {}, {}
    for name, p in net.params.items():
        n = int(p.value.numel())
        off = p._flat_off
        vals[name] = flat.val[off:off + n].reshape(tuple(reversed(p.value.shape))).clone()
        moms[name] = flat.mom[off:off + n].reshape(tuple(reversed(p.value.shape))).clone()
        if solver is not None:
            if flat.state2 is not None:
                st2[name] = flat.state2[off:off + n].reshape(tuple(reversed(p.value.shape))).clone()
            ts[name] = int(flat.solver_t[_segment_of(flat, off)]) if flat.solver_t is not None and n else 0
    # counter offsets of the dropout layers' Philox streams (training state: a resumed run must not repeat masks)
    rng = {l.name: int(l.block._offset) for l in net.layers if hasattr(l.block, "_offset")}
    ck = {"format": "xmodal-params-v2", "params": vals, "momentum": moms, "info": info, "epoch": epoch, "rng": rng}
    if solver is not None:
        ck["solver"] = {"name": solver, "opts": {k: float(v) for k, v in opts.solverOpts.items()}, "state2": st2,
                        "t": ts}
    tmp = path + ".tmp"
    torch.save(ck, tmp)
    os.replace(tmp, path)


_ANY_SOLVER = object()


def load_checkpoint(net, path, strict=True, solver=_ANY_SOLVER):
    """inverse of save_checkpoint (values stored in the flat buffers' memory order: reversed MATLAB shape).
    The whole file is validated against the net BEFORE anything is copied: a mismatch leaves the net untouched.
    `solver`: the solver of the run that resumes from the file (None = the default solver); a file written under another
    one is a CheckpointMismatch.  Not given (loading for evaluation): any file is accepted."""
    ck = torch.load(path, map_location=net.device, weights_only=True)
    if not isinstance(ck, dict) or ck.get("format") != "xmodal-params-v2" or not isinstance(ck.get("params"), dict):
        # an older-format or foreign file: unreadable for `cont` (skipped with a warning), not a mismatch
        raise CheckpointUnreadable("%s: not an xmodal-params-v2 checkpoint" % path)
    sv = ck.get("solver")
    if sv is not None and not (isinstance(sv, dict) and isinstance(sv.get("name"), str)):
        raise CheckpointUnreadable("%s: malformed solver state" % path)
    if solver is not _ANY_SOLVER and (sv["name"] if sv else None) != solver:
        raise CheckpointMismatch("%s was written with solver %r, this run uses solver %r" %
                                 (path, sv["name"] if sv else None, solver))
    if net._flat is None:
        net.pack_params()
    st2, ts = (sv.get("state2") or {}, sv.get("t") or {}) if sv else ({}, {})
    for name, p in net.params.items():
        if name in st2 and int(st2[name].numel()) != int(p.value.numel()):
            raise CheckpointMismatch("second solver state of %r: %d values in the checkpoint, %d in the net" %
                                     (name, st2[name].numel(), p.value.numel()))
    todo = []
    for name, p in net.params.items():
        if name not in ck["params"]:
            if strict:
                raise CheckpointMismatch("checkpoint has no parameter %r" % name)
            continue
        n = int(p.value.numel())
        src = ck["params"][name]
        if int(src.numel()) != n:
            raise CheckpointMismatch("parameter %r: %d values in the checkpoint, %d in the net" %
                                     (name, src.numel(), n))
        mom = ck.get("momentum", {}).get(name)
        if mom is not None and int(mom.numel()) != n:
            raise CheckpointMismatch("momentum of %r: %d values in the checkpoint, %d in the net" %
                                     (name, mom.numel(), n))
        todo.append((p._flat_off, n, src, mom))
    for off, n, src, mom in todo:
        net._flat.val[off:off + n].copy_(src.reshape(-1))
        if mom is not None:
            net._flat.mom[off:off + n].copy_(mom.reshape(-1))
    if sv is not None and sv["name"] in vl.SOLVERS:
        flat = net._flat
        flat.state2 = flat.solver_t = None          # the file's solver state replaces the net's, whole
        solver_state(flat, sv["name"])
        for name, p in net.params.items():
            n = int(p.value.numel())
            if name in st2:
                flat.state2[p._flat_off:p._flat_off + n].copy_(st2[name].reshape(-1))
            if n and name in ts:
                flat.solver_t[_segment_of(flat, p._flat_off)] = int(ts[name])
    for l in net.layers:
        if hasattr(l.block, "_offset") and l.name in (ck.get("rng") or {}):
            l.block._offset = int(ck["rng"][l.name])
    net.paramGeneration = getattr(net, "paramGeneration", 0) + 1
    return ck


class CheckpointMismatch(ValueError):
    """the file is a valid xmodal-params-v2 checkpoint of a DIFFERENT net (names / shapes): never skipped by `cont`"""


class CheckpointUnreadable(OSError):
    """the file unpickles but is not an xmodal-params-v2 checkpoint (older format, foreign .pt): `cont` skips it"""


def cnn_train_dag(net, imdb, getBatch, learningRate=None, batchSize=64, numEpochs=300, train=None, val=None,
                  cont=True, expDir=None, epochSize=float("inf"), parameterServer=None, extractStatsFn=extractStats,
                  momentum=0.9, weightDecay=5e-4, derOutputs=("objective", 1), randomSeed=0, verbose=False,
                  solver=None, solverOpts=None, nesterovUpdate=False):
    """[net, info] = cnn_train_dag(net, imdb, getBatch, 'learningRate', ..., 'batchSize', ..., 'numEpochs', ...,
    'train', ..., 'val', ..., 'continue', ..., 'expDir', ..., 'epochSize', ..., 'parameterServer', ...,
    'extractStatsFn', ...) -- the MatConvNet driver [EXT] as run_distillation.m:170-182 calls it.
    'solver' (None | 'adagrad' | 'rmsprop' | 'adadelta' | 'adam': @solver.<name>), 'solverOpts' (a dict; the solver's
    defaults fill the rest) and 'nesterovUpdate' (default solver only) are the driver's options of those names, as
    ferplus_baselines.m:70-80,140-141 can pass them through opts.train.

    Per epoch: shuffle `train` with the epoch's seed, keep the first `epochSize` samples (the reference's
    "mini-epochs"), one training pass, one validation pass in test mode, then a checkpoint
    `net-epoch-<n>.pt` in `expDir` (flat parameters + momentum + info) from which `cont` resumes.
    `gpus` is implicit: one process per GPU (torchrun), the process group gives the worker count."""
    import os
    opts = TrainOpts(learningRate=learningRate, momentum=momentum, weightDecay=weightDecay, batchSize=batchSize,
                     derOutputs=derOutputs, solver=solver, solverOpts=solverOpts, nesterovUpdate=nesterovUpdate)
    if len(opts.learningRate) < numEpochs:   # MatConvNet indexes min(epoch, numel(learningRate))
        pass
    parserv = parameterServer if isinstance(parameterServer, ParameterServer) else ParameterServer("torch")
    parserv.start()
    if net._flat is None:
        net.pack_params()
    train = list(train if train is not None else [])
    val = list(val if val is not None else [])
    info = {"train": [], "val": []}
    start = 0
    path = (lambda e: os.path.join(expDir, "net-epoch-%d.pt" % e)) if expDir else None
    if expDir and parserv.rank == 0:
        os.makedirs(expDir, exist_ok=True)
    if cont and expDir:
        done = sorted(e for e in range(1, numEpochs + 1) if os.path.exists(path(e)))
        while done:                      # newest readable checkpoint wins; unreadable ones are skipped
            try:
                ck = load_checkpoint(net, path(done[-1]), solver=opts.solver)
            except CheckpointMismatch:   # readable, but of another net: restarting would overwrite those files
                raise
            except (OSError, EOFError, RuntimeError, pickle.UnpicklingError, KeyError, ValueError, TypeError,
                    AttributeError) as e:   # truncated / damaged / foreign (CheckpointMismatch was re-raised above)
                print("cnn_train_dag: skipping unreadable checkpoint %s (%s)" % (path(done[-1]), e), flush=True)
                done.pop()
                continue
            start = done[-1]
            info = ck["info"]
            break
    for epoch in range(start, numEpochs):
        rng = np.random.default_rng(epoch + 1 + randomSeed)       # rng(epoch + opts.randomSeed)
        order = [train[i] for i in rng.permutation(len(train))]
        if epochSize < len(order):
            order = order[:int(epochSize)]
        info["train"].append(process_epoch(net, imdb, getBatch, order, opts, epoch, "train", parserv, extractStatsFn))
        info["val"].append(process_epoch(net, imdb, getBatch, val, opts, epoch, "val", parserv, extractStatsFn))
        if verbose and parserv.rank == 0:
            print("epoch %d: train %s | val %s" % (epoch + 1, info["train"][-1], info["val"][-1]), flush=True)
        if path and parserv.rank == 0:
            save_checkpoint(net, path(epoch + 1), info, epoch + 1, opts)
    parserv.stop()
    return net, info

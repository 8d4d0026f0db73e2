"""The library's kernel profiler (include/xmodal_prof.h) from Python: which kernels ran, how often, how long."""
import collections
import contextlib
import ctypes as C

import torch

from . import _lib

Row = collections.namedtuple("Row", "key name launches ms flops bytes")


def collect(L=None):
    """The records since the last enable, one Row per kernel instantiation in first-launch order."""
    L = L or _lib.load()
    n = L.xm_prof_collect(0, None, None, None, None)   # cap 0: writes nothing, returns the count
    keys, ms, fl, cnt = (C.c_int * n)(), (C.c_double * n)(), (C.c_double * n)(), (C.c_longlong * n)()
    L.xm_prof_collect(n, keys, ms, fl, cnt)
    nb = L.xm_prof_collect_bytes(0, None, None)
    bkeys, by = (C.c_int * nb)(), (C.c_double * nb)()
    L.xm_prof_collect_bytes(nb, bkeys, by)
    bytes_of = dict(zip(bkeys, by))
    rows = []
    for i in range(n):
        buf = C.create_string_buffer(128)
        _lib.check(L.xm_prof_kernel_name(keys[i], buf, 128))
        rows.append(Row(keys[i], buf.value.decode(), cnt[i], ms[i], fl[i], bytes_of.get(keys[i], 0.0)))
    return rows


@contextlib.contextmanager
def recording(L=None):
    """Records every profiled launch of the block; the device is synchronised before recording stops."""
    L = L or _lib.load()
    L.xm_prof_enable(1)
    try:
        yield
    finally:
        torch.cuda.synchronize()
        L.xm_prof_enable(0)


def kernels_run(fn, L=None):
    """(fn(), rows): the result of fn and the kernels it launched."""
    with recording(L):
        out = fn()
    return out, collect(L)

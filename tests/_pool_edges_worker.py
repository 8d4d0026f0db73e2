"""Worker of tests/test_gpu_norm_pool_edges.py: the 3 x 3 max-pooling cases of tests/pool_routing.py (LDS_CASES) -- forward,
forward with the routing table, backward with the plain signature, backward with the table -- results to an .npz.
Run in a fresh process (the library reads its path selectors once): python tests/_pool_edges_worker.py out.npz"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)


def run_case(vl, name, view=None):
    """the four calls of one case; `view` maps the device input to the view the kernels get"""
    import pool_routing as PR
    H, W, C, N, stride, pad = PR.LDS_CASES[name]
    x, dzdy = PR.lds_case_input(name)
    xd, dd = vl.from_numpy(x), vl.from_numpy(dzdy)
    if view is not None:
        xd = view(xd)
    y = vl.vl_nnpool(xd, PR.POOL3, stride=stride, pad=pad, method="max")
    y2, am = vl.vl_nnpool(xd, PR.POOL3, stride=stride, pad=pad, method="max", want_argmax=True)
    dx = vl.vl_nnpool(xd, PR.POOL3, dd, stride=stride, pad=pad, method="max")
    dx2 = vl.vl_nnpool(xd, PR.POOL3, dd, stride=stride, pad=pad, method="max", argmax=am)
    return {"y": vl.to_numpy(y), "y2": vl.to_numpy(y2), "am": am.cpu().numpy().reshape(y.shape, order="F"),
            "dx": vl.to_numpy(dx), "dx2": vl.to_numpy(dx2)}


def main(out):
    import pool_routing as PR
    from mcncrossmodalemotions_amd import vl
    res = {}
    for name in sorted(PR.LDS_CASES):
        for k, v in run_case(vl, name).items():
            res[name + "_" + k] = v
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1])

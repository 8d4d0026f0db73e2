"""fp64 numpy restatement of vl_nnnormalize [EXT: vl_nnnormalize.m, normalize_cpu], the reference of tests/test_gpu_lrn.py.

    PARAM = [N KAPPA ALPHA BETA], X is H x W x C x S
    m1 = floor((N - 1) / 2), m2 = N - 1 - m1, G(k) = [k - m1, k + m2] within the C channels
    L = KAPPA + ALPHA * sum_{t in G(k)} X(t)^2,  Y = X .* L.^(-BETA)
    DX(k) = DZDY(k) L(k)^(-BETA) - 2 ALPHA BETA X(k) sum_{t in [k - m2, k + m1]} DZDY(t) X(t) L(t)^(-BETA - 1)

tests/test_lrn_cpu.py checks it: the forward against torch's local_response_norm (odd N: torch pads even windows the
other way round), the backward against central differences of the forward."""
import numpy as np

TOL = 1e-4      # tests/test_gpu_ops.py: |hip - ref| <= TOL * max(1, max |ref|)

# (C, N): windows that clip at one end, at both, that cover every channel, even and odd, wider than 2 C
WINDOW_CASES = [(1, 1), (1, 5), (2, 5), (4, 5), (5, 5), (6, 5), (11, 5), (6, 4), (6, 2), (7, 6), (3, 8), (3, 7), (40, 5),
                (9, 9), (5, 11)]
VGG_M_PARAM = [5, 2, 1e-4, 0.75]


def strong(N, beta=0.75):
    """parameters under which a wrong window shows: KAPPA = ALPHA = 1"""
    return [N, 1.0, 1.0, beta]


def window(N, mirrored=False):
    m1 = (int(N) - 1) // 2
    m2 = int(N) - 1 - m1
    return (m2, m1) if mirrored else (m1, m2)


def covers_all(C, N):
    m1, m2 = window(N)
    return m1 >= C - 1 and m2 >= C - 1


def scale(x, param, mirrored=False):
    """L, the same size as x"""
    N, kappa, alpha, _ = param
    m1, m2 = window(N, mirrored)
    x = np.asarray(x, np.float64)
    sq = x * x
    C = x.shape[2]
    L = np.full(x.shape, float(kappa))
    for k in range(C):
        L[:, :, k] += alpha * sq[:, :, max(0, k - m1):min(C - 1, k + m2) + 1].sum(2)
    return L


def forward(x, param, mirrored=False):
    return np.asarray(x, np.float64) * scale(x, param, mirrored) ** (-float(param[3]))


def backward(x, param, dzdy):
    N, _, alpha, beta = param
    m1, m2 = window(N)
    x, dzdy = np.asarray(x, np.float64), np.asarray(dzdy, np.float64)
    L = scale(x, param)
    r = dzdy * x * L ** (-beta - 1.0)
    C = x.shape[2]
    dx = dzdy * L ** (-float(beta))
    for k in range(C):
        dx[:, :, k] -= 2.0 * alpha * beta * x[:, :, k] * r[:, :, max(0, k - m2):min(C - 1, k + m1) + 1].sum(2)
    return dx


def case(shape, seed):
    """(x, dzdy) ~ N(0, 1), float32 values held in Fortran order"""
    rng = np.random.default_rng(seed)
    x = np.asfortranarray(rng.standard_normal(shape).astype(np.float32))
    d = np.asfortranarray(rng.standard_normal(shape).astype(np.float32))
    return x, d

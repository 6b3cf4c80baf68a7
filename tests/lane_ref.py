"""The per-channel passes of the training step restated in numpy float64 (csrc/elementwise.hip: batch statistics, BN
apply, channel softmax; csrc/train.hip: BN backward, relu / max-pool adjoints), shared by tests/test_lane_ref_host.py
and tests/test_gpu_lanes.py.  Tensors are NHWC; channel results are [C].  Nothing here rounds except to_bf16 / to_f32:

    bn_stats         mean and biased variance over N,H,W, two-pass (the truth)
    bn_stats_3op     the kernel's last step on exact sums: m = S/M, v = max(SS/M - m*m, 0)
    bn_apply         act((x - mean) / sqrt(var + eps) * gamma + beta)
    bn_backward      g = dy * (y > 0);  dbeta = sum g;  dgamma = sum g*xhat;
                     dx = gamma * rstd * (g - dbeta/N - xhat * dgamma/N);  dbias = sum_p dx   (N = count or M)
    relu_backward    dy * (y > 0), optionally split into the first k channels and the rest
    maxpool_backward add + dy routed to each 2x2/2 SAME window's first maximum of x (TF MaxPoolGrad)
    relu_backward_bias   dz = (y > 0) * (dy + add), or with a pooled dy (y > 0) * (add + maxpool_backward(y, dy));
                         dbias = channel sums of dz rounded to f32 (the kernel sums its f32 value)
"""

import numpy as np
import torch

AX = (0, 1, 2)


def f64(a):
    return np.asarray(a, np.float64)


def to_f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def to_bf16(a):
    """Round to f32, then to bfloat16 with ties to even (what a kernel's f32 value stored as bf16 becomes)."""
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32)))
    return t.to(torch.bfloat16).to(torch.float64).numpy()


def bn_stats(x):
    # channel-major, so that numpy sums each channel's contiguous run pairwise (a strided reduction adds in sequence,
    # which at millions of pixels costs the digits the three-operation form is judged by)
    xt = np.ascontiguousarray(f64(x).reshape(-1, np.shape(x)[-1]).T)
    mean = xt.mean(axis=1)
    return mean, ((xt - mean[:, None]) ** 2).mean(axis=1)


def bn_stats_3op(x):
    x = f64(x)
    m_count = float(x.shape[0] * x.shape[1] * x.shape[2])
    m = x.sum(axis=AX) / m_count
    v = (x * x).sum(axis=AX) / m_count - m * m
    return m, np.maximum(v, 0.0)


def _chan(v, c, default):
    return np.full(c, default, np.float64) if v is None else f64(v)


def bn_preact(x, mean, var, gamma, beta, eps):
    x = f64(x)
    c = x.shape[-1]
    xh = (x - _chan(mean, c, 0.0)) / np.sqrt(_chan(var, c, 1.0) + eps)
    return xh * _chan(gamma, c, 1.0) + _chan(beta, c, 0.0)


def bn_apply(x, mean, var, gamma, beta, eps, act="none"):
    v = bn_preact(x, mean, var, gamma, beta, eps)
    if act == "relu":
        return np.maximum(v, 0.0)
    if act == "sigmoid":
        return 1.0 / (1.0 + np.exp(-v))
    assert act == "none"
    return v


def bn_backward(x, dy, y_mask, mean, var, gamma, eps, count=None, sums=None):
    """-> dx, dgamma, dbeta, dbias.  dgamma / dbeta are this tensor's own channel sums; ``sums`` = (sum g, sum g*xhat)
    over ``count`` pixels replaces them inside dx (SyncBN: the replicas' sums added)."""
    x, g = f64(x), f64(dy)
    c = x.shape[-1]
    if y_mask is not None:
        g = np.where(f64(y_mask) > 0.0, g, 0.0)
    r = 1.0 / np.sqrt(f64(var) + eps)
    xh = (x - f64(mean)) * r
    dbeta, dgamma = g.sum(axis=AX), (g * xh).sum(axis=AX)
    n = float(x.shape[0] * x.shape[1] * x.shape[2]) if count is None else float(count)
    sg, sgx = (dbeta, dgamma) if sums is None else (f64(sums[0]), f64(sums[1]))
    dx = _chan(gamma, c, 1.0) * r * (g - sg / n - xh * sgx / n)
    return dx, dgamma, dbeta, dx.sum(axis=AX)


def relu_backward(dy, y, split=0):
    """-> dx, or (dx_lo, dx) = the first ``split`` channels and the rest."""
    d = np.where(f64(y) > 0.0, f64(dy), 0.0)
    return d if split == 0 else (d[..., :split], d[..., split:])


def _first_max_routes(x, dy):
    """dy [n,ceil(h/2),ceil(w/2),c] spread over x's [n,h,w,c] frame: each window's value at its first maximum of x in
    row-major order (taps past an odd edge are not in the window), zero elsewhere."""
    x, dy = f64(x), f64(dy)
    n, h, w, c = x.shape
    ph, pw = (h + 1) // 2, (w + 1) // 2
    assert dy.shape == (n, ph, pw, c)
    pad = np.full((n, 2 * ph, 2 * pw, c), -np.inf)
    pad[:, :h, :w] = x
    taps = pad.reshape(n, ph, 2, pw, 2, c).transpose(2, 4, 0, 1, 3, 5).reshape(4, n, ph, pw, c)  # k = 2*dy + dx
    first = np.argmax(taps, axis=0)  # the first maximum; a window's tap 0 is always inside the frame
    routed = np.where(first[None] == np.arange(4).reshape(4, 1, 1, 1, 1), dy[None], 0.0)
    out = routed.reshape(2, 2, n, ph, pw, c).transpose(2, 3, 0, 4, 1, 5).reshape(n, 2 * ph, 2 * pw, c)
    return out[:, :h, :w]


def maxpool_backward(x, dy, add=None):
    g = _first_max_routes(x, dy)
    return g if add is None else to_f32(g + f64(add))


def relu_backward_bias(dy, y, add=None, pool=False):
    """-> dz (the kernel's f32 value: dy + add is one f32 addition), dbias."""
    y = f64(y)
    g = _first_max_routes(y, dy) if pool else f64(dy)
    if add is not None:
        g = g + f64(add)
    dz = to_f32(np.where(y > 0.0, g, 0.0))
    return dz, dz.sum(axis=AX)


def softmax(x):
    x = f64(x)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def ulp32(a):
    """The spacing of f32 at |a| (of the smallest normal below it)."""
    a = np.maximum(np.abs(np.asarray(a, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 23)


def exact_ints(rs, shape):
    """Nonzero integers from {-4..-1, 1..4}: every channel sum of them (and of their squares) is exact in float64 and
    in the kernels' f64 partial sums, in any order."""
    v = rs.randint(1, 5, size=shape)
    return (v * (2 * rs.randint(0, 2, size=shape) - 1)).astype(np.float64)


def check_exact_precondition(a):
    a = f64(a)
    assert np.abs(a.sum(axis=AX)).max() < 2.0 ** 24 and (a * a).sum(axis=AX).max() < 2.0 ** 53

"""tests/lane_ref.py pinned on the CPU, so that tests/test_gpu_lanes.py can trust it: the closed-form BN backward
against float64 autograd, its SyncBN (count) form against the whole batch, the vectorised pool adjoints against the
loop forms of tests/test_gpu_small_train.py and test_relu_backward_bias, and the kernel's three-operation statistics
against the two-pass ones on the exact-sum data of the seam cases."""

import numpy as np
import pytest
import torch

import lane_ref as lr
from oracle import train_ref as tr
from test_gpu_small_train import _maxpool_bwd_ref

EPS = tr.BN_EPS


def _scaled(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.mark.parametrize("c", [1, 3, 20])
@pytest.mark.parametrize("mask", [False, True])
def test_bn_backward_closed_form_vs_autograd(c, mask):
    rs = np.random.RandomState(10 * c + mask)
    shape = (2, 5, 7, c)
    x = rs.normal(size=shape) * 3 + 1
    dy = rs.normal(size=shape)
    gamma, beta = rs.uniform(0.5, 1.5, c), rs.normal(size=c)
    bias = torch.zeros(c, dtype=torch.float64, requires_grad=True)  # a conv bias added before the BN
    xr, gr, br = (torch.tensor(v, requires_grad=True) for v in (x, gamma, beta))
    out = tr._bn(xr + bias, gr, br)
    if mask:
        out = torch.relu(out)
    (out * torch.from_numpy(dy)).sum().backward()
    mean, var = lr.bn_stats(x)
    y = lr.bn_apply(x, mean, var, gamma, beta, EPS, "relu") if mask else None
    dx, dgamma, dbeta, dbias = lr.bn_backward(x, dy, y, mean, var, gamma, EPS)
    assert _scaled(dx, xr.grad.numpy()) <= 1e-10
    assert _scaled(dgamma, gr.grad.numpy()) <= 1e-10
    assert _scaled(dbeta, br.grad.numpy()) <= 1e-10
    # BN removes the bias: its gradient is zero up to rounding, judged on dx's scale as the GPU test judges it
    assert np.abs(dbias - bias.grad.numpy()).max() <= 1e-10 * np.abs(dx).sum(axis=lr.AX).max()


@pytest.mark.parametrize("mask", [False, True])
def test_bn_backward_count_form_equals_whole_batch(mask):
    rs = np.random.RandomState(3 + mask)
    shape = (4, 5, 7, 6)
    x, dy = rs.normal(size=shape) * 2 - 1, rs.normal(size=shape)
    gamma = rs.uniform(0.5, 1.5, 6)
    y = np.maximum(rs.normal(size=shape), 0) if mask else None
    mean, var = lr.bn_stats(x)
    whole = lr.bn_backward(x, dy, y, mean, var, gamma, EPS)
    m_all = shape[0] * shape[1] * shape[2]
    halves = [slice(0, 1), slice(1, 4)]
    part = [lr.bn_backward(x[s], dy[s], None if y is None else y[s], mean, var, gamma, EPS) for s in halves]
    sums = (part[0][2] + part[1][2], part[0][1] + part[1][1])
    assert _scaled(sums[0], whole[2]) <= 1e-12 and _scaled(sums[1], whole[1]) <= 1e-12
    dx = np.concatenate([lr.bn_backward(x[s], dy[s], None if y is None else y[s], mean, var, gamma, EPS,
                                        count=m_all, sums=sums)[0] for s in halves], 0)
    assert _scaled(dx, whole[0]) <= 1e-12


def _relu_bias_loop(dy, y, add, pool):
    """The loop reference of tests/test_gpu_train.py::test_relu_backward_bias."""
    n, h, w, c = y.shape
    g = add.astype(np.float64).copy() if add is not None else np.zeros(y.shape)
    if pool:
        ph, pw = (h + 1) // 2, (w + 1) // 2
        for b_ in range(n):
            for i in range(ph):
                for j in range(pw):
                    win = [(2 * i + a, 2 * j + bb) for a in (0, 1) for bb in (0, 1) if 2 * i + a < h and 2 * j + bb < w]
                    for ch in range(c):
                        vals = [y[b_, r, q, ch] for r, q in win]
                        k = int(np.argmax(vals))  # first maximum
                        g[b_, win[k][0], win[k][1], ch] += dy[b_, i, j, ch]
    else:
        g += dy
    return np.where(y > 0, g, 0.0)


POOL_SHAPES = [(1, 1, 1, 3), (2, 7, 9, 5), (1, 5, 5, 2), (2, 1, 4, 3), (1, 6, 1, 4), (2, 8, 6, 3)]


def _tie_heavy(rs, shape):
    return np.maximum(rs.randint(-2, 4, size=shape), 0).astype(np.float64) * 0.5  # few levels, relu zeros


@pytest.mark.parametrize("shape", POOL_SHAPES)
@pytest.mark.parametrize("with_add", [False, True])
def test_maxpool_backward_vectorised_equals_loop(shape, with_add):
    n, h, w, c = shape
    rs = np.random.RandomState(h * w + c)
    x = _tie_heavy(rs, shape)
    # integer dy and add: both references then sum exactly, whatever their order
    dy = rs.randint(-8, 9, size=(n, (h + 1) // 2, (w + 1) // 2, c)).astype(np.float64)
    add = rs.randint(-8, 9, size=shape).astype(np.float64) if with_add else None
    assert np.array_equal(lr.maxpool_backward(x, dy, add), _maxpool_bwd_ref(x, dy, add))
    # every window's gradient lands exactly once
    assert np.array_equal(lr.maxpool_backward(x, dy).sum(axis=(1, 2)), dy.sum(axis=(1, 2)))


@pytest.mark.parametrize("shape", POOL_SHAPES)
@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("with_add", [False, True])
def test_relu_backward_bias_vectorised_equals_loop(shape, pool, with_add):
    n, h, w, c = shape
    rs = np.random.RandomState(h * w + c + pool)
    y = _tie_heavy(rs, shape)
    dshape = (n, (h + 1) // 2, (w + 1) // 2, c) if pool else shape
    dy = rs.randint(-8, 9, size=dshape).astype(np.float64)
    add = rs.randint(-8, 9, size=shape).astype(np.float64) if with_add else None
    dz, dbias = lr.relu_backward_bias(dy, y, add, pool)
    want = _relu_bias_loop(dy, y, add, pool)
    assert np.array_equal(dz, want)
    assert np.array_equal(dbias, want.sum(axis=lr.AX))


def test_relu_backward_and_split():
    rs = np.random.RandomState(0)
    dy, y = rs.normal(size=(2, 3, 4, 7)), np.maximum(rs.normal(size=(2, 3, 4, 7)), 0)
    d = lr.relu_backward(dy, y)
    assert np.array_equal(d, dy * (y > 0))
    lo, hi = lr.relu_backward(dy, y, split=3)
    assert np.array_equal(np.concatenate([lo, hi], -1), d) and lo.shape[-1] == 3


@pytest.mark.parametrize("shape", [(2, 7, 9, 5), (2, 57, 61, 3), (3, 129, 131, 2)])
def test_bn_stats_three_op_form_on_exact_data(shape):
    rs = np.random.RandomState(shape[1])
    x = lr.exact_ints(rs, shape)
    assert set(np.unique(x)) <= {-4.0, -3.0, -2.0, -1.0, 1.0, 2.0, 3.0, 4.0}
    lr.check_exact_precondition(x)
    (m2, v2), (m3, v3) = lr.bn_stats(x), lr.bn_stats_3op(x)
    assert np.all(np.abs(m3 - m2) <= 1e-12 * np.abs(m2))  # (both divide the same exact integer sum)
    assert np.all(np.abs(v3 - v2) <= 1e-12 * v2)


def test_bn_apply_defaults_softmax_and_bf16():
    rs = np.random.RandomState(1)
    x = rs.normal(size=(1, 2, 3, 4))
    assert np.array_equal(lr.bn_apply(x, None, None, None, None, 0.0), x)
    s = lr.softmax(x * 1e4)
    assert np.all(np.isfinite(s)) and np.abs(s.sum(-1) - 1).max() <= 1e-15
    assert np.array_equal(lr.softmax(np.full((1, 1, 2, 4), 3.0)), np.full((1, 1, 2, 4), 0.25))
    # ties to even: 1 + 2^-8 is halfway between 1 and 1 + 2^-7; 1 + 3 * 2^-8 between 1 + 2^-7 and 1 + 2^-6
    assert np.array_equal(lr.to_bf16([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -2.5]), [1.0, 1 + 2.0 ** -6, -2.5])
    assert lr.ulp32(1.0) == 2.0 ** -23 and lr.ulp32(3.0) == 2.0 ** -22

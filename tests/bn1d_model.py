"""A plain model of ias_bn1d_groups_forward / _backward (csrc/bn_kernels.hip) on CPU tensors, and the case table its tests
share (test_bn1d_model_cpu.py, test_bn1d_groups_gpu.py).

The operation: relu?(BatchNorm1d_train(z + lin_bias)) on G stacked groups of n rows of a [G n, F] matrix.  Every group is
normalised with its own batch statistics (mean, biased variance), the running statistics are updated group after group
(group 0 first, unbiased variance n / (n - 1)), the counter goes up by G.  A None argument means what NULL means in
include/ias_hip.h: lin_bias 0, weight 1, bias 0, running statistics / counter absent.

One function, two modes:
  dtype=torch.float64  the reference: every operation in fp64.
  dtype=torch.float32  the kernel's arithmetic: fp32 throughout, column sums in the kernel's order (thread ty of a feature
                       owns rows ty, ty + 8, ... and adds them in row order, the eight partial sums are added in index
                       order; the mean from sums shifted by the group's first row), the variance in a second pass around the fp32 mean.  It is evidence that an fp32
                       implementation of this design can hold the bounds below on the table's inputs, not a bit model
                       (the compiler may contract a multiply and an add the model keeps apart).
"""
import collections

import torch

ROW_THREADS = 8                     # BN1_RG: the threads that share a feature's rows
EPS, MOMENTUM, NBT_START = 1e-5, 0.1, 7

# The bounds of the 2-D kernels' test (test_fused_batchnorm_activation_matches_torch), against the fp64 mode on the same
# fp32 inputs: |got - ref| <= coeff * max(1, largest |reference element|); the running mean has an absolute bound
# (1e-5 of the largest column mean, 50).  g_lin_bias, the column sums of dx, is zero in exact arithmetic: its bound is
# absolute, on the scale of what is summed -- n times the largest |dx| of the reference (`scale` below).
COEFF = {"y": 2e-5, "save_mean": 2e-5, "save_invstd": 2e-5, "dx": 5e-5, "gw": 1e-4, "gb": 1e-4, "g_lin_bias": 1e-4,
         "running_var": 1e-5}
RUNNING_MEAN_BOUND = 1e-5 * 50


def bound(name, ref, scale=None):
    if name == "running_mean":
        return RUNNING_MEAN_BOUND
    return COEFF[name] * max(1.0, ref.abs().max().item() if scale is None else scale)


def lin_bias_scale(dx_ref, n):
    return n * dx_ref.abs().max().item()


def fraction_of_bound(name, got, ref, scale=None):
    """max |got - ref| as a fraction of the quantity's bound (<= 1: holds)."""
    return (got.double() - ref.double()).abs().max().item() / bound(name, ref.double(), scale)


Forward = collections.namedtuple("Forward", "y save_mean save_invstd running_mean running_var nbt")
Backward = collections.namedtuple("Backward", "dx gw gb g_lin_bias")


def _colsum(x, dtype):
    """Column sums of x [n, F]: exact-order fp64 sum, or the kernel's order in fp32."""
    if dtype == torch.float64:
        return x.sum(0)
    n, F = x.shape
    k = -(-n // ROW_THREADS)
    p = torch.zeros(k * ROW_THREADS, F, dtype=dtype)
    p[:n] = x
    p = p.view(k, ROW_THREADS, F)
    part = torch.zeros(ROW_THREADS, F, dtype=dtype)
    for i in range(k):
        part = part + p[i]
    s = part[0].clone()
    for t in range(1, ROW_THREADS):
        s = s + part[t]
    return s


def _opt(t, dtype):
    return None if t is None else t.to(dtype)


def _group_stats(x, n, eps, dtype):
    """x [n, F] -> centred rows, mean, biased variance, invstd."""
    inv_n = torch.tensor(1.0, dtype=dtype) / torch.tensor(float(n), dtype=dtype)
    if dtype == torch.float64:
        mean = _colsum(x, dtype) * inv_n
    else:
        mean = x[0] + _colsum(x - x[0], dtype) * inv_n        # the kernel sums x - K, K = the group's first row
    c = x - mean
    var = _colsum(c * c, dtype) * inv_n
    invstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=dtype))
    return c, mean, var, invstd


def forward(z, lin_bias, weight, bias, running_mean, running_var, nbt, G, n, eps, momentum, relu, dtype):
    F = z.shape[1]
    assert z.shape[0] == G * n
    z, lin_bias, weight, bias = z.to(dtype), _opt(lin_bias, dtype), _opt(weight, dtype), _opt(bias, dtype)
    rm, rv = _opt(running_mean, dtype), _opt(running_var, dtype)
    mom = torch.tensor(momentum, dtype=dtype)
    unbias = torch.tensor(float(n), dtype=dtype) / torch.tensor(float(n - 1), dtype=dtype)
    x = z if lin_bias is None else z + lin_bias
    y = torch.empty_like(x)
    save_mean, save_invstd = torch.empty(G, F, dtype=dtype), torch.empty(G, F, dtype=dtype)
    for g in range(G):
        c, mean, var, invstd = _group_stats(x[g * n:(g + 1) * n], n, eps, dtype)
        a = invstd if weight is None else invstd * weight
        v = c * a
        if bias is not None:
            v = v + bias
        y[g * n:(g + 1) * n] = torch.clamp_min(v, 0.0) if relu else v
        save_mean[g], save_invstd[g] = mean, invstd
        if rm is not None:
            rm = (1.0 - mom) * rm + mom * mean
        if rv is not None:
            rv = (1.0 - mom) * rv + mom * (var * unbias)
    return Forward(y, save_mean, save_invstd, rm, rv, None if nbt is None else int(nbt) + G)


def backward(z, lin_bias, weight, dy, mask, G, n, eps, dtype):
    """dy [G n, F] -> dx, gw, gb (sums over the groups in group order), g_lin_bias (column sums of dx).  `mask` [G n, F]
    (bool, or None without a ReLU) is where the ReLU let the value through: given, never derived here."""
    F = z.shape[1]
    z, lin_bias, weight, dy = z.to(dtype), _opt(lin_bias, dtype), _opt(weight, dtype), dy.to(dtype)
    inv_n = torch.tensor(1.0, dtype=dtype) / torch.tensor(float(n), dtype=dtype)
    x = z if lin_bias is None else z + lin_bias
    d_all = dy if mask is None else dy * mask.to(dtype)
    dx = torch.empty_like(x)
    gw, gb, glb = (torch.zeros(F, dtype=dtype) for _ in range(3))
    for g in range(G):
        rows = slice(g * n, (g + 1) * n)
        c, _, _, invstd = _group_stats(x[rows], n, eps, dtype)
        a = invstd if weight is None else invstd * weight
        xhat, d = c * invstd, d_all[rows]
        s1, s2 = _colsum(d, dtype), _colsum(d * xhat, dtype)
        v = a * (d - s1 * inv_n - xhat * (s2 * inv_n))
        dx[rows] = v
        gw, gb, glb = gw + s2, gb + s1, glb + _colsum(v, dtype)
    return Backward(dx, gw, gb, glb)


# ---- the case table: (G, n, F, relu, lin_bias present) ------------------------------------------------------------------
# n: 2, 3 (the smallest), 8 | 9 (one row per thread | a second row for thread 0), 127 | 128 | 129 (16 -> 32 rows per thread
# in registers), 255 | 256 | 257 (32 rows per thread -> rows re-read), 300.  Every boundary n (128, 129, 256, 257) with
# G = 1, G = 2 (two groups per pass at n <= 128) and an odd G >= 3; G = 4: the two-group pass loops twice.
# F: 1, 63, 65 (dead lanes in the only / the last workgroup), 64 (none), 130 (three workgroups).
CASES = [
    (1, 128, 65, 1, 1), (2, 128, 130, 1, 1), (3, 128, 63, 0, 0),
    (1, 129, 64, 0, 1), (2, 129, 65, 1, 0), (5, 129, 1, 1, 1),
    (1, 256, 130, 1, 0), (2, 256, 63, 0, 1), (3, 256, 65, 1, 1),
    (1, 257, 1, 1, 1), (2, 257, 64, 1, 1), (5, 257, 65, 0, 0),
    (1, 2, 65, 1, 1), (2, 2, 1, 0, 1), (3, 2, 130, 1, 0),
    (4, 3, 63, 1, 1), (1, 3, 64, 0, 0),
    (4, 8, 65, 1, 1), (5, 9, 130, 0, 1), (2, 9, 64, 1, 0),
    (4, 127, 130, 1, 1), (3, 127, 1, 0, 1),
    (4, 255, 65, 1, 0), (1, 255, 63, 1, 1),
    (5, 300, 130, 1, 1), (2, 300, 65, 0, 1), (4, 300, 64, 1, 0),
]
CASE_IDS = [f"G{G}-n{n}-F{F}-relu{relu}-lb{lb}" for G, n, F, relu, lb in CASES]

Inputs = collections.namedtuple("Inputs", "z lin_bias weight bias running_mean running_var nbt dy")
MIN_SPREAD = 0.5


def make_inputs(G, n, F, lin_bias, seed=0):
    """fp32 inputs of a case.  Columns as in test_fused_batchnorm_activation_matches_torch: randn * 2 + linspace(-5, 50, F)
    (means large against the spread), weight = rand + 0.5, bias = randn; running statistics away from their initial
    values, the counter starts at NBT_START.  For n = 2 and n = 3 a (group, column) whose standard deviation falls below
    MIN_SPREAD is redrawn: two nearly equal rows amplify the rounding of an fp32 mean near 50 (half an ulp, 2e-6) by
    invstd, and no fp32 BatchNorm holds the bounds there.  With a floor of 0.1 the fp32 mode above missed the dx bound
    5.3-fold at n = 2 (dx there is a difference of nearly equal terms times weight * invstd, so its error grows with
    1 / spread^2); with 0.5 it stays below a fifth of every bound."""
    gen = torch.Generator().manual_seed(1000 * G + 7 * n + F + 100003 * seed)
    r = torch.randn(G, n, F, generator=gen)
    if n <= 3:
        for _ in range(100):
            bad = r.std(dim=1, unbiased=False) * 2.0 < MIN_SPREAD          # [G, F]
            if not bool(bad.any()):
                break
            fresh = torch.randn(G, n, F, generator=gen)
            r = torch.where(bad.unsqueeze(1), fresh, r)
        assert not bool((r.std(dim=1, unbiased=False) * 2.0 < MIN_SPREAD).any())
    z = (r * 2.0 + torch.linspace(-5, 50, F)).reshape(G * n, F).contiguous()
    lb = torch.randn(F, generator=gen) * 0.5 if lin_bias else None
    weight, bias = torch.rand(F, generator=gen) + 0.5, torch.randn(F, generator=gen)
    running_mean = torch.randn(F, generator=gen) * 3.0 + 1.0
    running_var = torch.rand(F, generator=gen) * 2.0 + 0.25
    dy = torch.randn(G * n, F, generator=gen)
    return Inputs(z, lb, weight, bias, running_mean, running_var, NBT_START, dy)

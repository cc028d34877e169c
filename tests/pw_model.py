"""fp64 model and derived error bounds for the thin 1x1 convolutions of csrc/pointwise_kernels.hip, and the exact input sets
of their C-ABI tests.  CPU only, test infrastructure: the package does not use it.

With x [B,Cin,HW], an optional scale s [B,Cin], w [Cout,Cin] and the cotangent g [B,Cout,HW] (fp32, taken to fp64):
    y[b]  = W (x[b] * s[b])                      (s per input row)
    gx[b] = W^T g[b]                             (the gradient of the product x * s)
    gw    = sum_b g[b] (x[b] * s[b])^T

The bounds are derived, not measured.  u = 2^-24 is the unit roundoff of fp32 and gamma(n) = n u / (1 - n u) (n u < 1,
asserted) bounds the relative error of a value that went through n roundings.  A sum of n products accumulated in ANY
order carries, on the way of each term to the total, one rounding for the product and at most n - 1 for additions; an
FMA would halve that, but nothing here assumes the MFMA fuses: two roundings per term, 2 n, plus 2 to spare, so
    |got - ref| <= gamma(2 n + 2) A,      A = sum |terms|.
* forward and input gradient: n = K terms (Cin forward, Cout for the input gradient), A = |W| (|x| |s|) or |W|^T |g|.
  The scaled forward rounds x * s once more per term: gamma(3 K + 2).
* weight gradient: n = B HW terms (partial sums and their reduction are more of the same additions), T = the weight
  gradient of |g| and |x| |s|.  The scaled form multiplies a (sample, split) sum by s once: one more rounding on each
  term's way, gamma(2 B HW + 3).
Where a bound is 0 every term is 0 and the value must be exactly 0 (conv_model.ratio).

The weight gradient's bound is weak at large B HW (a dropped chunk of 64 positions stays far inside it), hence the exact
sets: small integers with power-of-two scales, exact in fp32 in any summation order, and one-hot weights on ramps."""
from collections import namedtuple

import torch

from conv_model import RAMP_MOD, U, ramp, ratio  # noqa: F401  (ratio, ramp: what the tests import from here)

Model = namedtuple("Model", "y gx gw y_bound gx_bound gw_bound")


def gamma(n):
    assert n * U < 1, n
    return n * U / (1 - n * U)


def _values(x, s, w, g):
    """y, gx, gw in the dtype of the inputs (fp64: the model; fp32: the same expressions as plain CPU arithmetic)."""
    B, K, HW = x.shape
    M = w.shape[0]
    assert tuple(w.shape) == (M, K) and tuple(g.shape) == (B, M, HW) and (s is None or tuple(s.shape) == (B, K))
    xs = x if s is None else x * s[:, :, None]
    y = torch.matmul(w, xs)
    gx = torch.matmul(w.t(), g)
    gw = torch.matmul(g.permute(1, 0, 2).reshape(M, B * HW), xs.permute(1, 0, 2).reshape(K, B * HW).t())
    return y, gx, gw


def values(x, s, w, g):
    """The three results alone, in fp64 (for the exact sets, which need no bound)."""
    return _values(x.double(), None if s is None else s.double(), w.double(), g.double())


def model(x, s, w, g):
    """x [B,Cin,HW], s [B,Cin] or None, w [Cout,Cin], g [B,Cout,HW] (fp32, CPU) -> Model of fp64 tensors: the three results
    and the bound on |got - ref| of each."""
    assert all(t.dtype == torch.float32 and t.device.type == "cpu" for t in (x, w, g) + (() if s is None else (s,)))
    B, K, HW = x.shape
    M = w.shape[0]
    y, gx, gw = values(x, s, w, g)
    A, Agx, T = values(x.abs(), None if s is None else s.abs(), w.abs(), g.abs())
    scaled = s is not None
    return Model(y, gx, gw, gamma((3 if scaled else 2) * K + 2) * A, gamma(2 * M + 2) * Agx,
                 gamma(2 * B * HW + (3 if scaled else 2)) * T)


def loops(x, s, w, g):
    """y, gx, gw by the literal triple-loop definition, in fp64 (tiny shapes only)."""
    x, w, g = x.double(), w.double(), g.double()
    B, K, HW = x.shape
    M = w.shape[0]
    s = torch.ones(B, K, dtype=torch.float64) if s is None else s.double()
    y, gx, gw = torch.zeros(B, M, HW, dtype=torch.float64), torch.zeros_like(x), torch.zeros_like(w)
    for b in range(B):
        for m in range(M):
            for k in range(K):
                for p in range(HW):
                    y[b, m, p] += w[m, k] * (x[b, k, p] * s[b, k])
                    gx[b, k, p] += w[m, k] * g[b, m, p]
                    gw[m, k] += g[b, m, p] * (x[b, k, p] * s[b, k])
    return y, gx, gw


# ---- input set (a): seeded randn, the scale in (0, 1]
def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def randn_inputs(shape, seed=301):
    """x, s, w, g of the case (B, Cin, Cout, HW)."""
    B, Cin, Cout, HW = shape
    return (torch.randn((B, Cin, HW), generator=_gen(seed)), 1.0 - torch.rand((B, Cin), generator=_gen(seed + 3)),
            torch.randn((Cout, Cin), generator=_gen(seed + 1)), torch.randn((B, Cout, HW), generator=_gen(seed + 2)))


# ---- input set (b): small integers, scales that are powers of two
def integer_inputs(shape, seed=401):
    """x, g uniform integers in [-4, 4], w in [-3, 3], s from {0.5, 1, 2}.  With the scale every term of the weight gradient
    is at most 4 * 4 * 2 = 16 * 2 in magnitude and every term of the forward 3 * 4 * 2 = 12 * 2, of the input gradient 12,
    all multiples of one half; asserted here: no sum of magnitudes reaches 2^24 halves, so every product, partial sum and
    total is exact in fp32 in any summation order, and all three results must equal the fp64 model bit for bit."""
    B, Cin, Cout, HW = shape
    assert integer_set_halves(shape) < 2 ** 24, shape
    x = torch.randint(-4, 5, (B, Cin, HW), generator=_gen(seed)).float()
    w = torch.randint(-3, 4, (Cout, Cin), generator=_gen(seed + 1)).float()
    g = torch.randint(-4, 5, (B, Cout, HW), generator=_gen(seed + 2)).float()
    s = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (B, Cin), generator=_gen(seed + 3))]
    return x, s, w, g


def integer_set_halves(shape):
    """The largest sum of magnitudes the integer set can give at this shape, in units of one half."""
    B, Cin, Cout, HW = shape
    return 2 * max(16 * 2 * B * HW, 12 * 2 * max(Cin, Cout))


# ---- input set (c): one-hot rows on ramps
ONE_HOT_OFFSETS = (0, 5)


def one_hot(Cout, Cin, offset):
    """w [Cout,Cin]: row m has a single 1 at column (7 m + offset) mod Cin."""
    w = torch.zeros(Cout, Cin)
    w[torch.arange(Cout), one_hot_columns(Cout, Cin, offset)] = 1.0
    return w


def one_hot_columns(Cout, Cin, offset):
    return (7 * torch.arange(Cout) + offset) % Cin


def one_hot_inputs(shape, offset):
    """x, w, g: ramps (integers below 4093) and the one-hot weight.  The forward is a row copy (times a power of two when
    scaled), the input gradient a sum of at most ceil(Cout / Cin) + 1 ramp rows: exact in fp32."""
    B, Cin, Cout, HW = shape
    assert RAMP_MOD * Cout < 2 ** 23
    return ramp((B, Cin, HW)), one_hot(Cout, Cin, offset), ramp((B, Cout, HW), 17)


def one_hot_results(x, s, g, Cin, offset):
    """y and gx of the one-hot weight without a matrix product: rows copied, rows added (fp64: exact)."""
    cols = one_hot_columns(g.shape[1], Cin, offset)
    xs = x.double() if s is None else x.double() * s.double()[:, :, None]
    gx = torch.zeros(x.shape, dtype=torch.float64)
    gx.index_add_(1, cols, g.double())
    return xs[:, cols, :], gx

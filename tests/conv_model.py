"""fp64 model and derived error bounds for the depthwise and stem convolutions of csrc/conv_kernels.hip.  CPU only, test
infrastructure: the package does not use it.

The reference is F.conv2d in fp64 (plus autograd for the two gradients) on CPU copies of the fp32 inputs: depthwise with
groups = C and padding (K - 1) // 2, the stem 3 -> 16 with K 3, stride 2, padding 1.

The bounds are derived, not measured.  u = 2^-24 is the unit roundoff of fp32.  A sum of n products accumulated with fused
multiply-adds in ANY order carries at most n roundings, each at most u times a partial sum, and every partial sum is at
most the sum of the terms' magnitudes:
    |got - ref| <= n u A (1 + O(n u)),      A = sum |terms|.
* forward and input gradient: n = K K taps; the bounds use K K + 1 (the stem: 27 + 1 = 28), the extra term covering the
  second-order part.  A is the same convolution (or its transpose) of |x| (or |g|) with |w|, in fp64.  Where A == 0 every
  term is zero and the value must be exactly 0.
* weight gradient: n = B Ho Wo positions per tap (partial sums and their reduction are more of the same additions), the
  factor 1.01 covers the second-order part (n u < 0.01 for n < 167 000; asserted).  T is the weight gradient of |x|, |g|."""
from collections import namedtuple

import torch
import torch.nn.functional as F

U = 2.0 ** -24

Model = namedtuple("Model", "y gx gw y_bound gx_bound gw_bound")


def out_size(n, K, S):
    return (n + 2 * ((K - 1) // 2) - K) // S + 1


def _conv_and_grads(x, w, g, S, groups):
    """fp64 conv2d of x with w (padding (K - 1) // 2) and its gradients for the cotangent g."""
    P = (w.shape[-1] - 1) // 2
    x, w = x.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
    y = F.conv2d(x, w, None, S, P, 1, groups)
    assert tuple(y.shape) == tuple(g.shape), (tuple(y.shape), tuple(g.shape))
    gx, gw = torch.autograd.grad(y, (x, w), g)
    return y.detach(), gx, gw


def model(x, w, g, S, groups):
    """x [B,Cin,H,W], w [Cout,Cin/groups,K,K], g [B,Cout,Ho,Wo] (fp32, CPU) -> Model of fp64 tensors: the three results and
    the bound on |got - ref| of each."""
    K = w.shape[-1]
    taps = w.shape[1] * K * K                      # products per output element: K K (depthwise), 27 (stem)
    y, gx, gw = _conv_and_grads(x.double(), w.double(), g.double(), S, groups)
    A, Agx, T = _conv_and_grads(x.double().abs(), w.double().abs(), g.double().abs(), S, groups)
    n = g.shape[0] * g.shape[2] * g.shape[3]
    assert n * U < 0.01, "the factor 1.01 of the weight gradient's bound assumes n u < 0.01"
    # (the input gradient sums at most K K taps per output channel; depthwise: one output channel per input channel)
    return Model(y, gx, gw, (taps + 1) * U * A, (K * K * (w.shape[0] // groups) + 1) * U * Agx, 1.01 * n * U * T)


def dw_model(x, w, g, S):
    return model(x, w, g, S, x.shape[1])


def stem_model(x, w, g):
    return model(x, w, g, 2, 1)


def ratio(got, ref, bound):
    """The largest |got - ref| / bound; inf where got is not finite, or where bound == 0 and got is not exactly 0."""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    zero = bound == 0
    if bool((got[zero] != 0).any()):
        return float("inf")
    err = (got - ref).abs()[~zero]
    return (err / bound[~zero]).max().item() if err.numel() else 0.0


# ---- input set (a): seeded randn
# shape -> seed, where the default's draw puts fp32 conv2d on the CPU (products and sums rounded separately: up to 3 roundings
# where the bound of two FMAs counts 2) above half a bound: the degenerate shapes, whose weight gradient has 1 .. 3 terms
SEEDS = {(2, 3, 2, 1, 5, 2): 131, (1, 1, 1, 1, 3, 1): 111, (1, 1, 1, 1, 5, 2): 111, (2, 1, 1): 461, (3, 2, 2): 211}


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator(device="cpu").manual_seed(seed))


def dw_inputs(shape):
    """x, w, g of the depthwise case (B, C, H, W, K, S)."""
    B, C, H, W, K, S = shape
    seed = SEEDS.get(shape, 101)
    return (_randn((B, C, H, W), seed), _randn((C, 1, K, K), seed + 1),
            _randn((B, C, out_size(H, K, S), out_size(W, K, S)), seed + 2))


def stem_inputs(shape):
    """x, w, g of the stem case (B, H, W)."""
    B, H, W = shape
    seed = SEEDS.get(shape, 201)
    return (_randn((B, 3, H, W), seed), _randn((16, 3, 3, 3), seed + 1),
            _randn((B, 16, out_size(H, 3, 2), out_size(W, 3, 2)), seed + 2))


# ---- the literal definition (tiny shapes only)
def loops(x, w, g, S, groups):
    """y, gx, gw by the nested-loop definition of a grouped, zero-padded, strided cross-correlation, in fp64."""
    x, w, g = x.double(), w.double(), g.double()
    B, Cin, H, W = x.shape
    Cout, cpg, K, _ = w.shape
    P, opg = (K - 1) // 2, Cout // groups
    Ho, Wo = g.shape[2], g.shape[3]
    y, gx, gw = torch.zeros(B, Cout, Ho, Wo, dtype=torch.float64), torch.zeros_like(x), torch.zeros_like(w)
    for b in range(B):
        for co in range(Cout):
            for ho in range(Ho):
                for wo in range(Wo):
                    for cl in range(cpg):
                        ci = (co // opg) * cpg + cl
                        for kh in range(K):
                            for kw in range(K):
                                hi, wi = ho * S + kh - P, wo * S + kw - P
                                if 0 <= hi < H and 0 <= wi < W:
                                    y[b, co, ho, wo] += w[co, cl, kh, kw] * x[b, ci, hi, wi]
                                    gx[b, ci, hi, wi] += w[co, cl, kh, kw] * g[b, co, ho, wo]
                                    gw[co, cl, kh, kw] += x[b, ci, hi, wi] * g[b, co, ho, wo]
    return y, gx, gw


# ---- the exact input sets
RAMP_MOD = 4093     # prime, below 2^12: rows, planes and samples of a ramp never line up


def ramp(shape, start=0):
    """fp32 integers (start + flat index) mod 4093."""
    n = 1
    for d in shape:
        n *= d
    return ((torch.arange(n, dtype=torch.int64) + start) % RAMP_MOD).to(torch.float32).view(shape)


def one_hot_dw(C, K, offset):
    """w [C,1,K,K]: channel c has a single 1 at tap (c + offset) mod K K."""
    w = torch.zeros(C, K * K)
    w[torch.arange(C), (torch.arange(C) + offset) % (K * K)] = 1.0
    return w.view(C, 1, K, K)


def one_hot_stem(offset):
    """w [16,3,3,3]: output channel co has a single 1 at tap (co + offset) mod 27 of the 27 (ci, kh, kw)."""
    w = torch.zeros(16, 27)
    w[torch.arange(16), (torch.arange(16) + offset) % 27] = 1.0
    return w.view(16, 3, 3, 3)


def _tap_windows(H, W, Ho, Wo, K, S, kh, kw):
    """The output positions whose tap (kh, kw) falls inside the image, as slices (output rows, output columns, input rows,
    input columns), or None where there are none."""
    P = (K - 1) // 2

    def axis(n, no, k):
        lo = max(0, -((k - P) // S))                       # first o with o S + k - P >= 0
        hi = min(no - 1, (n - 1 - k + P) // S)             # last o with o S + k - P <= n - 1
        if hi < lo:
            return None
        return slice(lo, hi + 1), slice(lo * S + k - P, hi * S + k - P + 1, S)
    a, b = axis(H, Ho, kh), axis(W, Wo, kw)
    return None if a is None or b is None else (a[0], b[0], a[1], b[1])


def shift_forward(x, taps, K, S):
    """The forward of one-hot weights by copying: out[b, co] = channel taps[co][0] of x shifted by tap (kh, kw), zero outside
    the image.  taps: per output channel (input channel, kh, kw).  fp32, no arithmetic."""
    B, _, H, W = x.shape
    Ho, Wo = out_size(H, K, S), out_size(W, K, S)
    out = torch.zeros(B, len(taps), Ho, Wo, dtype=x.dtype)
    for co, (ci, kh, kw) in enumerate(taps):
        win = _tap_windows(H, W, Ho, Wo, K, S, kh, kw)
        if win is not None:
            out[:, co, win[0], win[1]] = x[:, ci, win[2], win[3]]
    return out


def shift_backward(g, taps, K, S, H, W):
    """The depthwise input gradient of one-hot weights by copying (one output channel per input channel): gx[b, c] = g[b, c]
    placed at the tap's input positions, zero elsewhere."""
    B, C, Ho, Wo = g.shape
    gx = torch.zeros(B, C, H, W, dtype=g.dtype)
    for co, (ci, kh, kw) in enumerate(taps):
        win = _tap_windows(H, W, Ho, Wo, K, S, kh, kw)
        if win is not None:
            gx[:, ci, win[2], win[3]] = g[:, co, win[0], win[1]]
    return gx


def dw_taps(C, K, offset):
    return [(c, ((c + offset) % (K * K)) // K, ((c + offset) % (K * K)) % K) for c in range(C)]


def stem_taps(offset):
    return [(((co + offset) % 27) // 9, (((co + offset) % 27) % 9) // 3, ((co + offset) % 27) % 3) for co in range(16)]


def tap_counts(H, W, K, S):
    """counts [Ho, Wo]: in-range taps of each output position; valid [K, K]: output positions at which each tap is in
    range.  fp64 integers: what all-ones inputs give (per input channel and sample)."""
    Ho, Wo = out_size(H, K, S), out_size(W, K, S)
    counts, valid = torch.zeros(Ho, Wo, dtype=torch.float64), torch.zeros(K, K, dtype=torch.float64)
    for kh in range(K):
        for kw in range(K):
            win = _tap_windows(H, W, Ho, Wo, K, S, kh, kw)
            if win is not None:
                counts[win[0], win[1]] += 1
                valid[kh, kw] = counts[win[0], win[1]].numel()
    return counts, valid

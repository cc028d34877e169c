"""The fp64 formulation of the squeeze-excitation gate's two 1x1 convolutions (ias_se_mlp_forward / _backward,
csrc/se_kernels.hip; the one test_squeeze_excitation_matches_torch writes with torch ops) on CPU tensors, and the shapes
and inputs test_se_mlp_gpu.py runs -- checked on the CPU by test_se_mlp_model_cpu.py.

  forward   h = relu(pooled w1^T + b1) [B, Cs],  z = h w2^T + b2 [B, C],  s = hardsigmoid(z) = clamp(z + 3, 0, 6) / 6
  backward  gz = gs / 6 where -3 < z < 3,  gh = (gz w2) where h > 0,  gp = gh w1,
            gw2 = gz^T h,  gb2 = colsum gz,  gw1 = gh^T pooled,  gb1 = colsum gh
The backward takes z and h as arguments (the C entry does): the masks are read from the arrays it is given.
"""
import collections
import math

import torch

# (B, C, Cs): why
SHAPES = [
    (1, 8, 8),            # one sample: the pair kernels' second slot is empty
    (3, 10, 6),           # scalar forms (C, Cs not multiples of 4), an odd batch
    (2, 96, 24),          # vectorised forms, one second-layer slice
    (2, 960, 240),        # pair backward at 71 KB of LDS
    (3, 1024, 1024),      # pair backward at its cap, 82 KB
    (2, 1028, 260),       # just past the cap: the per-sample backward
    (2, 8192, 64),        # forward at 66 KB of LDS, 64 second-layer slices
    (2, 12224, 64),       # forward at the ABI's limit C + Cs = 12288, 98 KB
]
VARIANT_SHAPES = [(2, 96, 24), (2, 960, 240)]       # also run with NULL biases and with weights 4 bytes off alignment
SEEDS = {(1, 8, 8): 8}                              # (eight gate elements: a draw that has some in every region)
SHAPE_IDS = [f"B{B}-C{C}-Cs{Cs}" for B, C, Cs in SHAPES]
H_BOUND, GRAD_BOUND = 1e-5, 1e-4          # x max(1, largest |reference element|): h, z, s | gp and the parameter gradients

Inputs = collections.namedtuple("Inputs", "pooled w1 b1 w2 b2 gs")
Forward = collections.namedtuple("Forward", "h z s")
Backward = collections.namedtuple("Backward", "gz gh gp gw1 gb1 gw2 gb2")

W2_FACTOR = 5.0     # z = h w2^T + b2 gets a standard deviation of about 3.5: all three regions of the hard sigmoid


def make_inputs(B, C, Cs, seed=None):
    """Weights randn / sqrt(fan_in), the second layer's times W2_FACTOR so that the gate's pre-activation values fall on
    both saturated sides of the hard sigmoid and between them; half of the hidden units are shut by the ReLU."""
    seed = SEEDS.get((B, C, Cs), 0) if seed is None else seed
    gen = torch.Generator().manual_seed(31 * C + 7 * Cs + B + 100003 * seed)
    pooled = torch.randn(B, C, generator=gen)
    w1 = torch.randn(Cs, C, generator=gen) / math.sqrt(C)
    b1 = torch.randn(Cs, generator=gen) * 0.5
    w2 = torch.randn(C, Cs, generator=gen) * (W2_FACTOR / math.sqrt(Cs))
    b2 = torch.randn(C, generator=gen)
    gs = torch.randn(B, C, generator=gen)
    return Inputs(pooled, w1, b1, w2, b2, gs)


def forward(pooled, w1, b1, w2, b2):
    p, w1, w2 = pooled.double(), w1.double(), w2.double()
    pre = p @ w1.t()
    if b1 is not None:
        pre = pre + b1.double()
    h = torch.clamp_min(pre, 0.0)
    z = h @ w2.t()
    if b2 is not None:
        z = z + b2.double()
    return Forward(h, z, torch.clamp(z + 3.0, 0.0, 6.0) / 6.0)


def backward(gs, z, h, pooled, w1, w2):
    gs, z, h, p, w1, w2 = (t.double() for t in (gs, z, h, pooled, w1, w2))
    gz = torch.where((z > -3.0) & (z < 3.0), gs / 6.0, torch.zeros_like(gs))
    gh = torch.where(h > 0.0, gz @ w2, torch.zeros_like(h))
    return Backward(gz, gh, gh @ w1, gh.t() @ p, gh.sum(0), gz.t() @ h, gz.sum(0))


def region_shares(fw):
    """Shares of the gate elements below, inside and above the hard sigmoid's linear piece, and of the hidden units the
    ReLU passes / shuts."""
    z, h = fw.z, fw.h
    return {"z<-3": (z < -3).double().mean().item(), "|z|<3": (z.abs() < 3).double().mean().item(),
            "z>3": (z > 3).double().mean().item(), "h>0": (h > 0).double().mean().item(), "h=0": (h == 0).double().mean().item()}


MIN_SHARE = {"z<-3": 0.05, "|z|<3": 0.05, "z>3": 0.05, "h>0": 0.20, "h=0": 0.20}

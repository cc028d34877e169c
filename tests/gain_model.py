"""The fp64 model of the output-gain contract (include/ias_hip_gain.h): the gain law, ias_gain_apply, ias_gain_backward,
ias_gain_solve, and the scalar model of the gain-only descent of tests/test_gain_gpu.py.  numpy / torch on the CPU."""
import math

import numpy as np
import torch

LO, HI = -60.0, 20.0
CHUNK = 8192                                         # IAS_GAIN_CHUNK
K = (math.log(10.0) / 20.0) * (HI - LO)              # d ln A / d g01
UNITY01 = 0.75


def db_of(g01):
    """fp32 g01 -> dB in fp64, as the kernels form it."""
    return LO + (HI - LO) * np.asarray(g01, dtype=np.float32).astype(np.float64)


def amplitude(g01):
    """fp32 g01 [B] -> A [B] fp64 (not rounded to fp32)."""
    return 10.0 ** (db_of(g01) / 20.0)


def _row_sums(a, b):
    """The exact row sums of a b for fp32 arrays [B, T] (math.fsum of the exact fp64 products) -> fp64 [B]; NaN / inf
    follow IEEE."""
    prod = a.astype(np.float64) * b.astype(np.float64)
    out = np.empty(prod.shape[0])
    for r, row in enumerate(prod):
        out[r] = math.fsum(row.tolist()) if np.isfinite(row).all() else row.sum()
    return out


def apply(audio, g01):
    """-> A_b audio[b] in fp64 (the device rounds A to fp32 and then the product: 2^-22 relative in all)."""
    return amplitude(g01)[:, None] * audio.astype(np.float64)


def backward(g_out, audio, g01):
    """-> (g_audio [B, T] fp64, g_gain01 [B] fp64, sum |g_out audio| [B] for the bound of D_b)."""
    A = amplitude(g01)
    D = _row_sums(g_out, audio)
    mag = np.abs(g_out.astype(np.float64) * audio.astype(np.float64)).sum(axis=1)
    return A[:, None] * g_out.astype(np.float64), D * A * K, mag


def solve(target, render):
    """-> (g01 [B] fp32, dB [B] fp64 before g01's rounding)."""
    et, er = _row_sums(target, target), _row_sums(render, render)
    db = np.zeros(et.shape[0])
    ok = np.isfinite(et) & np.isfinite(er) & (et > 0) & (er > 0)
    with np.errstate(divide="ignore", over="ignore"):
        db[ok] = np.clip(10.0 * np.log10(et[ok] / er[ok]), LO, HI)
    return ((db - LO) / (HI - LO)).astype(np.float32), db


class ApplyGain(torch.autograd.Function):
    """The model as an autograd function in fp64 (A is not rounded to fp32 here: a rounded A is a step function of g01),
    with the backward of the contract written out, for torch.autograd.gradcheck."""

    @staticmethod
    def forward(ctx, audio, g01):
        A = 10.0 ** ((LO + (HI - LO) * g01) / 20.0)
        ctx.save_for_backward(audio, A)
        return A.unsqueeze(1) * audio

    @staticmethod
    def backward(ctx, g_out):
        audio, A = ctx.saved_tensors
        return A.unsqueeze(1) * g_out, (g_out * audio).sum(dim=1) * A * K


def gain_only_descent(true_db, init_db=0.0, steps=50, lr=0.02, betas=(0.9, 0.999), eps=1e-8, level=1.0):
    """The matcher's fit with every Voice column frozen at the target's and the gain alone free, against a target that is
    10^(true_db / 20) x the render, under a mel POWER loss: the loss is exactly |a^2 - c| level with c = 10^(true_db / 10)
    and level = mean(M) of the render's mel, so the fit is a scalar Adam run on g01 (clamped to 0 .. 1, best-so-far over
    the iterates and the last value).  -> (best / initial loss, the best gain in dB)."""
    c = 10.0 ** (true_db / 10.0)
    g = (init_db - LO) / (HI - LO)
    m = v = 0.0
    best, best_db, first = math.inf, None, None

    def loss_grad(g):
        a2 = 10.0 ** ((LO + (HI - LO) * g) / 10.0)
        return abs(a2 - c) * level, math.copysign(1.0, a2 - c) * a2 * 2.0 * K * level

    for t in range(1, steps + 2):
        loss, grad = loss_grad(g)
        first = loss if first is None else first
        if loss < best:
            best, best_db = loss, LO + (HI - LO) * g
        if t > steps:
            break
        m = betas[0] * m + (1 - betas[0]) * grad
        v = betas[1] * v + (1 - betas[1]) * grad * grad
        denom = math.sqrt(v) / math.sqrt(1 - betas[1] ** t) + eps
        g = min(max(g - lr / (1 - betas[0] ** t) * m / denom, 0.0), 1.0)
    return best / first, best_db

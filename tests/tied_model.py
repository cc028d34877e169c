"""fp64 numpy restatement of the contract of ias_match_tied_step (include/ias_hip_tied.h), written from its text and not
from the kernel, and the states its tests start from.

The hyperparameters are rounded to fp32 first, as the entry point receives them (``_rule_fp64`` of
tests/test_match_gpu.py does the same: 1 - fp32(0.999) differs from 0.001 by 1.3e-5 relative).  Everything else is fp64:
the model does not round the mean gradient of a tied column to fp32 as the kernel does, so it differs from the kernel by
the kernel's fp32 roundings alone."""
import numpy as np


def f32(x):
    return float(np.float32(x))


def state(N, P, G, seed=0):
    """dict of numpy arrays: params01 in 0.2 .. 0.8, zero moments, best_loss +inf, counters 0 (``_state`` of
    tests/test_match_gpu.py for N rows in G groups)."""
    rng = np.random.default_rng(seed)
    p = (0.2 + 0.6 * rng.random((N, P))).astype(np.float32)
    return {"params01": p, "m": np.zeros((N, P), np.float32), "v": np.zeros((N, P), np.float32),
            "best_params": p.copy(), "step": np.zeros(G, np.int32), "skipped": np.zeros(G, np.int32),
            "best_loss": np.full(G, np.inf, np.float64), "group_loss": np.zeros(G, np.float64)}


def as_fp64(st):
    return {k: (a.astype(np.float64) if a.dtype.kind == "f" else a.copy()) for k, a in st.items()}


def tied_step(st, grad, loss, group_start, free, tied, active, update=1, lr=0.01, betas=(0.9, 0.999), eps=1e-8):
    """One ias_match_tied_step on ``st`` (fp64 arrays of ``as_fp64``, in place).  grad [N, P], loss [N]: the fp32 values
    the kernel gets, as fp64."""
    b1, b2, lr, eps = f32(betas[0]), f32(betas[1]), f32(lr), f32(eps)
    grad = np.asarray(grad, dtype=np.float64)
    loss = np.asarray(loss, dtype=np.float64)
    free = np.asarray(free) != 0
    tied = (np.asarray(tied) != 0) & free
    own = free & ~tied
    for g in range(len(group_start) - 1):
        r0, r1 = int(group_start[g]), int(group_start[g + 1])
        n = r1 - r0
        if not active[g] or n < 1:
            continue
        rows = slice(r0, r1)
        s = np.float64(0.0)
        for r in range(r0, r1):                                       # row order
            s = loss[r] if r == r0 else s + loss[r]
        L = s / np.float64(n)
        st["group_loss"][g] = L
        if np.isfinite(L) and L < st["best_loss"][g]:                 # strict; the pre-update parameters
            st["best_params"][rows] = st["params01"][rows]
            st["best_loss"][g] = L
        if not update:
            continue
        if not np.isfinite(loss[rows]).all() or not np.isfinite(grad[rows][:, free]).all():
            st["skipped"][g] += 1
            continue
        st["step"][g] += 1
        t = int(st["step"][g])
        step_size = lr / (1.0 - b1 ** t)
        bc2_sqrt = (1.0 - b2 ** t) ** 0.5

        def adam(p, m, v, gr):
            m = b1 * m + (1.0 - b1) * gr
            v = b2 * v + (1.0 - b2) * gr * gr
            return np.clip(p - step_size * m / (np.sqrt(v) / bc2_sqrt + eps), 0.0, 1.0), m, v

        gsum = np.zeros(grad.shape[1])
        for r in range(r0, r1):
            gsum = grad[r].copy() if r == r0 else gsum + grad[r]
        gbar = gsum / np.float64(n)
        p, m, v = adam(st["params01"][r0, tied], st["m"][r0, tied], st["v"][r0, tied], gbar[tied])
        for r in range(r0, r1):                                       # one update, written to every row
            st["params01"][r, tied], st["m"][r, tied], st["v"][r, tied] = p, m, v
        for r in range(r0, r1):                                       # own columns: the row's gradient, not divided by n
            p, m, v = adam(st["params01"][r, own], st["m"][r, own], st["v"][r, own], grad[r, own])
            st["params01"][r, own], st["m"][r, own], st["v"][r, own] = p, m, v
    return st

#!/usr/bin/env python3
"""Records the bits of the matcher's two optimiser steps (ias_match_adam_step, ias_match_tied_step) on fixed inputs:

    python scripts/match_step_bits.py [--out tests/golden/match_step_bits.npz]

tests/test_match_step_bits_gpu.py replays the same inputs (``replay`` below) and asserts equality with the committed file,
which was written by this script on an MI355X at the commit before the two kernels came to share one Adam update.  Rerun
it only where a change of those bits is meant.  The inputs are those of tests/test_tied_gpu.py:

* ``singleton``: N = 7 rows, one per group, six iterations at lr 0.02, betas (0.8, 0.99), eps 1e-7, with a NaN gradient in
  a free column, inf in a frozen one, a NaN loss and one inactive row, through both entries (``adam_*``, ``tied_*``);
* ``groups``: N = 11 rows in groups of 1, 4, 1 and 5 with own, tied and frozen columns and one inactive group, five
  iterations at the default hyperparameters, through the tied entry."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ARRAYS = ("params01", "m", "v", "best_params", "step", "skipped", "best_loss", "group_loss")
P = 78
FROZEN = [5, 17, 40, 77]
OWN = [0, 1, 30]


def _state(N, G, seed, dev):
    import torch
    p = (0.2 + 0.6 * np.random.default_rng(seed).random((N, P))).astype(np.float32)
    st = {"params01": p, "m": np.zeros((N, P), np.float32), "v": np.zeros((N, P), np.float32), "best_params": p.copy(),
          "step": np.zeros(G, np.int32), "skipped": np.zeros(G, np.int32), "best_loss": np.full(G, np.inf, np.float64),
          "group_loss": np.zeros(G, np.float64)}
    return {k: torch.from_numpy(a).to(dev) for k, a in st.items()}


def _inputs(N, seed, iters):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((N, P)).astype(np.float32),
             (rng.random(N) + (0.0 if it % 2 == 0 else 1.0)).astype(np.float32)) for it in range(iters)]


def replay(dev):
    """-> {"<case>_<entry>_<array>": numpy array}: the state of every case after its last iteration."""
    import torch
    from inverse_audio_synthesis_amd.match import match_adam_step, tied_adam_step
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    free = np.ones(P, np.uint8)
    free[FROZEN] = 0
    tied = np.ones(P, np.uint8)
    tied[OWN] = 0
    free, tied = t(free), t(tied)

    def tied_step(st, grad, loss, group_start, active, lr=0.01, betas=(0.9, 0.999), eps=1e-8):
        tied_adam_step(st["params01"], t(grad), st["m"], st["v"], st["best_params"], t(loss),
                       t(np.asarray(group_start, np.int32)), st["step"], st["skipped"], st["best_loss"], st["group_loss"],
                       free, tied, t(np.asarray(active, np.uint8)), 1, lr, betas, eps)

    out = {}
    N = 7
    active = np.array([1, 1, 1, 0, 1, 1, 1], np.uint8)
    a, b = _state(N, N, 3, dev), _state(N, N, 3, dev)
    hyper = dict(lr=0.02, betas=(0.8, 0.99), eps=1e-7)
    for it, (grad, loss) in enumerate(_inputs(N, 4, 6)):
        if it in (1, 4):
            grad[1, 10], grad[2, FROZEN[0]], loss[5] = np.nan, np.inf, np.nan
        tied_step(a, grad, loss, np.arange(N + 1), active, **hyper)
        match_adam_step(b["params01"], t(grad), b["m"], b["v"], b["step"], t(loss), b["best_loss"], b["best_params"], free,
                        t(active), b["skipped"], hyper["lr"], hyper["betas"], hyper["eps"])
    out.update({f"singleton_tied_{k}": a[k].cpu().numpy() for k in ARRAYS})
    out.update({f"singleton_adam_{k}": b[k].cpu().numpy() for k in ARRAYS[:-1]})      # the untied entry has no group_loss

    sizes = (1, 4, 1, 5)
    N = sum(sizes)
    st = _state(N, len(sizes), 1, dev)
    for grad, loss in _inputs(N, 2, 5):
        tied_step(st, grad, loss, np.concatenate([[0], np.cumsum(sizes)]), [1, 1, 0, 1])
    out.update({f"groups_tied_{k}": st[k].cpu().numpy() for k in ARRAYS})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "match_step_bits.npz"))
    args = ap.parse_args()
    import torch
    arrays = replay(torch.device("cuda:0"))
    np.savez(args.out, **arrays)
    print(f"{args.out}: {len(arrays)} arrays, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The descent of tests/test_gain_gpu.py::test_matcher_mixer_levels_with_and_without_gain on the CPU, through the oracle's
render in fp64 and torch.optim.Adam: four sounds whose target is 0.125 x their own render (18 dB down), the three mixer
levels free and started at 0.5, 50 steps at lr 0.02, once with a fitted output gain per sound (started at the closed-form
energy ratio of the target against the start's render, as ``match.solve_gain``) and once without.  For which seeds does
the gained fit at least halve every sound's mel L1, and end below the fit without a gain for every sound?  No GPU, no
project kernel.

    python scripts/gain_oracle_descent.py [SEED ...]

Prints, per seed and sound, best / initial loss with the gain (both relative to the gained start) and the best loss with
the gain over the best loss without it (the best-so-far of the 50 iterates and the last parameters, as ``fit`` keeps it)."""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import spectral_oracle as spo   # noqa: E402
from oracle import synth_oracle as so       # noqa: E402
from oracle import synth_spec as S          # noqa: E402

MEL = dict(sample_rate=16000, n_fft=1024, hop_length=512, n_mels=128, power=2.0)
LO, HI = -60.0, 20.0                         # the gain law of include/ias_hip_gain.h
SCALE = 0.125


def descend(seed, with_gain, steps=50, lr=0.02):
    """-> (initial loss [4], best loss [4]) of the four sounds of the oracle's batch ``seed``."""
    cfg = so.VoiceConfig(4, 16000, 1.0)
    noise = so.make_noise(cfg).double()
    tp = so.sample_params01(cfg, seed).double()
    cols = [S.INDEX[("mixer", n)] for n in ("vco_1", "vco_2", "noise")]
    target = SCALE * so.render_from_params01(cfg, tp, noise, "f64")
    tmel = spo.mel_spectrogram(target, **MEL)

    def render(w):
        p = tp.clone()
        p[:, cols] = w
        return so.render_from_params01(cfg, p, noise, "f64")

    w = torch.nn.Parameter(torch.full((4, 3), 0.5, dtype=torch.float64))
    free = [w]
    g = None
    if with_gain:
        with torch.no_grad():
            start = render(w)
            db = 10.0 * torch.log10((target ** 2).sum(1) / (start ** 2).sum(1))
        g = torch.nn.Parameter(((db.clamp(LO, HI) - LO) / (HI - LO)).float().double())      # g01 is stored in fp32
        free.append(g)

    def losses():
        audio = render(w)
        if g is not None:
            audio = audio * (10.0 ** ((LO + (HI - LO) * g) / 20.0)).unsqueeze(1)
        return (spo.mel_spectrogram(audio, **MEL) - tmel).abs().mean(dim=(1, 2))

    # one Adam over the sum of the per-sound losses: Adam is elementwise and a sound's loss depends on its own row alone
    opt = torch.optim.Adam(free, lr=lr, betas=(0.9, 0.999), eps=1e-8)
    history = []
    for _ in range(steps):
        opt.zero_grad()
        rows = losses()
        rows.sum().backward()
        history.append(rows.detach().clone())
        opt.step()
        with torch.no_grad():
            for t in free:
                t.clamp_(0.0, 1.0)
    with torch.no_grad():
        history.append(losses())
    history = torch.stack(history)
    return history[0], history.min(dim=0)[0]


if __name__ == "__main__":
    fmt = lambda t: "[" + ", ".join(f"{x:.4f}" for x in t.tolist()) + "]"     # noqa: E731
    for seed in [int(a) for a in sys.argv[1:]] or range(8):
        gi, gb = descend(seed, True)
        pi, pb = descend(seed, False)
        ok = bool((gb / gi <= 0.5).all() and (gb < pb).all())
        print(f"seed {seed}: with gain best / initial {fmt(gb / gi)}; without {fmt(pb / pi)}; "
              f"best with / best without {fmt(gb / pb)}; initial with / without {fmt(gi / pi)}"
              f"{'' if ok else '   (a condition fails)'}", flush=True)

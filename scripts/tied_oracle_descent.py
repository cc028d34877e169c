#!/usr/bin/env python3
"""The tied descent of tests/test_tied_gpu.py::test_fit_tied_descends_on_shared_mixer_levels on the CPU, through the
oracle's render in fp64 and torch.optim.Adam on the group's mean loss: which preset seeds let a shared set of mixer levels
at least halve the mean mel L1 of three notes in 50 steps at lr 0.02?  No GPU, no project kernel.

    python scripts/tied_oracle_descent.py [SEED ...]

Prints, per seed, best / initial mean loss (the best-so-far of the 50 iterates and the last parameters, as fit_tied keeps
it)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import spectral_oracle as spo   # noqa: E402
from oracle import synth_oracle as so       # noqa: E402
from oracle import synth_spec as S          # noqa: E402

MIDI01 = (0.35, 0.45, 0.55)                  # keyboard.midi_f0 of the three notes, in 0..1 (MIDI 44.45, 57.15, 69.85)
MEL = dict(sample_rate=16000, n_fft=1024, hop_length=512, n_mels=128, power=2.0)


def phrase_params(seed):
    """[3, 78] fp32: row 0 of the oracle's batch ``seed`` at the three notes."""
    tp = so.sample_params01(so.VoiceConfig(4, 16000, 1.0), seed)[:1].repeat(3, 1)
    tp[:, S.INDEX[("keyboard", "midi_f0")]] = torch.tensor(MIDI01)
    return tp


def descend(seed, steps=50, lr=0.02):
    cfg = so.VoiceConfig(3, 16000, 1.0)
    noise = so.make_noise(so.VoiceConfig(4, 16000, 1.0))[:3].double()     # the rows sit at positions 0..2 of a batch of 4
    tp = phrase_params(seed).double()
    cols = [S.INDEX[("mixer", n)] for n in ("vco_1", "vco_2", "noise")]
    target = so.render_from_params01(cfg, tp, noise, "f64")
    tmel = spo.mel_spectrogram(target, **MEL)

    def group_loss(w):
        p = tp.clone()
        p[:, cols] = w.unsqueeze(0).expand(3, 3)
        mel = spo.mel_spectrogram(so.render_from_params01(cfg, p, noise, "f64"), **MEL)
        return (mel - tmel).abs().mean(dim=(1, 2)).mean()

    w = torch.nn.Parameter(torch.full((3,), 0.5, dtype=torch.float64))
    opt = torch.optim.Adam([w], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = group_loss(w)
        loss.backward()
        losses.append(float(loss.detach()))
        opt.step()
        with torch.no_grad():
            w.clamp_(0.0, 1.0)
    with torch.no_grad():
        losses.append(float(group_loss(w)))
    return min(losses) / losses[0], losses[0]


if __name__ == "__main__":
    for seed in [int(a) for a in sys.argv[1:]] or range(8):
        ratio, first = descend(seed)
        print(f"seed {seed}: initial mean mel-L1 {first:.6g}, best / initial = {ratio:.4f}")

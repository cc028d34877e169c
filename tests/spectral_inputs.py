"""Deterministic audio for the spectral tests, and the mel shapes that test_mel_shapes_cpu.py and test_mel_shapes_gpu.py
share (plain module: no fixtures).  Both generators return fp32 [B, T] on the host."""
import math

import torch

from helpers import randn

ROW_SCALES = (1.0, 1e-3, 0.3)


def noise(B, T, seed):
    """White noise of standard deviation 0.3: a flat spectrum, so under slaney normalisation every mel band is live and
    within an order of magnitude of the spectrogram's maximum."""
    return (randn((B, T), seed) * 0.3).contiguous()


def tones(B, T, rate, seed, noise=0.1):
    """Three sines per row (the construction of test_fft_forms_gpu._audio with the frequencies tied to the rate:
    0.005 rate (b + 1), 0.04 rate + 37 b, 0.2 rate - 500 b at amplitudes 0.3, 0.2, 0.1) plus Gaussian noise of the given
    amplitude; the batch is normalised to peak 0.9, then the rows are scaled by 1, 1e-3, 0.3 (repeating): row 1 is quiet."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(T, dtype=torch.float64) / float(rate)
    x = noise * torch.randn(B, T, generator=g, dtype=torch.float64)
    for b in range(B):
        for f, amp in ((0.005 * rate * (b + 1), 0.3), (0.04 * rate + 37.0 * b, 0.2), (0.2 * rate - 500.0 * b, 0.1)):
            x[b] += amp * torch.sin(2.0 * math.pi * f * t + 0.5 * b)
    x = 0.9 * x / x.abs().amax()
    scale = torch.tensor([ROW_SCALES[b % len(ROW_SCALES)] for b in range(B)], dtype=torch.float64)
    return (x * scale.unsqueeze(1)).to(torch.float32).contiguous()


class MelCase:
    """One mel shape: (n_fft, rate, bands, hop, T, power) and the filterbank's extra arguments (f_min, f_max, norm)."""

    def __init__(self, n_fft, rate, bands, hop, T, power, **extra):
        self.n_fft, self.rate, self.bands, self.hop, self.T, self.power, self.extra = n_fft, rate, bands, hop, T, power, extra

    @property
    def id(self):
        tail = "".join(f"-{k}{v}" for k, v in sorted(self.extra.items()))
        return f"{self.n_fft}-{self.rate}-{self.bands}-hop{self.hop}-T{self.T}-p{int(self.power)}{tail}"

    @property
    def kwargs(self):
        """The keyword arguments of spectral.MelSpectrogram / MelSpectrogramL1 and of the oracle's mel_spectrogram / mel_l1."""
        return dict(sample_rate=self.rate, n_fft=self.n_fft, hop_length=self.hop, n_mels=self.bands, power=self.power,
                    **self.extra)

    @property
    def span(self):
        """The backward runs the span kernels (overlap-add inside the kernel): even hops up to n_fft / 2; otherwise the
        frame kernel and the fold."""
        return self.hop % 2 == 0 and self.hop <= self.n_fft // 2

    @property
    def seed(self):
        return 1000 + 7 * MEL_CASES.index(self)


BATCH = 3
MEL_CASES = [
    MelCase(512, 16000, 40, 128, 4000, 2.0),
    MelCase(512, 16000, 23, 77, 3001, 1.0),
    MelCase(512, 44100, 128, 256, 3001, 2.0),
    MelCase(512, 44100, 192, 128, 2000, 2.0),
    MelCase(512, 44100, 64, 300, 2500, 2.0, f_min=30.0, f_max=8000.0),
    MelCase(1024, 22050, 80, 77, 5001, 1.0),
    MelCase(1024, 44100, 100, 256, 6000, 2.0),
    MelCase(1024, 16000, 23, 512, 4097, 2.0),
    MelCase(1024, 44100, 160, 600, 5000, 1.0),
    MelCase(1024, 44100, 192, 256, 5000, 2.0),
    MelCase(1024, 44100, 64, 512, 5000, 2.0, f_min=30.0, f_max=8000.0),
    MelCase(1024, 44100, 40, 256, 5000, 2.0, norm=None),
    MelCase(2048, 44100, 128, 512, 9000, 2.0),
    MelCase(2048, 16000, 23, 240, 6000, 1.0),
    MelCase(2048, 44100, 192, 1100, 9001, 2.0),
    MelCase(2048, 44100, 128, 2048, 1114, 2.0),      # one frame per row
]


def case_inputs(case):
    """-> (noise, tones, a, b): the two value inputs and the (audio, target) pair of the loss and its gradient."""
    s = case.seed
    return (noise(BATCH, case.T, s), tones(BATCH, case.T, case.rate, s + 1), tones(BATCH, case.T, case.rate, s + 2),
            tones(BATCH, case.T, case.rate, s + 3))


def value_ratios(out, ref, empty=None):
    """Worst |out - ref| over the reference's maximum at four granularities, for [B, bands, frames] tensors: the whole
    tensor, each row, each (row, frame), each band over batch and frames -> dict of floats, plus "bands": the per-band
    ratios [bands].  Bands listed in ``empty`` (an all-zero filter: their maximum is 0) are left out of the band ratios."""
    out, ref = out.double(), ref.double()
    err = (out - ref).abs()
    band_max = ref.abs().amax(dim=(0, 2))
    if empty is not None and len(empty):
        band_max = band_max.clone()
        band_max[list(empty)] = float("inf")
    bands = err.amax(dim=(0, 2)) / band_max
    return {"global": (err.max() / ref.abs().max()).item(),
            "row": (err.amax(dim=(1, 2)) / ref.abs().amax(dim=(1, 2))).max().item(),
            "frame": (err.amax(dim=1) / ref.abs().amax(dim=1)).max().item(),
            "band": bands.max().item(),
            "bands": bands}


def grad_ratios(g, ref, n_fft):
    """Relative L2 error of a gradient [B, T] at four granularities: the whole tensor, each row, the first n_fft / 2
    samples of each row (the reflect-folded region) and the last n_fft / 2 -> dict of the worst of each."""
    g, ref = g.double(), ref.double()
    h = n_fft // 2

    def rel(a, b):
        return ((a - b).norm(dim=-1) / b.norm(dim=-1)).max().item()

    return {"whole": rel(g.flatten(), ref.flatten()), "row": rel(g, ref), "head": rel(g[:, :h], ref[:, :h]),
            "tail": rel(g[:, -h:], ref[:, -h:])}

"""The FFT kernels' complex helpers, product form against the superseded form, bit for bit.

The product library writes every product that takes a swapped or negated operand -- complex multiplies, multiplications
by -i inside the radix-4 / radix-8 butterflies -- per component, so that no operand pair is built in front of a packed
instruction (csrc/stft_core.h: cmul, cadd_negi, csub_negi, cnegi_sub).  The diagnostic library (-DIAS_DIAG)
keeps the generic 2-wide vector expressions.  Both are the same products, the same fused multiply-adds and the same
rounding points, so every kernel built on them must give the same bits from either library: the forward transforms of
all three sizes (mel and linear bins, one and two sub-transforms per frame, two frames per wave), and the backward
kernels of the linear-bin losses.  Everything goes through the public modules of spectral.py, once per library."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def _audio(B, T, seed):
    """Seeded noise plus a few sines per row, peak below 1."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(T, dtype=torch.float64) / 44100.0
    x = 0.1 * torch.randn(B, T, generator=g, dtype=torch.float64)
    for b in range(B):
        for f, amp in ((220.0 * (b + 1), 0.3), (1760.0 + 37.0 * b, 0.2), (9000.0 - 500.0 * b, 0.1)):
            x[b] += amp * torch.sin(2.0 * math.pi * f * t + 0.5 * b)
    x = x.to(torch.float32)
    return (0.9 * x / x.abs().amax()).contiguous()


def _both(fn):
    """fn() on the product library and on the diagnostic one -> (product, diagnostic), tensors on the host."""
    from inverse_audio_synthesis_amd import _lib

    def host(r):
        torch.cuda.synchronize()
        return [t.detach().cpu() for t in r]

    prod = host(fn())
    with _lib.use_library(_lib.load_diag()):
        diag = host(fn())
    return prod, diag


def _same(names, prod, diag):
    for name, p, d in zip(names, prod, diag):
        assert torch.isfinite(p).all(), name
        assert p.shape == d.shape and torch.equal(p, d), (name, (p != d).sum().item())


@pytest.mark.parametrize("T", [5000, 5001])
def test_mel_path_same_bits(lib, dev, T):
    """n_fft 1024 / hop 512 / 128 mels, 10 frames per row: the first and last frame of a row take the reflect loads, at the
    odd length rows 1 and 2 start at odd offsets and the interior frames take the per-sample load path; row 1 clips and is
    normalised through rowpeak."""
    from inverse_audio_synthesis_amd.spectral import MelSpectrogramL1
    a, tgt = _audio(3, T, 11).clone(), _audio(3, T, 12)
    a[1] *= 1.7
    a, tgt = a.to(dev), tgt.to(dev)
    rowpeak = a.abs().amax(dim=1).contiguous()
    assert rowpeak[1].item() > 1.0 and rowpeak[0].item() <= 1.0

    def run():
        m = MelSpectrogramL1(sample_rate=44100, n_fft=1024, hop_length=512, n_mels=128).to(dev)
        mel = m.target(a)
        assert mel.shape == (3, 10, 128)
        return mel, m(a, target_audio=tgt, rowpeak=rowpeak), m(a, target_audio=tgt)

    _same(("mel", "loss with rowpeak", "loss"), *_both(run))


def _linear_losses(dev):
    from inverse_audio_synthesis_amd.spectral import MultiResolutionSTFTLoss, STFTL1
    return (("stft-l1 1024", STFTL1(n_fft=1024, hop_length=512).to(dev)),
            ("stft-l1 512", STFTL1(n_fft=512, hop_length=256).to(dev)),
            ("mr-stft", MultiResolutionSTFTLoss().to(dev)))


def test_linear_bins_same_bits(lib, dev):
    """STFT-L1 at n_fft 1024 and 512 (two frames per wave) and the three MR-STFT resolutions (2048: two sub-transforms)."""
    a, tgt = _audio(2, 5000, 21).to(dev), _audio(2, 5000, 22).to(dev)

    def run():
        with torch.no_grad():
            return [m(a, tgt) for _, m in _linear_losses(dev)]

    _same([n for n, _ in _linear_losses(dev)], *_both(run))


def test_backward_same_bits(lib, dev):
    """d loss / d audio of the same losses: the span kernels of n_fft 1024 / 2048 / 512 run the transform both ways."""
    a0, tgt = _audio(2, 5000, 31).to(dev), _audio(2, 5000, 32).to(dev)

    def run():
        out = []
        for _, m in _linear_losses(dev):
            a = a0.clone().requires_grad_(True)
            loss = m(a, tgt)
            loss.backward()
            assert a.grad is not None and a.grad.abs().max().item() > 0.0
            out += [loss, a.grad]
        return out

    names = [f"{n} {w}" for n, _ in _linear_losses(dev) for w in ("loss", "grad")]
    _same(names, *_both(run))

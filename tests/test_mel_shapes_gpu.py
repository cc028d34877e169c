"""The mel path of the HIP spectral kernels at every FFT size and a spread of filterbank shapes, against the oracle in fp64.

The rest of the suite runs the mel kernels at n_fft 1024 / 128 bands / hop 512 only.  Every other mel plan takes kernels that
no other GPU test reaches in the product library: forward the CSR kernel stft_kernel<9,4> / <10,4> / <11,12> (n_fft 1024
plans whose filterbank gets no segment table included), backward stft_grad_wave_kernel<9 | 10 | 11, MEL, SPAN> in both
forms (SPAN: even hops up to n_fft / 2; otherwise the frame kernel and the fold).  The shapes are spectral_inputs.MEL_CASES
(B = 3 everywhere); test_mel_shapes_cpu.py pins which forward kernel each lands on and shows that the oracle's own fp32
evaluation is more than ten times inside every bar used here.

Bars (the project's own, test_spectral_gpu.py / test_spectral_grad_gpu.py, applied at finer granularity):
  values    1e-4 of the maximum of the tensor, of each row (one row is 1000 times quieter than the others), on tones of
            each frame, on noise of each band over batch and frames; bands with an empty filter are exactly 0
  losses    1e-3 relative
  gradient  2e-3 relative L2 over the tensor, per row, on the first n_fft / 2 samples of every row (the reflect-folded
            region) and on the last n_fft / 2; a second backward gives the same bits
No element is excluded anywhere.

(f) shows that the per-band bar sees a one-bin error: a band's filter moved down by one bin in the device copy of the CSR
tables puts that band, and only that band, over the bar.  Only the CSR kernel is perturbed this way: a filterbank with one
filter shifted has three filters over a bin, and ias_stft_build_segtab refuses it, so the segment-table kernel cannot be
given the perturbed filters.

What these shapes found: n_fft 2048 with 23 bands (16 kHz) and with 192 bands gave NaN in the last band of every frame.
The filter loops pad every filter to four taps, so the last filter reads up to three words behind the power values in
the wave's scratch, with zero weights.  At n_fft 2048 the first of those words is a padding slot of the FFT passes that
nothing writes: whatever bits the LDS held, times zero.  The 128-band filterbank's last filter happens to end on a
multiple of four taps and never read it.  stft_kernel and stft_grad_wave_kernel (whose layout has the same hole at
n_fft 512) now zero the three words once per wave.

Measured on an MI355X, with that fix (worst ratio per case.  values: the asserted granularities on both inputs, as a
fraction of the respective maximum; loss: with and without rowpeak; gradient: whole / row / head / tail):

  case                                                 forward  backward  values    loss      gradient
  512-16000-40-hop128-T4000-p2                         CSR      span      2.9e-07   2.3e-07   9.1e-08
  512-16000-23-hop77-T3001-p1                          CSR      frames    3.3e-07   9.3e-08   3.5e-07
  512-44100-128-hop256-T3001-p2                        CSR      span      2.6e-07   1.5e-07   1.3e-07
  512-44100-192-hop128-T2000-p2                        CSR      span      2.9e-07   5.8e-08   1.5e-07
  512-44100-64-hop300-T2500-p2-f_max8000.0-f_min30.0   CSR      frames    2.8e-07   3.6e-07   1.4e-07
  1024-22050-80-hop77-T5001-p1                         CSR      frames    3.4e-07   4.2e-08   5.1e-07
  1024-44100-100-hop256-T6000-p2                       CSR      span      3.9e-07   9.4e-08   1.1e-07
  1024-16000-23-hop512-T4097-p2                        CSR      span      3.6e-07   1.6e-07   9.4e-08
  1024-44100-160-hop600-T5000-p1                       CSR      frames    2.4e-07   8.8e-08   9.1e-07
  1024-44100-192-hop256-T5000-p2                       segtab   span      3.3e-07   6.6e-08   1.2e-07
  1024-44100-64-hop512-T5000-p2-f_max8000.0-f_min30.0  segtab   span      3.6e-07   1.0e-07   1.1e-07
  1024-44100-40-hop256-T5000-p2-normNone               CSR      span      3.5e-07   9.8e-08   1.1e-07
  2048-44100-128-hop512-T9000-p2                       CSR      span      3.2e-07   1.4e-07   1.4e-07
  2048-16000-23-hop240-T6000-p1                        CSR      span      4.9e-07   2.0e-07   1.0e-05
  2048-44100-192-hop1100-T9001-p2                      CSR      frames    3.7e-07   1.6e-07   1.6e-07
  2048-44100-128-hop2048-T1114-p2                      CSR      frames    3.8e-07   1.6e-07   1.1e-07

  per-sound form (d): row losses <= 1.8e-07, gradients <= 1.2e-06
  linear bins (e): <= 3.3e-07 of every row's and every frame's maximum, magnitude and power, all three sizes
  one-bin shift (f): the shifted band at 1.6e-01 of its maximum, every other band <= 3.4e-07
No library call refused a shape (the largest, n_fft 2048 / 192 bands, needs 152504 of the forward's 153600 bytes of LDS).
"""
import pytest
import torch

from oracle import spectral_oracle as spo
from spectral_inputs import BATCH, MEL_CASES, case_inputs, grad_ratios, tones, value_ratios

pytestmark = pytest.mark.gpu
VALUE_BAR, LOSS_BAR, GRAD_BAR = 1e-4, 1e-3, 2e-3
BY_ID = {c.id: c for c in MEL_CASES}
ROWS_CASES = [BY_ID[i] for i in ("512-44100-128-hop256-T3001-p2", "1024-44100-160-hop600-T5000-p1",
                                 "2048-16000-23-hop240-T6000-p1")]
ROW_COTANGENTS = (1.0, 0.0, 0.5)


class _Ref:
    """The fp64 oracle's results for one case, computed once and never modified."""


_REFS = {}


def _ref(case):
    r = _REFS.get(case.id)
    if r is not None:
        return r
    r = _Ref()
    kw = case.kwargs
    r.noise, r.tones, r.a, r.b = case_inputs(case)
    r.mel_noise = spo.mel_spectrogram(r.noise.double(), **kw)
    r.mel_tones = spo.mel_spectrogram(r.tones.double(), **kw)
    fb = spo.melscale_fbanks(case.n_fft // 2 + 1, kw.get("f_min", 0.0), kw.get("f_max", float(case.rate // 2)),
                             case.bands, case.rate, kw.get("norm", "slaney"))
    r.empty = torch.nonzero(fb.abs().sum(dim=0) == 0).flatten().tolist()
    ad = r.a.double().requires_grad_(True)
    diff = (spo.mel_spectrogram(ad, **kw) - spo.mel_spectrogram(r.b.double(), **kw)).abs()
    r.row_means = diff.mean(dim=(1, 2))
    loss = diff.mean()
    (r.grad,) = torch.autograd.grad(loss, ad, retain_graph=True)
    cot = torch.tensor(ROW_COTANGENTS, dtype=torch.float64)
    (r.grad_rows,) = torch.autograd.grad((r.row_means * cot).sum(), ad)
    r.row_means = r.row_means.detach()
    r.loss = loss.item()
    assert abs(r.loss - spo.mel_l1(r.a.double(), r.b.double(), **kw).item()) <= 1e-12 * r.loss
    # the clipping row of the folded normalisation: row 0 times 1.7
    r.a2 = r.a.clone()
    r.a2[0] *= 1.7
    peak = r.a2.abs().amax(dim=1)
    assert peak[0].item() > 1.0 and (peak[1:] <= 1.0).all()
    norm = r.a2.double() / torch.where(peak > 1.0, peak, torch.ones_like(peak)).double().unsqueeze(1)
    r.loss_normalised = spo.mel_l1(norm, r.b.double(), **kw).item()
    _REFS[case.id] = r
    return r


def _fmt(d):
    return " ".join(f"{k}={v:.2e}" for k, v in d.items() if k != "bands")


def _check_grad(tag, g, ref, n_fft):
    assert g.shape == ref.shape and torch.isfinite(g).all(), tag
    r = grad_ratios(g, ref, n_fft)
    print(f"{tag}: gradient rel-L2 {_fmt(r)}")
    for k, v in r.items():
        assert v <= GRAD_BAR, (tag, k, v)


@pytest.mark.parametrize("case", MEL_CASES, ids=lambda c: c.id)
def test_values(lib, dev, case):
    """(a) MelSpectrogram against the fp64 oracle on noise and on tones."""
    from inverse_audio_synthesis_amd.spectral import MelSpectrogram
    r = _ref(case)
    mel = MelSpectrogram(**case.kwargs).to(dev)
    assert (mel.plan.mel_count == 0).nonzero().flatten().tolist() == r.empty
    for name, x, ref, own in (("noise", r.noise, r.mel_noise, "band"), ("tones", r.tones, r.mel_tones, "frame")):
        out = mel(x.to(dev)).cpu()
        assert out.shape == ref.shape and torch.isfinite(out).all(), name
        v = value_ratios(out, ref, r.empty)
        print(f"{case.id} {name}: value error over maximum {_fmt(v)}")
        for k in ("global", "row", own):
            assert v[k] <= VALUE_BAR, (name, k, v[k], v["bands"].argmax().item())
        if r.empty:
            assert (out[:, r.empty, :] == 0.0).all(), name


@pytest.mark.parametrize("case", MEL_CASES, ids=lambda c: c.id)
def test_fused_loss(lib, dev, case):
    """(b) The fused forward (loss_mode 1), its cached-target form, and the folded normalisation (rowpeak)."""
    from inverse_audio_synthesis_amd.spectral import MelSpectrogramL1
    r = _ref(case)
    m = MelSpectrogramL1(**case.kwargs).to(dev)
    a, b = r.a.to(dev), r.b.to(dev)
    got = m(a, target_audio=b)
    rel = abs(got.item() - r.loss) / r.loss
    assert torch.equal(m(a, target_mel=m.target(b)), got)
    a2 = r.a2.to(dev)
    rowpeak = a2.abs().amax(dim=1).contiguous()
    got2 = m(a2, target_audio=b, rowpeak=rowpeak).item()
    rel2 = abs(got2 - r.loss_normalised) / r.loss_normalised
    print(f"{case.id}: loss rel err {rel:.2e}, with rowpeak {rel2:.2e}")
    assert rel <= LOSS_BAR, (got.item(), r.loss)
    assert rel2 <= LOSS_BAR, (got2, r.loss_normalised)


@pytest.mark.parametrize("case", MEL_CASES, ids=lambda c: c.id)
def test_gradient(lib, dev, case):
    """(c) d loss / d audio against fp64 autograd through the oracle; twice, for the same bits."""
    from inverse_audio_synthesis_amd.spectral import MelSpectrogramL1
    r = _ref(case)
    m = MelSpectrogramL1(**case.kwargs).to(dev)
    b = r.b.to(dev)
    grads = []
    for _ in range(2):
        xa = r.a.to(dev).requires_grad_(True)
        loss = m(xa, target_audio=b)
        loss.backward()
        grads.append(xa.grad.clone())
    assert abs(loss.item() - r.loss) <= LOSS_BAR * r.loss
    _check_grad(f"{case.id} ({'span' if case.span else 'frames'})", grads[0].cpu(), r.grad, case.n_fft)
    assert torch.equal(grads[0], grads[1]), (grads[0] != grads[1]).sum().item()


@pytest.mark.parametrize("case", ROWS_CASES, ids=lambda c: c.id)
def test_per_sound_form(lib, dev, case):
    """(d) per_item and its gradient under the row cotangents [1, 0, 0.5]: the row with cotangent 0 gets exactly 0."""
    from inverse_audio_synthesis_amd.spectral import MelSpectrogramL1
    r = _ref(case)
    m = MelSpectrogramL1(**case.kwargs).to(dev)
    b = r.b.to(dev)
    xa = r.a.to(dev).requires_grad_(True)
    per = m.per_item(xa, target_audio=b)
    assert per.shape == (BATCH,)
    got = per.detach().cpu().double()
    print(f"{case.id}: per-row loss rel err {((got - r.row_means).abs() / r.row_means).max().item():.2e}")
    assert ((got - r.row_means).abs() <= LOSS_BAR * r.row_means).all(), (got, r.row_means)
    whole = m(r.a.to(dev), target_audio=b).item()
    assert abs(per.mean().item() - whole) <= LOSS_BAR * whole
    per.backward(torch.tensor(ROW_COTANGENTS, device=dev))
    g = xa.grad.cpu()
    assert (g[1] == 0.0).all()
    live = [i for i, c in enumerate(ROW_COTANGENTS) if c != 0.0]
    _check_grad(f"{case.id} per-sound", g[live], r.grad_rows[live], case.n_fft)


@pytest.mark.parametrize("n_fft,win,hop", [(512, 240, 50), (1024, 600, 120), (2048, 1200, 240)])
def test_linear_bins_at_row_and_frame_scale(lib, dev, n_fft, win, hop):
    """(e) The linear-bin values of the three MR-STFT resolutions, magnitude and power, held to each row's and each frame's
    own maximum (the other tests judge them against the global maximum and torch's fp32 transform)."""
    from inverse_audio_synthesis_amd.spectral import STFTPlan, VALUE_MAG, VALUE_POWER
    x = tones(BATCH, 6000, 44100, 77)
    plan = STFTPlan(n_fft, win, hop).to(dev)
    for mode, power in ((VALUE_MAG, 1.0), (VALUE_POWER, 2.0)):
        ref = spo.spectrogram(x.double(), n_fft, win, hop, power)
        out = plan.values(x.to(dev), mode).transpose(1, 2).cpu()
        assert out.shape == ref.shape and torch.isfinite(out).all()
        v = value_ratios(out, ref)
        print(f"linear bins {n_fft}/{win}/{hop} power {power:g}: value error over maximum {_fmt(v)}")
        for k in ("global", "row", "frame"):
            assert v[k] <= VALUE_BAR, (power, k, v[k])


def test_per_band_bar_sees_a_one_bin_shift(lib, dev):
    """(f) n_fft 1024 / 22050 Hz / 80 bands (the CSR kernel): one interior filter starts one bin too low."""
    from inverse_audio_synthesis_amd.spectral import MelSpectrogram
    case = BY_ID["1024-22050-80-hop77-T5001-p1"]
    r = _ref(case)
    mel = MelSpectrogram(**case.kwargs).to(dev)
    assert mel.plan.segtab is None
    band = 40
    start, count = int(mel.plan.mel_start[band]), int(mel.plan.mel_count[band])
    assert start >= 1 and count >= 2 and start + count + 4 <= case.n_fft // 2       # every access stays inside the power array
    mel.plan.mel_start[band] -= 1
    v = value_ratios(mel(r.noise.to(dev)).cpu(), r.mel_noise, r.empty)
    over = torch.nonzero(v["bands"] > VALUE_BAR).flatten().tolist()
    print(f"shifted band {band}: ratio {v['bands'][band].item():.2e}, worst other band "
          f"{torch.cat([v['bands'][:band], v['bands'][band + 1:]]).max().item():.2e}")
    assert over == [band], over

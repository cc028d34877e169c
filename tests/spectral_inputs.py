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


# ------------------------------------------------------------------------- silence, faint noise and clamped bins
# The rows of test_spectral_silence_cpu.py / test_spectral_silence_gpu.py: regions of loud noise, faint noise and exact
# zeros, so that the MR-STFT clamp sqrt(max(|X|^2, eps)) and the `live` tests of the backward kernels are exercised.  The
# log-magnitude gradient of a bin is sign / (count V): a bin within rounding of eps is live in one precision and clamped
# in the other and then carries the whole difference, so every row keeps |X|^2 out of [eps / 4, 4 eps] at every resolution
# below (test_spectral_silence_cpu.py proves it).  Seeds and boundaries were found by a search over candidates and are
# literal here: edit one and the CPU test says whether the new row still keeps the dead zone.
EPS = 1e-8
SILENCE_T = 12001                  # a multiple of no hop
LOUD_STD, FAINT_STD, FLOOR_STD = 0.3, 2e-7, 0.03
FAINT_SEED_OFFSET = 500
TONES_RATE = 16000
_T = SILENCE_T
RESOLUTION_SETS = {
    "1024": dict(fft_sizes=(1024,), hop_sizes=(120,), win_lengths=(600,)),
    "2048": dict(fft_sizes=(2048,), hop_sizes=(240,), win_lengths=(1200,)),
    "512": dict(fft_sizes=(512,), hop_sizes=(50,), win_lengths=(240,)),
    "defaults": dict(fft_sizes=(1024, 2048, 512), hop_sizes=(120, 240, 50), win_lengths=(600, 1200, 240)),
    "oddhop": dict(fft_sizes=(512, 1024), hop_sizes=(125, 256), win_lengths=(512, 1024)),   # no span plan: frames fallback
}


def resolutions(res):
    """The (n_fft, hop, win) triples of one resolution set."""
    return list(zip(res["fft_sizes"], res["hop_sizes"], res["win_lengths"]))


ALL_RESOLUTIONS = sorted({r for res in RESOLUTION_SETS.values() for r in resolutions(res)})

# name -> (prediction, target); a row is (seed, ((kind, stop), ...)): consecutive regions, the last one ending at T, or
# (seed, "tones")
SILENCE_ROWS = {
    "mid_gap": ((42, (("loud", 3028), ("silence", 8007), ("loud", _T))),
                (12, (("loud", 3528), ("silence", 7007), ("loud", _T)))),
    "lead_tail": ((3, (("silence", 2521), ("loud", 9028), ("silence", _T))),
                  (13, (("silence", 2600), ("loud", 9521), ("silence", _T)))),
    "faint_gap": ((84, (("loud", 3200), ("faint", 8100), ("loud", _T))),
                  (14, (("loud", 3200), ("silence", 8100), ("loud", _T)))),
    "faint_vs_loud": ((565, (("loud", 3300), ("faint", 8300), ("loud", _T))),
                      (15, (("loud", _T),))),
    "tgt_silent": ((6, (("loud", _T),)), (0, (("silence", _T),))),
    "pred_silent": ((0, (("silence", _T),)), (16, (("loud", _T),))),
    "pred_faint": ((8, (("faint", _T),)), (18, (("loud", _T),))),
    "identical": ((9, (("loud", 4014), ("silence", 8521), ("loud", _T))),) * 2,
    "both_silent": ((0, (("silence", _T),)),) * 2,
    "tones_floor": ((4610, "tones"), (120, "tones")),
}
GAPPED = ("mid_gap", "lead_tail", "faint_gap", "faint_vs_loud", "identical")     # 10 % .. 90 % of the bins clamped
WITH_FAINT = ("faint_gap", "faint_vs_loud", "pred_faint")                        # non-zero bins below eps / 4


def silence_row(spec, T=SILENCE_T):
    """One fp32 row [T] from its (seed, regions) entry."""
    seed, parts = spec
    if parts == "tones":
        return tones(1, T, TONES_RATE, seed, noise=FLOOR_STD)[0]
    kinds = {"loud": randn((1, T), seed)[0] * LOUD_STD, "faint": randn((1, T), seed + FAINT_SEED_OFFSET)[0] * FAINT_STD,
             "silence": torch.zeros(T)}
    x, start = torch.zeros(T), 0
    for kind, stop in parts:
        x[start:stop] = kinds[kind][start:stop]
        start = stop
    assert start == T
    return x.contiguous()


def silence_pair(name):
    """-> (prediction, target), fp32 [T] each."""
    p, t = SILENCE_ROWS[name]
    return silence_row(p), silence_row(t)


def silence_batch(names):
    """-> (predictions, targets), fp32 [len(names), T] each, rows in the order of ``names``."""
    pairs = [silence_pair(n) for n in names]
    return torch.stack([p for p, _ in pairs]).contiguous(), torch.stack([t for _, t in pairs]).contiguous()


def quiet_region(name):
    """(a, b): the prediction's first region that is not loud (its faint or silent stretch)."""
    start = 0
    for kind, stop in SILENCE_ROWS[name][0][1]:
        if kind != "loud":
            return start, stop
        start = stop
    raise ValueError(name)


def untouched_range(a, b, win, hop, T=SILENCE_T):
    """Frame f of a centred STFT with a window of ``win`` samples (centred in n_fft) reads the samples
    [f hop - win / 2, f hop + win / 2).  -> (lo, hi): the samples of the region [a, b) that only frames lying entirely
    inside [a, b) read.  The last frame that starts before a is f0 - 1 with f0 = ceil((a + win / 2) / hop), the first one
    that ends after b is f1 + 1 with f1 = floor((b - win / 2) / hop), so lo = (f0 - 1) hop + win / 2 and
    hi = (f1 + 1) hop - win / 2.  (a >= win and b <= T - win: no reflected frame reaches the region.)"""
    assert win % 2 == 0 and a >= win and b <= T - win
    f0 = -(-(a + win // 2) // hop)
    f1 = (b - win // 2) // hop
    lo, hi = (f0 - 1) * hop + win // 2, (f1 + 1) * hop - win // 2
    assert a <= lo < hi <= b
    return lo, hi


def untouched_range_of(name, res):
    """``untouched_range`` of the prediction's quiet region for every resolution of the set at once (the intersection)."""
    a, b = quiet_region(name)
    ranges = [untouched_range(a, b, win, hop) for _n, hop, win in resolutions(res)]
    return max(lo for lo, _ in ranges), min(hi for _, hi in ranges)


def stft_power(x, n_fft, hop, win):
    """|X|^2 of the oracle's STFT (torch.stft, hann window of ``win`` centred in n_fft) in x's precision -> [B, bins, frames]."""
    X = torch.stft(x, n_fft, hop, win, torch.hann_window(win).to(x.dtype), return_complex=True)
    return X.real ** 2 + X.imag ** 2


def mrstft_sums(x, y, n_fft, hop, win, eps=EPS):
    """The three per-row sums of one MR-STFT resolution in x's precision -> [B, 3]:
    sum (T - V)^2, sum T^2, sum |ln V - ln T| with V, T = sqrt(max(|X|^2, eps)) of prediction and target."""
    v = torch.sqrt(torch.clamp(stft_power(x, n_fft, hop, win), min=eps))
    t = torch.sqrt(torch.clamp(stft_power(y, n_fft, hop, win), min=eps))
    return torch.stack([((t - v) ** 2).sum(dim=(1, 2)), (t ** 2).sum(dim=(1, 2)),
                        (torch.log(v) - torch.log(t)).abs().sum(dim=(1, 2))], dim=1)


def loss_from_sums(sums, counts):
    """The MR-STFT loss from the per-resolution sums [B, 3] and element counts: mean_k sqrt(s0) / sqrt(s1) + s2 / count."""
    return sum(torch.sqrt(s[:, 0]) / torch.sqrt(s[:, 1]) + s[:, 2] / c for s, c in zip(sums, counts)) / len(sums)


class SilenceRef:
    """The oracle's results for one (row pair, resolution set, precision): ``sums`` (a [3] tensor per resolution),
    ``counts``, ``loss`` (float) and ``grad`` (d loss / d prediction, [T] in the oracle's precision)."""


_SILENCE_REFS = {}


def silence_ref(name, res, dtype=torch.float64):
    """Computed once per (name, resolutions, precision) and shared by the tests; never modified."""
    from oracle import spectral_oracle as spo
    key = (name, tuple(resolutions(res)), dtype)
    r = _SILENCE_REFS.get(key)
    if r is not None:
        return r
    r = SilenceRef()
    x, y = silence_pair(name)
    a = x.to(dtype)[None].requires_grad_(True)
    loss = spo.mrstft_loss(a, y.to(dtype)[None], eps=EPS, **res)[0]
    (g,) = torch.autograd.grad(loss, a)
    r.loss, r.grad = loss.item(), g[0]
    with torch.no_grad():
        r.sums = [mrstft_sums(a, y.to(dtype)[None], *rs)[0] for rs in resolutions(res)]
    r.counts = [(n // 2 + 1) * (1 + SILENCE_T // h) for n, h, _w in resolutions(res)]
    if dtype == torch.float64:                                            # the sums are the oracle's
        own = loss_from_sums([s[None] for s in r.sums], r.counts).item()
        assert abs(own - r.loss) <= 1e-12 * abs(r.loss), (own, r.loss)
    _SILENCE_REFS[key] = r
    return r


def row_ratios(g, ref, n_fft):
    """Relative L2 error of one row's gradient [T] over the row, its first n_fft / 2 samples and its last n_fft / 2 ->
    dict.  Where the reference is exactly 0 over a region the ratio is 0.0 if the gradient is exactly 0 there too, and
    inf otherwise."""
    g, ref = g.double(), ref.double()
    h = n_fft // 2

    def rel(a, b):
        if torch.count_nonzero(b).item() == 0:
            return 0.0 if torch.count_nonzero(a).item() == 0 else float("inf")
        return ((a - b).norm() / b.norm()).item()

    return {"row": rel(g, ref), "head": rel(g[:h], ref[:h]), "tail": rel(g[-h:], ref[-h:])}


SIGN_MARGIN = 1e-6


def sign_margin_violations(px, py, n_fft, eps=None, power=1.0):
    """Both gradients carry sign(V - T) of every bin, so a bin whose V and T agree to rounding is a second trap of the
    kind of the dead zone: its sign belongs to whoever rounded last.  A radix FFT of n_fft <= 2048 points in fp32 leaves
    an error of about log2(n_fft) <= 11 roundings (6e-8 each) of the frame's norm ||w x||_2 in a bin, so the inputs keep
    the magnitudes |V - T| above SIGN_MARGIN = 1e-6 (sixteen roundings) of the larger of the two frames' norms (power 2:
    the powers above 2 max(|X|, |Y|) times that).  px, py: fp64 powers [B, bins, frames]; eps: the MR-STFT clamp (bins
    clamped on both sides are equal by construction and excluded), None for the plain values of STFTL1 (bins that are
    exactly 0 on both sides excluded) -> the number of violations."""
    norm = torch.sqrt(2.0 * torch.maximum(px.sum(dim=1), py.sum(dim=1)) / n_fft).unsqueeze(1)
    if eps is None:
        v, t, same = px.sqrt(), py.sqrt(), (px == 0) & (py == 0)
    else:
        v, t, same = px.clamp(min=eps).sqrt(), py.clamp(min=eps).sqrt(), (px < eps) & (py < eps)
    if power == 2.0:
        close = (px - py).abs() <= 2.0 * torch.maximum(v, t) * SIGN_MARGIN * norm
    else:
        close = (v - t).abs() <= SIGN_MARGIN * norm
    return int((close & ~same).sum())


# the STFTL1 shapes of test_spectral_silence_gpu.py: (n_fft, hop, power), window = n_fft
STFT_L1_CASES = [(1024, 256, 1.0), (512, 100, 2.0), (2048, 512, 1.0)]
L1_ROWS = ("mid_gap", "lead_tail", "faint_gap", "pred_silent")
L1_KINDS = [("stft", c) for c in STFT_L1_CASES] + [("mel", (1024, 512, 2.0))]      # mel: MelSpectrogramL1's defaults
_L1_REFS = {}


def l1_ref(kind, name, case, dtype=torch.float64):
    """STFTL1 (case = (n_fft, hop, power)) or the default MelSpectrogramL1 of one row pair in the oracle ->
    (loss, d loss / d prediction [T]); computed once and shared."""
    from oracle import spectral_oracle as spo
    key = (kind, name, case, dtype)
    if key not in _L1_REFS:
        x, y = silence_pair(name)
        a = x.to(dtype)[None].requires_grad_(True)
        if kind == "stft":
            loss = spo.stft_l1(a, y.to(dtype)[None], n_fft=case[0], hop_length=case[1], power=case[2])
        else:
            loss = spo.mel_l1(a, y.to(dtype)[None])
        (g,) = torch.autograd.grad(loss, a)
        _L1_REFS[key] = (loss.item(), g[0])
    return _L1_REFS[key]

"""The per-sound multi-resolution STFT loss (MultiResolutionSTFTLoss.per_item) on the GPU: forward against the fp64
oracle and the batch loss, the per-row contract (position invariance, parallel streams), the backward (span path and
frames fallback), the scalar kernels against their host formula, the matcher with loss="multi_resolution_stft" and the
match_audio.py entry point."""
import ctypes
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

from oracle import spectral_oracle as spo
from oracle import synth_oracle as so
from helpers import randn, rel_l2

pytestmark = pytest.mark.gpu

DEFAULTS = dict(fft_sizes=(1024, 2048, 512), hop_sizes=(120, 240, 50), win_lengths=(600, 1200, 240))
ODD = dict(fft_sizes=(512, 1024), hop_sizes=(125, 256), win_lengths=(512, 1024))
# (resolutions, T): auraloss' defaults at 16 kHz with T = 20001 (a multiple of no hop; rows of every length sit at every
# 16-byte phase) and at 44.1 kHz for 1 s; a two-resolution set with an odd hop, which has no span plan (frames fallback)
SHAPES = [(DEFAULTS, 20001), (DEFAULTS, 44100), (ODD, 20001)]
IDS = ["defaults16k", "defaults44k", "oddhop"]
G = [0.7, 0.0, 1.9, 0.25]


def _module(res, dev):
    from inverse_audio_synthesis_amd.spectral import MultiResolutionSTFTLoss
    return MultiResolutionSTFTLoss(**res).to(dev)


def _oracle(res):
    return lambda a, t: spo.mrstft_loss(a, t, **res)[0]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_per_item_forward(lib, dev, shape):
    res, T = shape
    m = _module(res, dev)
    x, y = randn((3, T), 41) * 0.3, randn((3, T), 42) * 0.3
    got = m.per_item(x.to(dev), y.to(dev))
    assert got.shape == (3,) and got.dtype == torch.float32
    ref_fn = _oracle(res)
    for b in range(3):
        ref = ref_fn(x[b:b + 1].double(), y[b:b + 1].double()).item()
        assert abs(got[b].item() - ref) <= 1e-3 * abs(ref), (b, got[b].item(), ref)
        one = m.per_item(x[b:b + 1].to(dev), y[b:b + 1].to(dev)).item()
        batch = m(x[b:b + 1].to(dev), y[b:b + 1].to(dev)).item()
        assert abs(one - batch) <= 1e-5 * abs(batch), (b, one, batch)
    assert torch.equal(m.per_item(x.to(dev), y.to(dev)), got)
    # the cached targets give the same bits
    assert torch.equal(m.per_item(x.to(dev), targets=m.target(y.to(dev))), got)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_per_item_is_position_invariant(lib, dev, shape):
    """A row's loss is the same bits wherever it sits in the batch, whatever the other rows are, and with the resolutions
    on side streams or not."""
    res, T = shape
    m = _module(res, dev)
    x, y = (randn((8, T), 51) * 0.3).to(dev), (randn((8, T), 52) * 0.3).to(dev)
    base = m.per_item(x, y)
    perm = torch.tensor([5, 2, 7, 0, 3, 6, 1, 4], device=dev)
    assert torch.equal(m.per_item(x[perm].contiguous(), y[perm].contiguous()), base[perm])
    one = m.per_item(x[3:4].contiguous(), y[3:4].contiguous())
    assert torch.equal(one[0], base[3])
    m.parallel = False
    assert torch.equal(m.per_item(x, y), base)


def _grad(m, x, y, g, dev):
    xa = x.to(dev).requires_grad_(True)
    (torch.tensor(g, device=dev) * m.per_item(xa, y.to(dev))).sum().backward()
    return xa.grad.detach().clone()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_per_item_backward(lib, dev, shape):
    """d (sum_b g_b L_b) / d x: rows with g_b = 0 exactly 0; against fp64 autograd through the oracle (rel-L2 2e-3, as
    tests/test_spectral_grad_gpu.py); row b against g_b times the batch loss' gradient of row b alone (rel-L2 1e-5);
    run to run and serial / parallel: the same bits."""
    res, T = shape
    B = len(G)
    m = _module(res, dev)
    x, y = randn((B, T), 61) * 0.3, randn((B, T), 62) * 0.3
    got = _grad(m, x, y, G, dev)
    assert torch.isfinite(got).all()
    for b in range(B):
        if G[b] == 0:
            assert torch.count_nonzero(got[b]).item() == 0
            continue
        xb = x[b:b + 1].to(dev).requires_grad_(True)
        m(xb, y[b:b + 1].to(dev)).backward()
        want = xb.grad.detach()[0] * G[b]
        assert rel_l2(got[b].cpu(), want.cpu()) <= 1e-5, (b, rel_l2(got[b].cpu(), want.cpu()))
    ref_fn = _oracle(res)
    a = x.double().requires_grad_(True)
    total = sum(G[b] * ref_fn(a[b:b + 1], y[b:b + 1].double()) for b in range(B))
    (ref,) = torch.autograd.grad(total, a)
    assert rel_l2(got.cpu(), ref) <= 2e-3, rel_l2(got.cpu(), ref)
    assert torch.equal(_grad(m, x, y, G, dev), got)
    m.parallel = False
    assert torch.equal(_grad(m, x, y, G, dev), got)


def test_span_plans_of_the_shapes(lib):
    """The defaults take the span path at both rates, the odd-hop set has no span plan for its first resolution."""
    def ok(B, T, n_fft, hop):
        return lib.ias_stft_grad_span_plan(B, T, n_fft, hop, 0, n_fft // 2 + 1, (ctypes.c_int * 3)()) == 0
    for T in (20001, 44100):
        assert all(ok(4, T, n, h) for n, h in zip(DEFAULTS["fft_sizes"], DEFAULTS["hop_sizes"]))
    assert not ok(4, 20001, 512, 125)


@pytest.mark.parametrize("n_fft,hop,win", [(1024, 120, 600), (512, 125, 512)], ids=["span", "oddhop"])
def test_backward_entry_without_tables(lib, dev, n_fft, hop, win):
    """ias_stft_loss_backward_mrstft_rows with tables = NULL (the workgroup-per-frame-pair kernel) and with the plan's
    tables (the wave-per-frame kernels), both with the coefficient pairs of ias_mrstft_coef_rows, against fp64 autograd of
    sum_b g_b L_b for this one resolution (rel-L2 2e-3).  The two FFT cores differ by ~1e-4 (rel-L2) near the reflected
    ends: sign(V - T) / V flips where V and T agree to rounding."""
    from inverse_audio_synthesis_amd import _lib
    from inverse_audio_synthesis_amd.spectral import STFTPlan, VALUE_MAG_CLAMPED
    B, T, eps = 4, 20001, 1e-8
    plan = STFTPlan(n_fft, win, hop).to(dev)
    x, y = (randn((B, T), 71) * 0.3).to(dev), (randn((B, T), 72) * 0.3).to(dev)
    tgt = plan.values(y, VALUE_MAG_CLAMPED, eps)
    sums = plan.mrstft_rows(plan.values(x, VALUE_MAG_CLAMPED, eps), tgt)
    g = torch.tensor(G, device=dev)
    coef = torch.empty((B, 2), dtype=torch.float64, device=dev)
    _lib.check(lib.ias_mrstft_coef_rows(_lib.ptr(sums), _lib.ptr(g), float(tgt[0].numel()), 1, B, _lib.ptr(coef),
                                        _lib.stream()), "ias_mrstft_coef_rows")
    outs = []
    for tables in (plan.tables, None):
        frame_grad = torch.empty((B, plan.num_frames(T), n_fft), dtype=torch.float32, device=dev)
        out = torch.empty_like(x)
        _lib.check(lib.ias_stft_loss_backward_mrstft_rows(
            _lib.ptr(x), _lib.ptr(plan.window), _lib.ptr(tables) if tables is not None else None, _lib.ptr(tgt),
            _lib.ptr(coef), _lib.ptr(frame_grad), _lib.ptr(out), B, T, n_fft, hop, plan.n_out, eps, _lib.stream()),
            "ias_stft_loss_backward_mrstft_rows")
        outs.append(out)
    assert torch.count_nonzero(outs[1][1]).item() == 0 and torch.count_nonzero(outs[0][1]).item() == 0
    a = x.cpu().double().requires_grad_(True)
    yd = y.cpu().double()
    one = dict(fft_sizes=(n_fft,), hop_sizes=(hop,), win_lengths=(win,))
    total = sum(G[b] * spo.mrstft_loss(a[b:b + 1], yd[b:b + 1], **one)[0] for b in range(B))
    (ref,) = torch.autograd.grad(total, a)
    for out in outs:
        assert rel_l2(out.cpu(), ref) <= 2e-3, rel_l2(out.cpu(), ref)
    assert rel_l2(outs[1].cpu(), outs[0].cpu()) <= 1e-3, rel_l2(outs[1].cpu(), outs[0].cpu())


# ------------------------------------------------------------------------------------------------ scalar kernels
def test_rows_total_and_coef_rows_against_host_formula(lib, dev):
    from inverse_audio_synthesis_amd import _lib
    B, nres = 4, 2
    gen = torch.Generator().manual_seed(81)
    sums = [torch.rand((B, 3), generator=gen, dtype=torch.float64) * 100 + 1 for _ in range(nres)]
    sums[1][2, 1] = 0.0                       # row 2 of resolution 1: sum T^2 = 0 -> coef[0] = 0
    sums[0][3, 0] = 0.0                       # row 3 of resolution 0: V == T -> coef[0] = 0
    counts = [1234.0, 5678.0]
    dsums = [s.to(dev) for s in sums]
    out = torch.empty(B, dtype=torch.float32, device=dev)
    ptrs = (ctypes.c_void_p * nres)(*[s.data_ptr() for s in dsums])
    _lib.check(lib.ias_mrstft_rows_total(ptrs, (ctypes.c_double * nres)(*counts), nres, B, _lib.ptr(out), _lib.stream()),
               "ias_mrstft_rows_total")
    import math
    for b in range(B):
        total = 0.0
        for k in range(nres):
            s = sums[k][b].tolist()
            term = math.sqrt(s[0]) / math.sqrt(s[1]) + s[2] / counts[k] if s[1] > 0 else float("inf")
            total = term if k == 0 else total + term
        want = total / nres
        if math.isfinite(want):
            assert abs(out[b].item() - want) <= 1e-6 * abs(want), (b, out[b].item(), want)
        else:
            assert not math.isfinite(out[b].item())
    g = torch.tensor(G, dtype=torch.float32)
    for k in range(nres):
        coef = torch.full((B, 2), 7.0, dtype=torch.float64, device=dev)
        _lib.check(lib.ias_mrstft_coef_rows(_lib.ptr(dsums[k]), _lib.ptr(g.to(dev)), counts[k], nres, B, _lib.ptr(coef),
                                            _lib.stream()), "ias_mrstft_coef_rows")
        coef = coef.cpu()
        for b in range(B):
            s = sums[k][b].tolist()
            gb = float(g[b])
            if gb == 0.0:
                want = (0.0, 0.0)
            else:
                den = math.sqrt(s[0]) * math.sqrt(s[1])
                want = (gb / (nres * den) if den > 0 else 0.0, gb / (nres * counts[k]))
            for j in range(2):
                assert abs(coef[b, j].item() - want[j]) <= 1e-14 * abs(want[j]), (k, b, j, coef[b, j].item(), want[j])
    assert coef[1].tolist() == [0.0, 0.0]


# ------------------------------------------------------------------------------------------------ matcher
def _voice(dev, B=4, sr=16000, sec=1.0):
    from inverse_audio_synthesis_amd.voice import SynthConfig, Voice
    return Voice(SynthConfig(batch_size=B, sample_rate=sr, buffer_size_seconds=sec, reproducible=False)).to(dev)


def test_matcher_fixed_point(lib, dev):
    from inverse_audio_synthesis_amd.match import SoundMatcher
    v = _voice(dev)
    tp = so.sample_params01(so.VoiceConfig(4, 16000, 1.0), 7).to(dev)
    target = v.render(tp)
    res = SoundMatcher(v, loss="multi_resolution_stft").fit(target, init_params01=tp, steps=3)
    assert torch.count_nonzero(res.loss).item() == 0 and torch.count_nonzero(res.initial_loss).item() == 0
    assert torch.equal(res.params01, tp)
    assert res.skipped.tolist() == [0, 0, 0, 0]


def test_matcher_descends_on_mixer_levels(lib, dev):
    """As tests/test_match_gpu.py::test_matcher_descends_on_mixer_levels with the MR-STFT loss: the three mixer levels
    free at 0.5, every other column frozen at the target, 50 Adam steps at lr 0.02 must at least halve every sound's loss
    (measured on an MI355X: final / initial = 0.0272, 0.0125, 0.0184, 0.0048 for the four sounds).  The returned loss is, bit for bit, the per-item loss of a fresh render of the returned parameters."""
    from inverse_audio_synthesis_amd import voice_spec as S
    from inverse_audio_synthesis_amd.match import SoundMatcher
    v = _voice(dev)
    tp = so.sample_params01(so.VoiceConfig(4, 16000, 1.0), 7).to(dev)
    target = v.render(tp)
    free = [("mixer", n) for n in ("vco_1", "vco_2", "noise")]
    init = tp.clone()
    init[:, [S.INDEX[k] for k in free]] = 0.5
    frozen = [(m, n) for (m, n, *_r) in S.PARAMS if (m, n) not in free]
    matcher = SoundMatcher(v, loss="multi_resolution_stft", lr=0.02, frozen=frozen)
    res = matcher.fit(target, init_params01=init, steps=50)
    ratio = (res.loss.double() / res.initial_loss.double()).tolist()
    print("matcher descent: final / initial MR-STFT loss per sound:", [f"{r:.4f}" for r in ratio])
    assert all(r <= 0.5 for r in ratio), ratio
    assert torch.equal(res.params01[:, [S.INDEX[k] for k in frozen]], tp[:, [S.INDEX[k] for k in frozen]])
    assert res.skipped.tolist() == [0, 0, 0, 0]
    fresh = matcher.loss.per_item(v.render(res.params01), target)
    assert torch.equal(fresh, res.loss)


def test_matcher_pads_the_last_chunk(lib, dev):
    from inverse_audio_synthesis_amd.match import SoundMatcher
    v = _voice(dev)
    tp = torch.cat([so.sample_params01(so.VoiceConfig(4, 16000, 1.0), s) for s in (3, 4)]).to(dev)   # [8, 78]
    target = torch.cat([v.render(tp[:4]), v.render(tp[4:])])
    m = SoundMatcher(v, loss="multi_resolution_stft", lr=0.02)
    six = m.fit(target[:6], steps=4)
    four = m.fit(target[:4], steps=4)
    two = m.fit(target[4:6], steps=4)
    assert six.params01.shape == (6, 78) and six.loss.shape == (6,)
    assert torch.equal(six.params01[:4], four.params01) and torch.equal(six.loss[:4], four.loss)
    assert torch.equal(six.params01[4:], two.params01) and torch.equal(six.loss[4:], two.loss)
    assert torch.equal(six.initial_loss, torch.cat([four.initial_loss, two.initial_loss]))
    assert torch.isfinite(six.loss).all() and (six.loss <= six.initial_loss).all()
    with pytest.raises(ValueError):
        SoundMatcher(v, loss="mrstft")


# ------------------------------------------------------------------------------------------------ entry point
def _write_wav(path, x, sr):
    pcm = np.round(np.clip(x, -1, 1) * 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(pcm.tobytes())


def test_match_audio_entry_point(lib, dev, tmp_path):
    from conftest import ROOT
    v = _voice(dev, B=2)
    audio = v.render(so.sample_params01(so.VoiceConfig(2, 16000, 1.0), 13).to(dev)).cpu().numpy()
    _write_wav(tmp_path / "a.wav", audio[0], 16000)
    _write_wav(tmp_path / "b.wav", audio[1], 16000)
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "match_audio.py"), str(tmp_path / "a.wav"), str(tmp_path / "b.wav"),
           "torchsynth.rate=16000", "torchsynth.buffer_size_seconds=1.0", "--steps", "3", "--loss", "multi_resolution_stft",
           "--out", str(out)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:]
    for name in ("a", "b"):
        rec = json.load(open(out / f"{name}.params.json"))
        assert rec["loss_kind"] == "multi_resolution_stft"
        assert len(rec["params"]) == 78 and rec["final_loss"] <= rec["initial_loss"]
        with wave.open(str(out / f"{name}.match.wav"), "rb") as w:
            assert w.getnframes() == 16000 and w.getframerate() == 16000

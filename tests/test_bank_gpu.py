"""Spectral bank on the GPU: ias_l1_cdist against an fp64 reference, its per-row contract (the same bits wherever a pair
sits), non-finite rows, exact recovery of a bank voice, the distance as the matcher's own loss, several starts per sound
in SoundMatcher.fit and match_audio.py --init bank."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

from oracle import synth_oracle as so

pytestmark = pytest.mark.gpu


def _rand(shape, seed, dev):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def _ref(q, b):
    """fp64 mean |q[n] - b[m]| over k, on the device, a block of queries at a time."""
    out = []
    for n0 in range(0, q.shape[0], 8):
        qq = q[n0:n0 + 8].double()
        out.append((qq[:, None, :] - b.double()[None, :, :]).abs().sum(-1) / q.shape[1])
    return torch.cat(out)


# a representative cross product of N in {1, 3, 64, 130}, M in {1, 5, 257, 1000}, K in {1, 7, 4095, 4096, 4097, 44160}:
# every value of each, the three launch shapes (N <= 4, N <= 32, larger) and partial tiles, slices and chunks
CASES = [(1, 1, 1), (3, 5, 7), (64, 257, 4095), (130, 1000, 4096), (3, 1000, 4097), (1, 257, 44160), (130, 5, 44160),
         (64, 1, 4097), (130, 257, 7), (1, 1000, 4096), (3, 1, 44160), (64, 1000, 1), (130, 1, 4095), (1, 5, 4097)]


@pytest.mark.parametrize("N,M,K", CASES, ids=[f"{n}x{m}x{k}" for n, m, k in CASES])
def test_cdist_matches_fp64(lib, dev, N, M, K):
    from inverse_audio_synthesis_amd.retrieval import l1_cdist
    q, b = _rand((N, K), 1000 + N + K, dev), _rand((M, K), 2000 + M + K, dev) * 0.7 + 0.1
    got = l1_cdist(q, b)
    assert got.shape == (N, M) and got.dtype == torch.float32
    ref = _ref(q, b)
    rel = ((got.double() - ref).abs() / ref.abs().clamp_min(1e-30)).max().item()
    print(f"ias_l1_cdist ({N}, {M}, {K}) worst relative error vs fp64: {rel:.2e}")
    assert rel <= 1e-5
    assert torch.equal(l1_cdist(q, b), got)          # run to run


def test_cdist_full_size_sampled(lib, dev):
    """(128, 4096, 44160), the bank search of a full batch at the full config: 64 sampled pairs against fp64."""
    from inverse_audio_synthesis_amd.retrieval import l1_cdist
    N, M, K = 128, 4096, 44160
    q, b = torch.rand((N, K), device=dev) * 3.0, torch.rand((M, K), device=dev) * 3.0
    got = l1_cdist(q, b)
    g = torch.Generator().manual_seed(5)
    ns, ms = torch.randint(0, N, (64,), generator=g).to(dev), torch.randint(0, M, (64,), generator=g).to(dev)
    ref = (q[ns].double() - b[ms].double()).abs().sum(1) / K
    rel = ((got[ns, ms].double() - ref).abs() / ref).max().item()
    print(f"ias_l1_cdist (128, 4096, 44160) worst relative error over 64 pairs: {rel:.2e}")
    assert rel <= 1e-5


@pytest.mark.parametrize("K", [7, 4097, 44160])
def test_cdist_same_bits_wherever_a_pair_sits(lib, dev, K):
    """The pairs of a (5 x 7) problem, permuted among padding rows, in operands whose base pointers are moved by 1-3
    floats and under every launch shape (N = 5, 20, 70), give torch.equal distances."""
    from inverse_audio_synthesis_amd.retrieval import l1_cdist
    q, b = _rand((5, K), 31, dev), _rand((7, K), 32, dev)
    base = l1_cdist(q, b)
    for N2, M2, offq, offb, seed in ((5, 7, 1, 3, 1), (20, 300, 2, 1, 2), (70, 9, 3, 2, 3), (3 + 5, 1000, 1, 1, 4)):
        g = torch.Generator().manual_seed(seed)
        pn, pm = torch.randperm(N2, generator=g)[:5].to(dev), torch.randperm(M2, generator=g)[:7].to(dev)
        fq = _rand((offq + N2 * K,), 40 + seed, dev)
        fb = _rand((offb + M2 * K,), 50 + seed, dev)
        q2, b2 = fq.narrow(0, offq, N2 * K).view(N2, K), fb.narrow(0, offb, M2 * K).view(M2, K)
        q2[pn] = q
        b2[pm] = b
        d = l1_cdist(q2, b2)
        assert torch.equal(d[pn][:, pm], base), (N2, M2, offq, offb)
        assert torch.equal(l1_cdist(q2, b2), d)


def test_cdist_nonfinite_rows(lib, dev):
    from inverse_audio_synthesis_amd.retrieval import l1_cdist, rank_distances
    q, b = _rand((3, 5000), 61, dev), _rand((6, 5000), 62, dev)
    q[1, 4321] = float("nan")
    b[2, 17] = float("nan")
    b[4, 4999] = float("inf")
    d = l1_cdist(q, b)
    assert torch.isnan(d[1]).all() and torch.isnan(d[:, 2]).all() and not torch.isfinite(d[:, 4]).any()
    fin = torch.isfinite(d)
    assert fin[0].sum().item() == 4 and fin[2].sum().item() == 4
    idx = rank_distances(d)
    for n in (0, 2):
        order = idx[n].tolist()
        assert set(order[-2:]) == {2, 4} and order[-2:] == sorted(order[-2:])
        assert torch.equal(d[n, idx[n, :4]], d[n][fin[n]].sort().values)
    assert idx[1].tolist() == list(range(6))


def _voice(dev, B=4, sr=16000, sec=1.0):
    from inverse_audio_synthesis_amd.voice import SynthConfig, Voice
    return Voice(SynthConfig(batch_size=B, sample_rate=sr, buffer_size_seconds=sec, reproducible=False)).to(dev)


def _mel_kw():
    return dict(n_fft=1024, hop_length=512, n_mels=128, power=2.0)


@pytest.mark.parametrize("kind", ["mel", "stft257"])
def test_bank_recovers_its_own_voice_exactly(lib, dev, kind):
    from inverse_audio_synthesis_amd.retrieval import SpectralBank
    from inverse_audio_synthesis_amd.spectral import MelSpectrogramL1, STFTL1
    from inverse_audio_synthesis_amd.voice import sample_params01
    v = _voice(dev)
    loss = (MelSpectrogramL1(sample_rate=16000, **_mel_kw()) if kind == "mel" else
            STFTL1(n_fft=512, hop_length=128, power=1.0)).to(dev)
    stored = v.params01.clone()
    bank = SpectralBank(v, loss, [5, 6])
    assert bank.params01.shape == (8, 78) and bank.values.shape[0] == 8
    if kind == "stft257":
        assert bank.values.shape[2] == 257
    assert torch.equal(v.params01, stored)
    assert torch.equal(bank.params01[4:], sample_params01(4, 6).to(dev))
    j = 5                                                  # batch index 6, row 1
    own = v.render(sample_params01(4, 6).to(dev))[1]
    others = v.render(sample_params01(4, 99).to(dev))[:2]
    for pos in (0, 2):
        targets = torch.cat([others[:pos], own[None], others[pos:]])
        dist, idx = bank.nearest(target_audio=targets, k=3)
        assert dist.shape == (3, 3) and idx.dtype == torch.int64
        assert dist[pos, 0].item() == 0.0
        assert torch.equal(bank.values[idx[pos, 0]], loss.target(targets)[pos])
        assert idx[pos, 0].item() == j
        assert (dist[:, 1:] >= dist[:, :-1]).all()


def test_bank_distance_is_the_matchers_loss(lib, dev):
    from inverse_audio_synthesis_amd.match import SoundMatcher
    from inverse_audio_synthesis_amd.retrieval import SpectralBank
    v = _voice(dev)
    matcher = SoundMatcher(v, mel_kwargs=_mel_kw())
    bank = SpectralBank(v, matcher.loss, [3])               # bank item m rendered at row m
    target = v.render(so.sample_params01(so.VoiceConfig(4, 16000, 1.0), 11).to(dev))
    d = bank.distances(matcher.loss.target(target))
    for perm in ([0, 1, 2, 3], [2, 0, 3, 1]):              # target perm[r] placed at the row of bank item r
        res = matcher.fit(target[perm], init_params01=bank.params01, steps=0)
        want = d[perm, torch.arange(4)]
        rel = ((res.initial_loss.double() - want.double()).abs() / want.double()).max().item()
        print(f"bank distance vs matcher initial loss: worst relative difference {rel:.2e}")
        assert rel <= 1e-5


def test_fit_keeps_the_best_start(lib, dev):
    from inverse_audio_synthesis_amd import voice_spec as S
    from inverse_audio_synthesis_amd.match import SoundMatcher
    v = _voice(dev)
    m = SoundMatcher(v, mel_kwargs=_mel_kw(), lr=0.02)
    target = v.render(so.sample_params01(so.VoiceConfig(4, 16000, 1.0), 21).to(dev))[:3]
    init = torch.rand((3, 2, 78), generator=torch.Generator().manual_seed(8)).to(dev)
    res = m.fit(target, init_params01=init, steps=3, return_audio=True)
    flat = m.fit(target.repeat_interleave(2, 0), init_params01=init.reshape(6, 78), steps=3, return_audio=True)
    sl = flat.loss.reshape(3, 2)
    assert torch.equal(res.start_loss, sl) and torch.equal(res.start_initial_loss, flat.initial_loss.reshape(3, 2))
    for n in range(3):
        s = 0 if sl[n, 0] <= sl[n, 1] else 1
        r = 2 * n + s
        assert res.start[n].item() == s
        assert torch.equal(res.params01[n], flat.params01[r]) and torch.equal(res.loss[n], flat.loss[r])
        assert torch.equal(res.initial_loss[n], flat.initial_loss[r]) and torch.equal(res.skipped[n], flat.skipped[r])
        assert torch.equal(res.audio[n], flat.audio[r])
    two = m.fit(target, init_params01=init[:, 0], steps=3)      # a 2-D start is as before: no start fields
    assert two.start is None and two.start_loss is None and two.start_initial_loss is None and two.loss.shape == (3,)

    # noise silenced: a start at the target's own parameters renders the target at any row -> loss exactly 0
    noise = S.INDEX[("mixer", "noise")]
    tp = so.sample_params01(so.VoiceConfig(4, 16000, 1.0), 22).to(dev)
    tp[:, noise] = 0.0
    target = v.render(tp)[:2]
    starts = torch.rand((2, 3, 78), generator=torch.Generator().manual_seed(9)).to(dev)
    starts[:, :, noise] = 0.0
    starts[0, 1] = tp[0]
    starts[0, 2] = tp[0]
    starts[1, 2] = tp[1]
    m0 = SoundMatcher(v, mel_kwargs=_mel_kw(), lr=0.02, frozen=[("mixer", "noise")])
    res = m0.fit(target, init_params01=starts, steps=4)
    assert res.loss.tolist() == [0.0, 0.0] and res.start.tolist() == [1, 2]
    assert torch.equal(res.params01[0], tp[0]) and torch.equal(res.params01[1], tp[1])


def _write_wav(path, x, sr):
    pcm = np.round(np.clip(x, -1, 1) * 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(pcm.tobytes())


def test_match_audio_bank_init(lib, dev, tmp_path):
    from conftest import ROOT
    v = _voice(dev, B=2)
    audio = v.render(so.sample_params01(so.VoiceConfig(2, 16000, 1.0), 13).to(dev)).cpu().numpy()
    _write_wav(tmp_path / "a.wav", audio[0], 16000)
    _write_wav(tmp_path / "b.wav", audio[1][:12000], 16000)
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "match_audio.py"), str(tmp_path / "a.wav"), str(tmp_path / "b.wav"),
           "torchsynth.rate=16000", "torchsynth.buffer_size_seconds=1.0", "--steps", "3", "--out", str(out),
           "--init", "bank", "--bank-batches", "2", "--starts", "2"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "spectral bank of 256 voices" in r.stdout
    for name in ("a", "b"):
        rec = json.load(open(out / f"{name}.params.json"))
        assert rec["init"] == "bank" and 0 <= rec["bank_index"] < 256 and rec["bank_distance"] >= 0.0
        assert rec["start"] in (0, 1) and len(rec["params"]) == 78
        assert {"input", "loss_kind", "steps", "initial_loss", "final_loss", "skipped"} <= set(rec)
        assert rec["final_loss"] <= rec["initial_loss"]
        with wave.open(str(out / f"{name}.match.wav"), "rb") as w:
            assert w.getnframes() == 16000 and w.getframerate() == 16000

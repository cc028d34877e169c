"""Evolutionary search stage on the GPU: ias_evolve_sample against the numpy model (tests/evolve_model.py) and its
independence of the cut, ias_evolve_update against the model, evolve_search end to end (every elite's distance reproduced
bit for bit from its parameters and index), the search lowering the loss, match_audio.py --evolve, and the search loop
itself (``evolve.cross_entropy_search``) with a scorer written in torch."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

from oracle import synth_oracle as so

import evolve_model as em

pytestmark = pytest.mark.gpu

EMPTY = torch.iinfo(torch.int64).max
SEED = 0x1234567890ABCDEF


def _sample(mean, sigma, free, M, dev, **kw):
    from inverse_audio_synthesis_amd.evolve import evolve_sample
    N, P = mean.shape
    out = torch.full((N, M, P), -7.0, dtype=torch.float32, device=dev)
    return evolve_sample(mean, sigma, free, out=out, **kw)


def _inputs(N, P, dev, seed):
    """Means that reach both walls (so the clamp acts), sigma in [0, 0.5], about a third of the columns frozen."""
    g = torch.Generator().manual_seed(seed)
    mean = torch.rand((N, P), generator=g)
    edge = torch.rand((N, P), generator=g)
    mean = torch.where(edge < 0.2, mean * 0.02, torch.where(edge > 0.8, 1.0 - mean * 0.02, mean))
    sigma = torch.rand((N, P), generator=g) * 0.5
    sigma[:, ::5] = 0.5
    free = (torch.rand(P, generator=g) > 0.33).to(torch.uint8)
    free[0] = 1
    if P > 1:
        free[P - 1] = 0
    return mean.to(dev), sigma.to(dev), free.to(dev)


@pytest.mark.parametrize("N,M,P", [(1, 1, 1), (3, 5, 78), (2, 130, 128), (5, 64, 7)])
def test_sampler_matches_the_model(lib, dev, N, M, P):
    """|out - model| <= 2e-5 sigma + 1.2e-7: the u values are exact, |z| <= 5.77, a few ulp in logf, sqrtf and the
    pi-scaled sine / cosine keep |dz| below 2e-5, the clamp is 1-Lipschitz, and the rounded product and sum of a value
    that ends inside [0, 1] are each off by at most 2^-25."""
    mean, sigma, free = _inputs(N, P, dev, 100 + P)
    kw = dict(n_base=2, m_base=(1 << 32) - M - 1, seed=SEED, generation=3)
    out = _sample(mean, sigma, free, M, dev, **kw)
    ref = em.sample(mean.cpu().numpy(), sigma.cpu().numpy(), free.cpu().numpy(), M, **kw)
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
    tol = 2e-5 * sigma.cpu().numpy().astype(np.float64)[:, None, :] + 1.2e-7
    print(f"ias_evolve_sample ({N}, {M}, {P}): worst |out - model| {err.max():.3e}, worst err / tol {(err / tol).max():.3f}")
    assert (err <= tol).all()
    frozen = free == 0
    assert torch.equal(out[:, :, frozen], mean[:, None, frozen].expand(N, M, int(frozen.sum())))
    o = out[:, :, free != 0]
    assert ((o >= 0.0) & (o <= 1.0)).all()
    if N * M * P > 1000:
        assert (o == 0.0).any() and (o == 1.0).any()       # the clamp acted at both walls


def test_sampler_draws_standard_normals(lib, dev):
    """10^5 draws at mean 0.5, sigma 2^-6 (far from the walls; z = 64 (out - 0.5) up to 4e-6): mean and variance of z
    within 0.02 of 0 and 1 (their standard errors are 0.003 and 0.0045)."""
    N, M, P = 2, 500, 100
    mean = torch.full((N, P), 0.5, device=dev)
    sigma = torch.full((N, P), 2.0 ** -6, device=dev)
    free = torch.ones(P, dtype=torch.uint8, device=dev)
    z = (_sample(mean, sigma, free, M, dev, seed=11, generation=0).double() - 0.5) * 64.0
    m, v = z.mean().item(), z.var(unbiased=False).item()
    print(f"ias_evolve_sample: {z.numel()} draws, mean {m:+.5f}, variance {v:.5f}, max |z| {z.abs().max().item():.3f}")
    assert abs(m) <= 0.02 and abs(v - 1.0) <= 0.02
    zr = em.normals(N, M, P, 0, 0, 11, 0)
    assert np.abs(z.cpu().numpy() - zr).max() <= 2e-5 + 4e-6


def test_sampler_does_not_depend_on_the_cut(lib, dev):
    N, M, P = 3, 130, 78
    mean, sigma, free = _inputs(N, P, dev, 7)
    kw = dict(seed=SEED, generation=5)
    whole = _sample(mean, sigma, free, M, dev, **kw)
    assert torch.equal(_sample(mean, sigma, free, M, dev, **kw), whole)              # run to run
    for n in range(N):                                                             # sound by sound
        assert torch.equal(_sample(mean[n:n + 1], sigma[n:n + 1], free, M, dev, n_base=n, **kw), whole[n:n + 1])
    m0 = 0
    for piece in (1, 7, 122):                                                      # candidates in pieces
        part = _sample(mean, sigma, free, piece, dev, m_base=m0, **kw)
        assert torch.equal(part, whole[:, m0:m0 + piece]), piece
        m0 += piece
    assert m0 == M
    fr = free != 0
    other = _sample(mean, sigma, free, M, dev, seed=SEED + 1, generation=5)
    assert not torch.equal(other[:, :, fr], whole[:, :, fr])
    other = _sample(mean, sigma, free, M, dev, seed=SEED, generation=6)
    assert not torch.equal(other[:, :, fr], whole[:, :, fr])
    other = _sample(mean, sigma, free, M, dev, seed=SEED ^ (1 << 40), generation=5)  # the key's high word counts
    assert not torch.equal(other[:, :, fr], whole[:, :, fr])


@pytest.mark.parametrize("P", [7, 78])
def test_update_matches_the_model(lib, dev, P):
    """Hand-built state, N = 3, k = 5, M = 8, base = 16.  Sound 0: elites from the block (17, 23), from prev (3, 9) and an
    empty slot; 23 carries a NaN distance and 9 a +inf one, so two elites are valid.  Sound 1: no finite elite.  Sound 2:
    five valid elites.  A second call points one slot of sound 2 at an index found nowhere."""
    from inverse_audio_synthesis_amd.evolve import evolve_update
    N, k, M, base = 3, 5, 8, 16
    nan, inf = float("nan"), float("inf")
    g = torch.Generator().manual_seed(P)
    pop = torch.rand((N, M, P), generator=g)
    prev_params = torch.rand((N, k, P), generator=g)
    mean0, sigma0 = torch.rand((N, P), generator=g), torch.rand((N, P), generator=g) * 0.4 + 0.01
    free = (torch.rand(P, generator=g) > 0.3).to(torch.uint8)
    free[0], free[P - 1] = 0, 1
    pop[2, 4:7, P - 1] = 0.25                              # a column on which sound 2's elites agree: sigma meets sigma_min
    prev_params[2, :2, P - 1] = 0.25
    sigma0[2, P - 1] = 0.1
    elite_idx = torch.tensor([[17, 3, 23, 9, EMPTY], [16, 2, EMPTY, EMPTY, EMPTY], [20, 21, 4, 22, 6]])
    elite_dist = torch.tensor([[0.1, 0.2, nan, inf, inf], [nan, inf, inf, inf, inf], [0.01, 0.02, 0.03, 0.5, 0.7]])
    prev_idx = torch.tensor([[3, 9, 5, 1, 0], [2, EMPTY, EMPTY, EMPTY, EMPTY], [6, 4, 7, 8, EMPTY]])
    alpha, smin, smax = 0.7, 0.05, 0.3

    for lost in (False, True):
        ei, ed = elite_idx.clone(), elite_dist.clone()
        if lost:
            ei[2, 3], ed[2, 3] = 99, inf
        mean, sigma = mean0.clone().to(dev), sigma0.clone().to(dev)
        ep = torch.full((N, k, P), -3.0, device=dev)
        evolve_update(pop.to(dev), base, ed.to(dev), ei.to(dev), prev_idx.to(dev), prev_params.to(dev), ep, mean, sigma,
                      free.to(dev), alpha, smin, smax)
        rp, rm, rs = em.update(pop.numpy(), base, ed.numpy(), ei.numpy(), prev_idx.numpy(), prev_params.numpy(),
                               mean0.numpy(), sigma0.numpy(), free.numpy(), alpha, smin, smax)
        got = ep.cpu()
        want, real = torch.from_numpy(rp), ~torch.isnan(got)
        assert torch.equal(got.view(torch.int32)[real], want.view(torch.int32)[real])
        assert torch.equal(torch.isnan(got), torch.isnan(want))
        assert torch.isnan(got[2, 3]).all().item() == lost and torch.isnan(got).sum().item() == (P if lost else 0)
        assert torch.equal(got[0, 0], pop[0, 1]) and torch.equal(got[0, 1], prev_params[0, 0])
        assert torch.equal(got[0, 3], prev_params[0, 1]) and (got[0, 4] == 0).all() and (got[1, 2:] == 0).all()
        assert torch.equal(mean.cpu(), torch.from_numpy(rm))
        ulps = (sigma.cpu().view(torch.int32) - torch.from_numpy(rs).view(torch.int32)).abs().max().item()
        print(f"ias_evolve_update P = {P}{' (lost index)' if lost else ''}: sigma within {ulps} ulp of the model")
        assert ulps <= 1
        # the sound without a finite elite and the frozen columns keep their bits
        assert torch.equal(mean.cpu()[1], mean0[1]) and torch.equal(sigma.cpu()[1], sigma0[1])
        fz = free == 0
        assert torch.equal(mean.cpu()[:, fz], mean0[:, fz]) and torch.equal(sigma.cpu()[:, fz], sigma0[:, fz])
        moved = free != 0
        assert not torch.equal(mean.cpu()[0, moved], mean0[0, moved])
        sg = sigma.cpu()[[0, 2]][:, moved]
        assert (sg >= float(np.float32(smin))).all() and (sg <= float(np.float32(smax))).all()
        assert sigma.cpu()[2, P - 1].item() == float(np.float32(smin)) and (sg == float(np.float32(smax))).any()


def _voice(dev, B=4, sr=16000, sec=1.0):
    from inverse_audio_synthesis_amd.voice import SynthConfig, Voice
    return Voice(SynthConfig(batch_size=B, sample_rate=sr, buffer_size_seconds=sec, reproducible=False)).to(dev)


def _mel_kw():
    return dict(n_fft=1024, hop_length=512, n_mels=128, power=2.0)


def _mel(dev):
    from inverse_audio_synthesis_amd.spectral import MelSpectrogramL1
    return MelSpectrogramL1(sample_rate=16000, **_mel_kw()).to(dev)


FIELDS = ("params01", "dist", "idx", "mean", "sigma", "history")


def test_search_end_to_end(lib, dev):
    """B = 4, N = 3, M = 8, k = 3, G = 4."""
    from inverse_audio_synthesis_amd import voice_spec as S
    from inverse_audio_synthesis_amd.evolve import evolve_search
    from inverse_audio_synthesis_amd.retrieval import l1_cdist, rank_distances
    v, loss = _voice(dev), _mel(dev)
    B, N, M, k, G = 4, 3, 8, 3, 4
    stored = v.params01.clone()
    target = v.render(so.sample_params01(so.VoiceConfig(4, 16000, 1.0), 21).to(dev))[:N]
    init = torch.rand((N, 78), generator=torch.Generator().manual_seed(8)).to(dev)
    frozen = [("mixer", "noise"), ("keyboard", "midi_f0"), ("vco_1", "tuning")]
    kw = dict(target_audio=target, generations=G, population=M, elites=k, init_params01=init, seed=5, frozen=frozen)
    a = evolve_search(v, loss, **kw)
    b = evolve_search(v, loss, **kw)
    for f in FIELDS:
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert torch.equal(v.params01, stored)
    assert a.params01.shape == (N, k, 78) and a.dist.shape == (N, k) and a.idx.dtype == torch.int64
    assert a.history.shape == (G, N) and a.mean.shape == a.sigma.shape == (N, 78)
    assert not torch.equal(evolve_search(v, loss, **dict(kw, seed=6)).idx, a.idx)
    print("evolve_search history (G x N):", [[f"{x:.4f}" for x in row] for row in a.history.tolist()])
    assert (a.history[1:] <= a.history[:-1]).all()
    assert torch.equal(a.history[-1], a.dist[:, 0])
    assert torch.isfinite(a.dist).all() and ((a.idx >= 0) & (a.idx < G * M)).all()
    assert torch.equal(rank_distances(a.dist), torch.arange(k, device=dev).expand(N, k))
    # every elite again: its parameters at its own row, the other rows at the centre -> the same distance bits
    q = loss.target(target).reshape(N, -1)
    for n in range(N):
        for e in range(k):
            row = int(a.idx[n, e]) % M % B
            p = torch.full((B, 78), 0.5, device=dev)
            p[row] = a.params01[n, e]
            vals = loss.target(v.render(p, normalize=True))[row:row + 1].reshape(1, -1)
            d = l1_cdist(q[n:n + 1], vals)
            assert torch.equal(d.view(torch.int32)[0, 0], a.dist.view(torch.int32)[n, e]), (n, e, d.item(), a.dist[n, e])
    cols = [S.INDEX[f] for f in frozen]
    assert torch.equal(a.params01[:, :, cols], init[:, None, cols].expand(N, k, len(cols)))
    assert torch.equal(a.mean[:, cols], init[:, cols])
    assert ((a.params01 >= 0) & (a.params01 <= 1)).all()

    # a start at the target's own parameters with the noise silenced is found, kept and ranked first
    noise = S.INDEX[("mixer", "noise")]
    tp = so.sample_params01(so.VoiceConfig(4, 16000, 1.0), 22).to(dev)
    tp[:, noise] = 0.0
    target = v.render(tp)[:N]
    starts = torch.rand((N, 2, 78), generator=torch.Generator().manual_seed(9)).to(dev)
    starts[:, :, noise] = 0.0
    starts[:, 1] = tp[:N]
    r = evolve_search(v, loss, target_audio=target, generations=G, population=M, elites=k, init_params01=starts, seed=5,
                      frozen=[("mixer", "noise")])
    assert r.dist[:, 0].tolist() == [0.0] * N and r.idx[:, 0].tolist() == [1] * N
    assert torch.equal(r.params01[:, 0], tp[:N])
    assert (r.history == 0.0).all()


def test_a_start_scores_as_its_bank_voice(lib, dev):
    """B = 4, N = 2, M = 8, G = 1, k = 2, S = 2.  The starts are voices of a two-batch ``SpectralBank``, start s a bank item
    of row s, so it is rendered at the row it had in the bank: its distance among the elites is the bank's distance for
    that pair, bit for bit (one scoring path).  Each sound's target is one of its starts' own render at 0.97 of its
    level, so that this start is an elite with a distance above 0; the other start is checked when it is an elite too."""
    from inverse_audio_synthesis_amd.evolve import evolve_search
    from inverse_audio_synthesis_amd.retrieval import SpectralBank
    v, loss = _voice(dev), _mel(dev)
    B, N, M, k = 4, 2, 8, 2
    bank = SpectralBank(v, loss, [3, 9])
    item = torch.tensor([[4, 1], [0, 5]], device=dev)       # start s of sound n: a bank item m with m % B == s
    near = [0, 1]                                           # the start sound n's target is made from
    audio = torch.cat([v.render(bank.params01[j * B:(j + 1) * B], normalize=True) for j in range(2)])
    target = 0.97 * audio[[int(item[n, near[n]]) for n in range(N)]]
    r = evolve_search(v, loss, target_audio=target, generations=1, population=M, elites=k,
                      init_params01=bank.params01[item], seed=5)
    d = bank.distances(loss.target(target))
    for n in range(N):
        elites = r.idx[n].tolist()
        assert near[n] in elites, (n, elites, r.dist[n].tolist())
        for e, m in enumerate(elites):
            if m < 2:                                       # candidate m < S of generation 0 is start m
                bm = int(item[n, m])
                got, want = r.dist.view(torch.int32)[n, e], d.view(torch.int32)[n, bm]
                assert torch.equal(got, want), (n, m, r.dist[n, e], d[n, bm])
                assert m != near[n] or 0.0 < float(d[n, bm]) < float("inf")


def test_search_improves_the_fit(lib, dev):
    """Only the three mixer levels are free (tests/test_match_gpu.py::test_matcher_descends_on_mixer_levels), M = 32,
    G = 10, seed 0, the other settings at their defaults: the best distance after the last generation is strictly below
    the best of generation 0 for every sound (measured on an MI355X: history[-1] / history[0] = 0.4780, 0.0082, 0.0257,
    0.0018 for the four sounds).  Only the strict improvement is asserted."""
    from inverse_audio_synthesis_amd import voice_spec as S
    from inverse_audio_synthesis_amd.match import SoundMatcher
    v = _voice(dev)
    tp = so.sample_params01(so.VoiceConfig(4, 16000, 1.0), 7).to(dev)
    target = v.render(tp)
    free = [("mixer", n) for n in ("vco_1", "vco_2", "noise")]
    init = tp.clone()
    init[:, [S.INDEX[f] for f in free]] = 0.5
    frozen = [(m, n) for (m, n, *_r) in S.PARAMS if (m, n) not in free]
    matcher = SoundMatcher(v, mel_kwargs=_mel_kw(), frozen=frozen)
    r = matcher.search(target, generations=10, population=32, init_params01=init, seed=0)
    ratio = (r.history[-1].double() / r.history[0].double()).tolist()
    print("evolve_search on the mixer levels: history[-1] / history[0] per sound:", [f"{x:.4f}" for x in ratio])
    assert (r.history[-1] < r.history[0]).all(), ratio
    cols = [S.INDEX[f] for f in frozen]
    assert torch.equal(r.params01[:, :, cols], tp[:, None, cols].expand(4, 8, len(cols)))
    res = matcher.fit(target, init_params01=r.params01[:, :2].contiguous(), steps=2)      # the elites are starts for the fit
    assert res.loss.shape == (4,) and torch.isfinite(res.loss).all()


@pytest.mark.parametrize("P", [6, 78])
def test_loop_with_a_torch_scorer(lib, dev, P):
    """N = 3, M = 8, k = 3, G = 4 on the device primitives at the two widths the product uses (P = 6: the sampler's last
    group of four columns is partial), scored by mean |candidate - hidden vector|."""
    from inverse_audio_synthesis_amd.evolve import cross_entropy_search
    N, M, k, G = 3, 8, 3, 4
    g = torch.Generator().manual_seed(P)
    q = torch.rand((N, P), generator=g).to(dev)
    starts = torch.rand((N, 2, P), generator=g).to(dev)
    frozen = [1, P - 2]
    free = torch.ones(P, dtype=torch.uint8)
    free[frozen] = 0

    def score(_g, pop, out):
        out.copy_((pop - q[:, None]).abs().mean(-1))

    def search(starts, seed=5):
        return cross_entropy_search(starts, free.to(dev), score, G, M, k, 0.2, 0.7, 0.005, 0.5, seed)
    a, b = search(starts[:, :1].contiguous()), search(starts[:, :1].contiguous())
    for f in FIELDS:
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert not torch.equal(search(starts[:, :1].contiguous(), seed=6).idx, a.idx)
    assert a.params01.shape == (N, k, P) and a.history.shape == (G, N)
    assert (a.history[1:] <= a.history[:-1]).all() and torch.equal(a.history[-1], a.dist[:, 0])
    assert torch.isfinite(a.dist).all() and ((a.idx >= 0) & (a.idx < G * M)).all()
    assert torch.equal(a.params01[:, :, frozen], starts[:, :1, frozen].expand(N, k, 2))
    assert torch.equal(a.mean[:, frozen], starts[:, 0, frozen])
    # a start at the hidden vector, at slot 1 of 2, is found, kept and ranked first
    planted = starts.clone()
    planted[:, 1] = q
    r = search(planted)
    assert r.dist[:, 0].tolist() == [0.0] * N and r.idx[:, 0].tolist() == [1] * N
    assert torch.equal(r.params01[:, 0], q) and (r.history == 0.0).all()


def _write_wav(path, x, sr):
    pcm = np.round(np.clip(x, -1, 1) * 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(pcm.tobytes())


def test_match_audio_evolve(lib, dev, tmp_path):
    from conftest import ROOT
    v = _voice(dev, B=2)
    audio = v.render(so.sample_params01(so.VoiceConfig(2, 16000, 1.0), 13).to(dev)).cpu().numpy()
    _write_wav(tmp_path / "a.wav", audio[0], 16000)
    _write_wav(tmp_path / "b.wav", audio[1][:12000], 16000)
    base = [sys.executable, os.path.join(ROOT, "match_audio.py"), str(tmp_path / "a.wav"), str(tmp_path / "b.wav"),
            "torchsynth.rate=16000", "torchsynth.buffer_size_seconds=1.0", "--steps", "3", "--init", "bank",
            "--bank-batches", "2", "--starts", "2"]
    evo = ["--evolve", "3", "--evolve-population", "128", "--evolve-elites", "4", "--seed", "3"]
    for name, extra in (("with", evo), ("without", [])):
        out = tmp_path / name
        r = subprocess.run(base + ["--out", str(out)] + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-4000:]
        assert ("evolutionary search, 3 generations of 128" in r.stdout) == bool(extra)
        for wav in ("a", "b"):
            rec = json.load(open(out / f"{wav}.params.json"))
            assert rec["final_loss"] <= rec["initial_loss"] and rec["start"] in (0, 1) and len(rec["params"]) == 78
            if extra:
                assert rec["evolve_generations"] == 3 and rec["evolve_population"] == 128
                assert 0 <= rec["evolve_index"] < 3 * 128 and rec["evolve_distance"] >= 0.0
                assert "bank_index" not in rec
            else:
                assert not [key for key in rec if key.startswith("evolve")]
                assert 0 <= rec["bank_index"] < 256

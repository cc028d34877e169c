"""Streamed spectral bank search on the GPU: ias_topk_merge against the full sort it replaces (ties, non-finite values,
uneven blocks in any order, a strided block, fewer candidates than k), its refusals, SpectralBank.search against the
resident bank bit for bit, its memory (one chunk, not the bank) and match_audio.py --bank-stream."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

from test_bank_gpu import _mel_kw, _voice, _write_wav

pytestmark = pytest.mark.gpu

INT64_MAX = torch.iinfo(torch.int64).max


def _fresh(N, k, dev):
    return (torch.full((N, k), float("inf"), dtype=torch.float32, device=dev),
            torch.full((N, k), INT64_MAX, dtype=torch.int64, device=dev))


def _bits(x):
    return x.contiguous().view(torch.int32)


# a representative cross product of N in {1, 3, 130}, M in {1, 5, 257, 1000, 5000}, k in {1, 4, 64}: every value of each,
# fewer candidates than k ((3, 5, 64), (130, 1, 4)), one lane's share of one and of many columns, and rows longer than the
# 4096 keys a workgroup stages in LDS
MERGE_CASES = [(1, 1, 1), (3, 5, 64), (130, 257, 4), (3, 1000, 64), (130, 5000, 4), (1, 5000, 64), (130, 1, 4),
               (3, 257, 1), (1, 1000, 4)]


@pytest.mark.parametrize("nonfinite", [False, True], ids=["ties", "ties+nonfinite"])
@pytest.mark.parametrize("N,M,k", MERGE_CASES, ids=[f"{n}x{m}k{k}" for n, m, k in MERGE_CASES])
def test_merge_equals_the_full_sort(lib, dev, N, M, k, nonfinite):
    from inverse_audio_synthesis_amd.retrieval import rank_distances, topk_merge
    g = torch.Generator().manual_seed(100 * N + M + k)
    d = torch.randint(0, 4, (N, M), generator=g).float()
    if nonfinite:                                           # about 5 % of the entries, a third each
        u = torch.rand((N, M), generator=g)
        d[u < 0.05] = float("nan")
        d[u < 0.0333] = float("inf")
        d[u < 0.0167] = float("-inf")
    d = d.to(dev)
    kk = min(k, M)
    want_idx = rank_distances(d)[:, :kk]
    want_dist = torch.gather(d, 1, want_idx)

    def check(bd, bi, what):
        assert torch.equal(bi[:, :kk], want_idx), what
        assert torch.equal(_bits(bd[:, :kk]), _bits(want_dist)), what
        assert (bi[:, kk:] == INT64_MAX).all() and (_bits(bd[:, kk:]) == 0x7f800000).all(), what

    # uneven blocks (1, 7, 256, the rest) in a shuffled order, the last of them a view with row stride M + 3
    cuts, m0 = [], 0
    for w in (1, 7, 256, M):
        if m0 < M:
            cuts.append((m0, min(M, m0 + w)))
            m0 = cuts[-1][1]
    padded = torch.full((N, M + 3), -7.0, device=dev)
    padded[:, :M] = d
    bd, bi = _fresh(N, k, dev)
    for j in torch.randperm(len(cuts), generator=g).tolist():
        a, b = cuts[j]
        block = padded[:, a:b] if j == len(cuts) - 1 else d[:, a:b].contiguous()
        topk_merge(block, a, bd, bi)
    check(bd, bi, "blocks")

    one_d, one_i = _fresh(N, k, dev)
    topk_merge(d, 0, one_d, one_i)
    check(one_d, one_i, "one shot")
    assert torch.equal(one_i, bi) and torch.equal(_bits(one_d), _bits(bd))

    strided_d, strided_i = _fresh(N, k, dev)
    topk_merge(padded[:, :M], 0, strided_d, strided_i)
    assert torch.equal(strided_i, bi) and torch.equal(_bits(strided_d), _bits(bd))


def test_merge_keeps_global_indices_past_2_to_the_32(lib, dev):
    """``base`` is a 64-bit offset: blocks of a bank larger than 2^32 voices keep their indices and their order."""
    from inverse_audio_synthesis_amd.retrieval import topk_merge
    d = torch.tensor([[2.0, 1.0, 1.0], [0.0, float("nan"), 0.0]], device=dev)
    bd, bi = _fresh(2, 4, dev)
    hi = (1 << 33) + 5
    topk_merge(d, hi, bd, bi)
    topk_merge(d, 10, bd, bi)
    assert bi.tolist() == [[11, 12, hi + 1, hi + 2], [10, 12, hi, hi + 2]]
    assert bd.tolist() == [[1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0]]


def test_merge_refusals_leave_the_state_alone(lib, dev):
    N, M, k = 3, 5, 4
    d = torch.rand((N, M), device=dev)
    bd, bi = _fresh(N, k, dev)
    bd[:, 0], bi[:, 0] = 0.25, 2
    keep_d, keep_i = bd.clone(), bi.clone()
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(N=N, M=M, ld=M, base=0, k=k, dist=d):
        return lib.ias_topk_merge(p(dist) if dist is not None else None, N, M, ld, base, k, p(bd), p(bi), None)
    for kw in (dict(k=0), dict(k=65), dict(N=0), dict(ld=M - 1), dict(base=-1), dict(M=0), dict(dist=None)):
        assert call(**kw) == -1, kw                          # IAS_ERR_ARG
    assert call(N=65536) == -2                               # IAS_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(bi, keep_i) and torch.equal(_bits(bd), _bits(keep_d))
    assert call(base=100) == 0


def _losses(dev):
    from inverse_audio_synthesis_amd.spectral import MelSpectrogramL1, STFTL1
    return {"mel": MelSpectrogramL1(sample_rate=16000, **_mel_kw()).to(dev),
            "stft257": STFTL1(n_fft=512, hop_length=128, power=1.0).to(dev)}


BATCHES = [7, 2, 9, 2, 4, 11, 3]                            # batch 2 twice: exact ties, the lower position first


@pytest.mark.parametrize("kind", ["mel", "stft257"])
def test_streamed_search_equals_the_resident_bank(lib, dev, kind):
    from inverse_audio_synthesis_amd.retrieval import SpectralBank
    from inverse_audio_synthesis_amd.voice import sample_params01
    v = _voice(dev)
    loss = _losses(dev)[kind]
    targets = _voice(dev, B=8).render(sample_params01(8, 20).to(dev))[:5].clone()
    targets[3, 1234] = float("nan")
    stored = v.params01.clone()
    bank = SpectralBank(v, loss, BATCHES)
    tv = loss.target(targets)
    for k in (1, 3, 28, 40):
        want_dist, want_idx = bank.nearest(target_values=tv, k=k)
        if k >= 8:                                          # the tie: both copies of batch 2, the lower position first
            pos = {m: c for c, m in enumerate(want_idx[0].tolist())}
            assert all(pos[4 + r] < pos[12 + r] for r in range(4) if 4 + r in pos and 12 + r in pos)
        assert torch.isnan(want_dist[3]).all() and want_idx[3].tolist() == list(range(min(k, 28)))
        for chunk in (1, 2, 5, 7, 100):
            dist, idx, params = SpectralBank.search(v, loss, BATCHES, target_values=tv, k=k, chunk_batches=chunk)
            assert idx.dtype == torch.int64 and dist.dtype == torch.float32 and dist.shape == (5, min(k, 28))
            assert torch.equal(idx, want_idx), (k, chunk)
            assert torch.equal(_bits(dist), _bits(want_dist)), (k, chunk)
            assert params.shape == (5, min(k, 28), 78) and torch.equal(params, bank.params01[idx]), (k, chunk)
    dist, idx, _p = SpectralBank.search(v, loss, BATCHES, target_audio=targets, k=3, chunk_batches=2)
    want_dist, want_idx = bank.nearest(target_audio=targets, k=3)
    assert torch.equal(idx, want_idx) and torch.equal(_bits(dist), _bits(want_dist))
    assert torch.equal(v.params01, stored)


def test_streamed_search_refuses_multi_resolution_loss(lib, dev):
    from inverse_audio_synthesis_amd.retrieval import SpectralBank
    from inverse_audio_synthesis_amd.spectral import MultiResolutionSTFTLoss
    v = _voice(dev)
    with pytest.raises(ValueError, match="mel bank"):
        SpectralBank.search(v, MultiResolutionSTFTLoss().to(dev), [0], target_audio=v.render())


def test_streamed_search_holds_one_chunk_not_the_bank(lib, dev):
    from inverse_audio_synthesis_amd.retrieval import SpectralBank
    v = _voice(dev)
    loss = _losses(dev)["stft257"]
    targets = v.render()
    nb = 16
    SpectralBank.search(v, loss, range(nb), target_audio=targets, k=2, chunk_batches=1)     # tables, scratch, first use
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    SpectralBank.search(v, loss, range(nb), target_audio=targets, k=2, chunk_batches=1)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    bank_bytes = SpectralBank.nbytes(v, loss, nb)
    print(f"streamed search of {nb} batches, one per chunk: peak growth {grown} bytes, the bank's values {bank_bytes}")
    assert grown < bank_bytes / 2


def test_match_audio_bank_stream(lib, dev, tmp_path):
    from conftest import ROOT
    from oracle import synth_oracle as so
    v = _voice(dev, B=2)
    audio = v.render(so.sample_params01(so.VoiceConfig(2, 16000, 1.0), 13).to(dev)).cpu().numpy()
    _write_wav(tmp_path / "a.wav", audio[0], 16000)
    _write_wav(tmp_path / "b.wav", audio[1][:12000], 16000)
    recs = {}
    for name, extra in (("resident", []), ("stream", ["--bank-stream", "2"])):
        out = tmp_path / name
        cmd = [sys.executable, os.path.join(ROOT, "match_audio.py"), str(tmp_path / "a.wav"), str(tmp_path / "b.wav"),
               "torchsynth.rate=16000", "torchsynth.buffer_size_seconds=1.0", "--steps", "2", "--out", str(out),
               "--init", "bank", "--bank-batches", "3", "--starts", "2"] + extra
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-4000:]
        if extra:
            assert "spectral bank of 384 voices in chunks of 256" in r.stdout
        recs[name] = [json.load(open(out / f"{w}.params.json")) for w in ("a", "b")]
    for a, b in zip(recs["resident"], recs["stream"]):
        for key in ("bank_index", "bank_distance", "start"):
            assert a[key] == b[key], key
        assert 0 <= b["bank_index"] < 384

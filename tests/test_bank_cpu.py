"""Spectral bank without a GPU: the C ABI's host-side refusals, the ranking rule and match_audio.py's new flags."""
import math

import pytest
import torch


def test_cdist_workspace_refuses_bad_sizes(lib):
    for N, M, K in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 4, 4), (4, -1, 4), (4, 4, -7)):
        assert lib.ias_l1_cdist_workspace_bytes(N, M, K) < 0, (N, M, K)
    # one fp64 partial per pair and 4096-element chunk
    assert lib.ias_l1_cdist_workspace_bytes(1, 1, 1) == 8
    assert lib.ias_l1_cdist_workspace_bytes(3, 5, 4096) == 3 * 5 * 8
    assert lib.ias_l1_cdist_workspace_bytes(3, 5, 4097) == 3 * 5 * 2 * 8
    assert lib.ias_l1_cdist_workspace_bytes(128, 4096, 44160) == 128 * 4096 * 11 * 8
    # bad arguments are refused before anything is launched
    assert lib.ias_l1_cdist(None, None, 1, 1, 1, None, None, None) < 0


def test_rank_is_stable_with_nonfinite_last():
    from inverse_audio_synthesis_amd.retrieval import rank_distances
    nan, inf = math.nan, math.inf
    d = torch.tensor([[1.0, nan, 0.5, 1.0, inf, 0.5, -inf, 0.0],
                      [2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0],
                      [nan, nan, 3.0, nan, -1.0, inf, 3.0, -1.0]])
    idx = rank_distances(d)
    assert idx.dtype == torch.int64
    assert idx[0].tolist() == [7, 2, 5, 0, 3, 1, 4, 6]
    assert idx[1].tolist() == list(range(8))
    assert idx[2].tolist() == [4, 7, 2, 6, 0, 1, 3, 5]


def test_match_audio_accepts_bank_flags():
    import match_audio
    args, files, overrides = match_audio.parse_args(
        ["a.wav", "b.wav", "torchsynth.rate=16000", "--out", "o", "--init", "bank", "--bank-batches", "2", "--starts", "3"])
    assert args.init == "bank" and args.bank_batches == 2 and args.starts == 3
    assert files == ["a.wav", "b.wav"] and overrides == ["torchsynth.rate=16000"]
    args, _f, _o = match_audio.parse_args(["a.wav", "--out", "o"])
    assert args.init == "center" and args.starts == 1 and args.bank_batches == 32
    args, _f, _o = match_audio.parse_args(["a.wav", "--out", "o", "--init", "random", "--starts", "4"])
    assert args.init == "random" and args.starts == 4


@pytest.mark.parametrize("argv", [["--init", "center", "--starts", "2"], ["--starts", "2"], ["--init", "bank", "--starts",
                                  "0"], ["--init", "bank", "--bank-batches", "0"], ["--init", "nearest"]])
def test_match_audio_refuses_bad_starts(argv):
    import match_audio
    with pytest.raises(SystemExit) as e:
        match_audio.parse_args(["a.wav", "--out", "o"] + argv)
    assert e.value.code == 2


def test_bank_refuses_multi_resolution_loss():
    from inverse_audio_synthesis_amd.retrieval import SpectralBank
    from inverse_audio_synthesis_amd.spectral import MultiResolutionSTFTLoss
    from inverse_audio_synthesis_amd.voice import SynthConfig, Voice
    v = Voice(SynthConfig(batch_size=2, sample_rate=16000, buffer_size_seconds=1.0))
    with pytest.raises(ValueError, match="mel bank"):
        SpectralBank(v, MultiResolutionSTFTLoss(), [0])

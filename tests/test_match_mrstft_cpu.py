"""The per-sound MR-STFT loss without a GPU: host-side refusals of its C-ABI entries (nothing is launched) and the
matcher's loss name."""
import ctypes

import pytest


def _ptrs(n):
    return (ctypes.c_void_p * n)(*([None] * n))


def test_mrstft_rows_refusals(lib):
    assert lib.ias_mrstft_rows_partials_count(4096) == 1 and lib.ias_mrstft_rows_partials_count(4097) == 2
    assert lib.ias_mrstft_rows_partials_count(0) < 0 and lib.ias_mrstft_rows_partials_count(-5) < 0
    x = ctypes.c_void_p(16)                      # never dereferenced: every call below is refused before a launch
    assert lib.ias_mrstft_rows(None, x, 1, 10, x, x, None) < 0
    assert lib.ias_mrstft_rows(x, None, 1, 10, x, x, None) < 0
    assert lib.ias_mrstft_rows(x, x, 1, 10, None, x, None) < 0
    assert lib.ias_mrstft_rows(x, x, 1, 10, x, None, None) < 0
    assert lib.ias_mrstft_rows(x, x, 0, 10, x, x, None) < 0
    assert lib.ias_mrstft_rows(x, x, -1, 10, x, x, None) < 0
    assert lib.ias_mrstft_rows(x, x, 1, 0, x, x, None) < 0


def test_mrstft_rows_total_refusals(lib):
    x = ctypes.c_void_p(16)
    sums = (ctypes.c_void_p * 9)(*([16] * 9))
    counts = (ctypes.c_double * 9)(*([100.0] * 9))
    assert lib.ias_mrstft_rows_total(None, counts, 3, 4, x, None) < 0
    assert lib.ias_mrstft_rows_total(sums, None, 3, 4, x, None) < 0
    assert lib.ias_mrstft_rows_total(sums, counts, 3, 4, None, None) < 0
    assert lib.ias_mrstft_rows_total(sums, counts, 0, 4, x, None) < 0
    assert lib.ias_mrstft_rows_total(sums, counts, 9, 4, x, None) < 0
    assert lib.ias_mrstft_rows_total(sums, counts, 3, 0, x, None) < 0
    assert lib.ias_mrstft_rows_total(_ptrs(3), counts, 3, 4, x, None) < 0          # a null sums pointer
    bad = (ctypes.c_double * 3)(100.0, 0.0, 100.0)
    assert lib.ias_mrstft_rows_total(sums, bad, 3, 4, x, None) < 0                 # count <= 0


def test_mrstft_coef_rows_refusals(lib):
    x = ctypes.c_void_p(16)
    assert lib.ias_mrstft_coef_rows(None, x, 10.0, 3, 4, x, None) < 0
    assert lib.ias_mrstft_coef_rows(x, None, 10.0, 3, 4, x, None) < 0
    assert lib.ias_mrstft_coef_rows(x, x, 10.0, 3, 4, None, None) < 0
    assert lib.ias_mrstft_coef_rows(x, x, 10.0, 0, 4, x, None) < 0
    assert lib.ias_mrstft_coef_rows(x, x, 10.0, 9, 4, x, None) < 0
    assert lib.ias_mrstft_coef_rows(x, x, 10.0, 3, 0, x, None) < 0
    assert lib.ias_mrstft_coef_rows(x, x, 0.0, 3, 4, x, None) < 0


def test_mrstft_backward_rows_refusals(lib):
    x = ctypes.c_void_p(16)
    plan = (ctypes.c_int * 3)()
    # ias_stft_loss_backward_mrstft_rows(audio, window, tables, target, coef_rows, frame_grad, g_audio, B, T, n_fft, hop,
    #                                    n_out, eps, stream)
    ok = [x, x, x, x, x, x, x, 2, 20001, 1024, 120, 513, 1e-8, None]
    for i in (0, 1, 3, 4, 5, 6):
        args = list(ok)
        args[i] = None
        assert lib.ias_stft_loss_backward_mrstft_rows(*args) < 0, i
    for i, v in ((7, 0), (7, -1), (10, 0), (11, 512), (8, 512)):                  # B, hop, n_out != n_fft / 2 + 1, T <= n_fft / 2
        args = list(ok)
        args[i] = v
        assert lib.ias_stft_loss_backward_mrstft_rows(*args) < 0, (i, v)
    args = list(ok)
    args[9] = 4096
    assert lib.ias_stft_loss_backward_mrstft_rows(*args) < 0                      # n_fft
    # ias_stft_grad_frames_mrstft_rows(audio, tables, n_out, target, coef_rows, frame_grad, B, T, n_fft, hop, eps, stream)
    ok = [x, x, 513, x, x, x, 2, 20001, 1024, 120, 1e-8, None]
    for i in (0, 1, 3, 4, 5):
        args = list(ok)
        args[i] = None
        assert lib.ias_stft_grad_frames_mrstft_rows(*args) < 0, i
    for i, v in ((6, 0), (9, 0), (2, 512)):
        args = list(ok)
        args[i] = v
        assert lib.ias_stft_grad_frames_mrstft_rows(*args) < 0, (i, v)
    # ias_stft_grad_spans_mrstft_rows(..., chunk_spans, B, T, n_fft, hop, eps, plan_host, stream)
    ok = [x, x, 513, x, x, x, 2, 20001, 1024, 120, 1e-8, plan, None]
    for i in (0, 1, 3, 4, 5, 11):
        args = list(ok)
        args[i] = None
        assert lib.ias_stft_grad_spans_mrstft_rows(*args) < 0, i
    args = list(ok)
    args[5] = ctypes.c_void_p(20)                                                  # spans not 16-byte aligned
    assert lib.ias_stft_grad_spans_mrstft_rows(*args) < 0
    for i, v in ((6, 0), (9, -2), (2, 300)):
        args = list(ok)
        args[i] = v
        assert lib.ias_stft_grad_spans_mrstft_rows(*args) < 0, (i, v)


def test_matcher_accepts_multi_resolution_stft_and_lists_three_losses():
    from inverse_audio_synthesis_amd.match import SoundMatcher
    from inverse_audio_synthesis_amd.spectral import MultiResolutionSTFTLoss
    from inverse_audio_synthesis_amd.voice import SynthConfig, Voice
    v = Voice(SynthConfig(batch_size=2, sample_rate=16000, buffer_size_seconds=1.0))
    m = SoundMatcher(v, loss="multi_resolution_stft")
    assert isinstance(m.loss, MultiResolutionSTFTLoss) and m.loss_kind == "multi_resolution_stft"
    assert [(p.n_fft, p.hop_length, p.win_length) for p in m.loss.plans] == [(1024, 120, 600), (2048, 240, 1200),
                                                                               (512, 50, 240)]
    m = SoundMatcher(v, loss="multi_resolution_stft",
                     mrstft_kwargs=dict(fft_sizes=(512, 1024), hop_sizes=(125, 256), win_lengths=(512, 1024)))
    assert [(p.n_fft, p.hop_length) for p in m.loss.plans] == [(512, 125), (1024, 256)]
    for bad in ("mrstft", "mse"):
        with pytest.raises(ValueError) as e:
            SoundMatcher(v, loss=bad)
        msg = str(e.value)
        assert "unknown matching loss" in msg
        assert all(n in msg for n in ("'mel_l1'", "'stft_l1'", "'multi_resolution_stft'")), msg


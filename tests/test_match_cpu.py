"""Sound matching without a GPU: the WAV handling of match_audio.py, the parameter record it writes, the matcher's
argument checks and the host-side argument checks of the new C-ABI entries."""
import wave

import numpy as np
import pytest
import torch

import match_audio as ma


def _write(path, frames, sr, width):
    dtype = {2: "<i2", 4: "<i4"}[width]
    with wave.open(str(path), "wb") as w:
        w.setnchannels(frames.shape[1])
        w.setsampwidth(width)
        w.setframerate(sr)
        w.writeframes(np.ascontiguousarray(frames.astype(dtype)).tobytes())


@pytest.mark.parametrize("width,scale", [(2, 32768.0), (4, 2147483648.0)])
def test_read_wav_pcm_widths_and_stereo_average(tmp_path, width, scale):
    rng = np.random.default_rng(width)
    ints = rng.integers(-int(scale) // 2, int(scale) // 2, size=(1000, 2))
    _write(tmp_path / "s.wav", ints, 16000, width)
    x = ma.read_wav(str(tmp_path / "s.wav"), 16000)
    assert x.dtype == np.float32 and x.shape == (1000,)
    np.testing.assert_allclose(x, (ints[:, 0] / scale + ints[:, 1] / scale) / 2, rtol=0, atol=1e-7)
    mono = rng.integers(-int(scale) // 2, int(scale) // 2, size=(500, 1))
    _write(tmp_path / "m.wav", mono, 16000, width)
    np.testing.assert_allclose(ma.read_wav(str(tmp_path / "m.wav"), 16000), mono[:, 0] / scale, rtol=0, atol=1e-7)


def test_write_then_read_round_trip(tmp_path):
    x = np.sin(np.arange(4000) * 0.05).astype(np.float32) * 0.8
    x[10] = 1.5                          # clipped
    ma.write_wav(str(tmp_path / "o.wav"), x, 22050)
    with wave.open(str(tmp_path / "o.wav"), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 22050, 4000)
    y = ma.read_wav(str(tmp_path / "o.wav"), 22050)
    keep = np.arange(4000) != 10
    assert np.abs(y - x)[keep].max() <= 0.5 / 32768 + 1e-7
    assert y[10] == pytest.approx(32767 / 32768)


def test_wrong_rate_and_width_are_refused(tmp_path):
    _write(tmp_path / "r.wav", np.zeros((100, 1), dtype=np.int64), 48000, 2)
    with pytest.raises(ValueError, match="48000 Hz.*44100 Hz"):
        ma.read_wav(str(tmp_path / "r.wav"), 44100)
    with wave.open(str(tmp_path / "b8.wav"), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(1)
        w.setframerate(44100)
        w.writeframes(bytes(100))
    with pytest.raises(ValueError, match="8-bit"):
        ma.read_wav(str(tmp_path / "b8.wav"), 44100)


def test_pad_and_crop_warn():
    x = np.arange(10, dtype=np.float32)
    with pytest.warns(UserWarning, match="zero-padded"):
        y = ma.fit_length(x, 16, "x")
    assert y.shape == (16,) and (y[:10] == x).all() and (y[10:] == 0).all()
    with pytest.warns(UserWarning, match="cropped"):
        y = ma.fit_length(x, 4, "x")
    assert (y == x[:4]).all()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert ma.fit_length(x, 10) is x


def test_params_record_has_every_parameter_in_its_units():
    from inverse_audio_synthesis_amd import voice_spec as S
    from inverse_audio_synthesis_amd.voice_grad import _from_0to1
    p = torch.rand(78, generator=torch.Generator().manual_seed(0))
    rec = ma.params_record(p)
    assert len(rec) == 78
    assert [(r["module"], r["name"]) for r in rec] == [(m, n) for (m, n, *_r) in S.PARAMS]
    units = _from_0to1(p.double().reshape(1, -1))[0]
    for i, r in enumerate(rec):
        assert r["value01"] == float(p[i]) and r["value"] == pytest.approx(float(units[i]))


def test_matcher_refuses_unknown_loss_and_keys():
    from inverse_audio_synthesis_amd.match import SoundMatcher
    from inverse_audio_synthesis_amd.voice import SynthConfig, Voice
    v = Voice(SynthConfig(batch_size=2, sample_rate=16000, buffer_size_seconds=1.0))
    with pytest.raises(ValueError, match="unknown matching loss"):
        SoundMatcher(v, loss="mse")


def test_capi_argument_checks(lib):
    """Host-side refusals of the new entries (nothing is launched)."""
    assert lib.ias_l1_rows_partials_count(345 * 128) == 11
    assert lib.ias_l1_rows_partials_count(4096) == 1 and lib.ias_l1_rows_partials_count(4097) == 2
    assert lib.ias_l1_rows_partials_count(0) < 0
    assert lib.ias_l1_rows(None, None, 1, 10, None, None, None) < 0
    assert lib.ias_stft_loss_backward_rows(*([None] * 7), 0, *([None] * 4), 1, 1000, 512, 128, 257, 2, 1.0, None) < 0
    assert lib.ias_match_adam_step(*([None] * 11), 1, 78, 0.01, 0.9, 0.999, 1e-8, None) < 0


def test_fit_length_is_silent_without_a_name():
    import warnings
    x = np.arange(10, dtype=np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        y = ma.fit_length(x, 16, None)
        assert y.shape == (16,) and (y[:10] == x).all() and (y[10:] == 0).all()
        assert (ma.fit_length(x, 4, name=None) == x[:4]).all()
    with pytest.warns(UserWarning, match=r"^x: 10 samples, zero-padded to the synth buffer of 16$"):
        ma.fit_length(x, 16, "x")
    with pytest.warns(UserWarning, match=r"^input: 10 samples, cropped to the synth buffer of 4$"):
        ma.fit_length(x, 4)


@pytest.mark.parametrize("forward", [True, False])
def test_resample_rows_groups_by_rate(lib, monkeypatch, forward):
    """Rows at 48000, 16000, 48000 Hz to or from 16000 Hz: one ``resample`` call per rate in ascending order, the group
    zero-padded to its longest row in the rows' order, every output at its row's position and of its ``output_length``."""
    from inverse_audio_synthesis_amd import resample as R
    rates, lengths = [48000, 16000, 48000], [5, 3, 7]
    rows = [np.arange(1, n + 1, dtype=np.float32) * (i + 1) for i, n in enumerate(lengths)]
    rows[2] = torch.from_numpy(rows[2])
    calls = []

    def fake(x, a, b):                                # repeats or drops samples: [rows, L] -> [rows, ceil(L b / a)]
        return x.repeat_interleave(b // a, dim=1) if b > a else x[:, ::a // b]

    def stub(x, a, b):
        calls.append((x.clone(), a, b))
        return fake(x, a, b)
    monkeypatch.setattr(R, "resample", stub)
    fr, to = (rates, [16000] * 3) if forward else ([16000] * 3, rates)
    out = ma.resample_rows(rows, fr, to, torch.device("cpu"))
    assert [(a, b) for _x, a, b in calls] == ([(16000, 16000), (48000, 16000)] if forward else
                                              [(16000, 16000), (16000, 48000)])
    assert torch.equal(calls[0][0], torch.tensor([[2.0, 4.0, 6.0]]))
    assert torch.equal(calls[1][0], torch.tensor([[1.0, 2, 3, 4, 5, 0, 0], [3.0, 6, 9, 12, 15, 18, 21]]))
    want = [2, 3, 3] if forward else [15, 3, 21]                      # ceil(n / 3) and 3 n
    for i, y in enumerate(out):
        assert torch.equal(y, fake(torch.as_tensor(rows[i])[None], fr[i], to[i])[0]) and y.shape == (want[i],)


@pytest.mark.parametrize("loss", ["mel_l1", "stft_l1", "multi_resolution_stft"])
def test_search_stage_loss_rule(monkeypatch, loss):
    """A BANK_BATCH Voice at the synth's settings; the matcher's own loss, or for multi_resolution_stft a MelSpectrogramL1
    of ``cfg.mel`` with ``sample_rate`` defaulted to the synth's rate."""
    from types import SimpleNamespace as NS
    from inverse_audio_synthesis_amd import spectral, voice

    class Stub:
        def __init__(self, *a, **kw):
            self.a, self.kw, self.dev = a, kw, None

        def to(self, dev):
            self.dev = dev
            return self
    Mel = type("Mel", (Stub,), {})
    monkeypatch.setattr(voice, "SynthConfig", Stub)
    monkeypatch.setattr(voice, "Voice", Stub)
    monkeypatch.setattr(spectral, "MelSpectrogramL1", Mel)
    cfg = NS(torchsynth=NS(buffer_size_seconds=1.5, reproducible=False), mel={"n_fft": 512, "n_mels": 40})
    matcher = NS(loss=object())
    v, got = ma.search_stage(cfg, matcher, NS(loss=loss), 22050, "dev")
    assert v.dev == "dev" and v.a[0].kw == dict(batch_size=ma.BANK_BATCH, sample_rate=22050, buffer_size_seconds=1.5,
                                                reproducible=False)
    if loss == "multi_resolution_stft":
        assert type(got) is Mel and got.kw == {"n_fft": 512, "n_mels": 40, "sample_rate": 22050} and got.dev == "dev"
        cfg.mel["sample_rate"] = 16000
        assert ma.search_stage(cfg, matcher, NS(loss=loss), 22050, "dev")[1].kw["sample_rate"] == 16000
        assert cfg.mel == {"n_fft": 512, "n_mels": 40, "sample_rate": 16000}
    else:
        assert got is matcher.loss

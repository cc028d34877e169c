"""Band-limited resampler on the GPU (ias_resample, resample.resample / resample.Resample, match_audio.py --resample):
values against the fp64 restatement of torchaudio's formula (tests/test_resample_cpu.py), the per-row contract, signal
checks and the entry point."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

from test_resample_cpu import RATIOS, ref_plan, ref_resample

pytestmark = pytest.mark.gpu


def _x(B, T, seed):
    return torch.rand((B, T), generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 - 1


@pytest.mark.parametrize("method", ["sinc_interp_hann", "sinc_interp_kaiser"])
@pytest.mark.parametrize("ratio", list(RATIOS), ids=[f"{a}-{b}" for a, b in RATIOS])
def test_matches_fp64_restatement(lib, dev, ratio, method):
    from inverse_audio_synthesis_amd.resample import resample
    orig, new = ratio
    o, n, width, K = ref_plan(orig, new)
    kind = "hann" if method == "sinc_interp_hann" else "kaiser"
    # T = 1, T = K - 1, 4 s, and T that are not multiples of o (B = 128 among them)
    for B, T in ((1, 1), (3, K - 1), (1, 4 * orig), (128, 3 * o + 17), (3, 2 * o + 1)):
        x = _x(B, T, seed=B * 1000 + T).float()
        y = resample(x.to(dev), orig, new, resampling_method=method)
        ref = ref_resample(x.double().numpy(), orig, new, method=kind)
        assert tuple(y.shape) == ref.shape == (B, -(-n * T // o)), (B, T)
        err = np.abs(y.cpu().double().numpy() - ref).max()
        assert err <= 1e-5, (B, T, err)


@pytest.mark.parametrize("ratio", [(48000, 44100), (44100, 48000), (22050, 44100), (192000, 44100)],
                         ids=["48k-44k1", "44k1-48k", "22k05-44k1", "192k-44k1"])
def test_same_bits_for_the_same_row(lib, dev, ratio):
    from inverse_audio_synthesis_amd.resample import resample
    orig, new = ratio
    T = orig // 2 + 3
    x = _x(128, T, seed=7).float()
    row = x[5].clone()
    x[0], x[77] = row, row
    y = resample(x.to(dev), orig, new).cpu()
    assert torch.equal(y[0], y[77])
    alone = resample(row.reshape(1, T).to(dev), orig, new).cpu()[0]
    assert torch.equal(alone, y[0])
    assert torch.equal(resample(row.to(dev), orig, new).cpu(), alone)            # 1-D input
    for k in (1, 2, 3):                                                           # start moved by 1-3 floats
        buf = torch.zeros(T + 4, device=dev)
        buf[k:k + T] = row.to(dev)
        view = buf[k:k + T]
        assert view.data_ptr() % 16 == 4 * k
        assert torch.equal(resample(view, orig, new).cpu(), alone), k


def test_identity_module_and_cpu(lib, dev):
    from inverse_audio_synthesis_amd.resample import Resample, resample
    x = _x(3, 1000, seed=1).float().to(dev)
    assert torch.equal(resample(x, 44100, 44100), x)
    assert torch.equal(Resample(16000, 16000)(x), x)
    for method in ("sinc_interp_hann", "sinc_interpolation", "sinc_interp_kaiser", "kaiser_window"):
        m = Resample(48000, 44100, resampling_method=method)
        assert torch.equal(m(x), resample(x, 48000, 44100, resampling_method=method)), method
    hann, kaiser = resample(x, 48000, 44100), resample(x, 48000, 44100, resampling_method="kaiser_window")
    assert torch.equal(hann, resample(x, 48000, 44100, resampling_method="sinc_interpolation"))
    assert not torch.equal(hann, kaiser)
    # [..., T] keeps the leading dimensions
    assert tuple(resample(x.reshape(3, 1, 1000), 48000, 44100).shape) == (3, 1, 919)
    with pytest.raises(RuntimeError, match="ROCm device"):
        resample(x.cpu(), 48000, 44100)


def _sine(f, sr, T):
    return np.sin(2 * np.pi * f * np.arange(T) / sr)


def test_sines_round_trip_and_alias(lib, dev):
    from inverse_audio_synthesis_amd.resample import resample
    for f in (1000, 5000):
        y = resample(torch.tensor(_sine(f, 48000, 48000), dtype=torch.float32, device=dev), 48000, 44100).cpu().numpy()
        assert len(y) == 44100
        err = np.abs(y - _sine(f, 44100, 44100))[200:-200].max()
        assert err <= 1e-3, (f, err)
    x = torch.tensor(_sine(1000, 44100, 44100), dtype=torch.float32, device=dev)
    back = resample(resample(x, 44100, 48000), 48000, 44100).cpu().numpy()
    assert len(back) == 44100
    err = np.abs(back - x.cpu().numpy())[200:-200].max()
    assert err <= 1.5e-3, err
    alias = resample(torch.tensor(_sine(30000, 96000, 96000), dtype=torch.float32, device=dev), 96000, 44100)
    assert np.abs(alias.cpu().numpy())[200:-200].max() <= 1e-2


def _write_pcm(path, x, sr, width):
    v = np.round(np.clip(x, -1, 1) * (2 ** (8 * width - 1) - 1)).astype(np.int64)
    if width == 2:
        raw = v.astype("<i2").tobytes()
    else:
        u = (v & 0xFFFFFF).astype(np.uint32)
        raw = np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=-1).astype(np.uint8).tobytes()
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(width)
        w.setframerate(sr)
        w.writeframes(raw)


def test_match_audio_resample_entry_point(lib, dev, tmp_path):
    from conftest import ROOT
    t = np.arange(45000) / 48000                                                 # 24-bit, 48 kHz, short: padded
    _write_pcm(tmp_path / "a48.wav", 0.5 * np.sin(2 * np.pi * 440 * t) * np.exp(-3 * t), 48000, 3)
    t = np.arange(16000) / 16000
    _write_pcm(tmp_path / "b16.wav", 0.3 * np.sin(2 * np.pi * 220 * t) * np.exp(-2 * t), 16000, 2)
    out = tmp_path / "out"
    base = [sys.executable, os.path.join(ROOT, "match_audio.py"), str(tmp_path / "a48.wav"), str(tmp_path / "b16.wav"),
            "torchsynth.rate=16000", "torchsynth.buffer_size_seconds=1.0", "--steps", "3", "--out", str(out)]
    r = subprocess.run(base + ["--resample"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "resampled 48000 -> 16000 Hz" in r.stdout and "zero-padded" in r.stdout      # 45000 -> 15000 samples
    for name, sr, frames in (("a48", 48000, 48000), ("b16", 16000, 16000)):
        rec = json.load(open(out / f"{name}.params.json"))
        assert rec["input_rate"] == sr and rec["synth_rate"] == 16000
        assert len(rec["params"]) == 78 and rec["final_loss"] <= rec["initial_loss"]
        with wave.open(str(out / f"{name}.match.wav"), "rb") as w:
            assert w.getframerate() == sr and w.getnframes() == frames and w.getsampwidth() == 2
    r = subprocess.run(base, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, cwd=ROOT)
    assert r.returncode != 0
    assert "sample rate 48000 Hz, the synth runs at 16000 Hz" in r.stdout

"""ias_pitch_yin on the GPU against the fp64 model of its contract (tests/pitch_model.py), its per-frame bit guarantees,
``estimate_pitch`` end to end on tones and on Voice renders, and ``match_audio.py --pitch``."""
import functools
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import pitch_model as pm

pytestmark = pytest.mark.gpu

RATE = 16000
# (B, T, W, tau_min, tau_max, hop): odd T (rows at every 16-byte phase), W and tau_max multiples of neither 64 nor the
# kernel's seven lags per lane, an odd hop; the CPU tests' shape; exactly one frame ending at T with hop 1
CASES = [(3, 4099, 200, 5, 333, 97), (2, 8000, 512, 8, 512, 256), (1, 845, 512, 2, 333, 1)]
THR = 0.15


def _mix(a, b, gain):
    return (a + gain * b).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _inputs(case):
    B, T = CASES[case][:2]
    if case == 0:
        rows = [_mix(pm.tone("saw", 50.8, RATE, T), pm.tone("noise", 0, RATE, T, seed=11), 0.2),
                np.zeros(T, dtype=np.float32),                            # silence: c == 0, d' == 1 everywhere
                _mix(pm.tone("sine", 61.9, RATE, T), pm.tone("noise", 0, RATE, T, seed=12), 0.01)]
    elif case == 1:
        rows = [pm.tone("square", 43.4, RATE, T), pm.tone("saw_noise", 65.6, RATE, T, seed=13)]
    else:
        rows = [_mix(pm.tone("noise", 0, RATE, T, seed=14), pm.tone("sine", 47.1, RATE, T), 1.0)]
    x = np.stack(rows)
    assert x.shape == (B, T)
    return x


@functools.lru_cache(maxsize=None)
def _model(case):
    """-> per row (d' fp64 [F, tau_max + 1], c, energy fp64 [F]) of the model; computed once, never changed."""
    _B, _T, W, _tmin, tau_max, hop = CASES[case]
    return [pm.dprime(r, W, tau_max, hop) for r in _inputs(case)]


@functools.lru_cache(maxsize=None)
def _kernel(case):
    """-> (period, aperiodicity, energy [B, F], dprime [B, F, tau_max + 1]) of one launch, as numpy."""
    from inverse_audio_synthesis_amd.pitch import pitch_yin
    _B, _T, W, tmin, tau_max, hop = CASES[case]
    out = pitch_yin(torch.from_numpy(_inputs(case)).cuda(), W, tmin, tau_max, hop, threshold=THR, return_dprime=True)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_dprime_and_energy_match_the_model(lib, dev, case):
    """Relative error of d' at most 2 (W + 4) 2^-24 and of the energy at most (W + 1) 2^-24: the bounds of a W-term fp32
    chain of non-negative terms, once for d and once for its prefix sum (derived, not measured); d' is exactly 1 at lag 0
    and wherever the model's running sum is 0."""
    B, T, W, _tmin, tau_max, hop = CASES[case]
    F = pm.num_frames(T, W, tau_max, hop)
    _p, _a, energy, dprime = _kernel(case)
    assert dprime.shape == (B, F, tau_max + 1) and energy.shape == (B, F)
    u = 2.0 ** -24
    for b, (dp, c, e) in enumerate(_model(case)):
        got = dprime[b].astype(np.float64)
        zero = c == 0.0
        zero[:, 0] = True
        assert (dprime[b][zero] == np.float32(1.0)).all()
        diff = np.abs(got - dp)[~zero]
        assert (diff <= 2 * (W + 4) * u * dp[~zero]).all()                 # no division: an exact repeat has d' == 0
        err = diff[dp[~zero] > 0] / dp[~zero][dp[~zero] > 0]
        eerr = np.abs(energy[b].astype(np.float64) - e) / np.where(e > 0, e, 1.0)
        print(f"case {case} row {b}: d' rel err {err.max() if err.size else 0.0:.3e} (bound {2 * (W + 4) * u:.3e}), "
              f"energy rel err {eerr.max():.3e} (bound {(W + 1) * u:.3e})")
        assert eerr.max() <= (W + 1) * u
        assert (energy[b][e == 0.0] == 0.0).all()
    if case == 0:
        assert (dprime[1] == np.float32(1.0)).all()                       # the silent row


@pytest.mark.parametrize("case", range(len(CASES)))
def test_pick_and_refinement_on_the_kernels_own_dprime(lib, dev, case):
    """The model's pick run on the kernel's d' output leaves no near-tie ambiguity, so every frame is checked: the same
    integer lag, aperiodicity the same bits as d'[lag], period within 1e-6 relative."""
    B, _T, _W, tmin, tau_max, _hop = CASES[case]
    period, aper, _e, dprime = _kernel(case)
    for b in range(B):
        taus, want_period, want_aper = pm.pick(dprime[b], tmin, tau_max, THR)
        assert np.array_equal(_bits(aper[b]), _bits(want_aper))
        assert (np.abs(period[b] - want_period) <= 1e-6 * want_period).all()
        for f in range(dprime.shape[1]):
            # the kernel's lag: the lags whose d' has the reported bits and whose refined period is the reported one
            same = np.nonzero(_bits(dprime[b, f, tmin:]) == _bits(aper[b, f:f + 1])[0])[0] + tmin
            lags = [int(t) for t in same
                    if abs(pm.refine(dprime[b, f], int(t), tmin, tau_max) - float(period[b, f])) <= 1e-6 * period[b, f]]
            assert lags == [int(taus[f])], (b, f, lags, int(taus[f]))
    if case == 0:                                                         # silence: the first lag searched, unrefined
        assert (period[1] == np.float32(tmin)).all() and (aper[1] == np.float32(1.0)).all()


@pytest.mark.parametrize("case", range(len(CASES)))
def test_a_rows_bits_do_not_depend_on_the_batch(lib, dev, case):
    """Rows permuted, the batch padded with other rows, a row alone at an offset of 1 to 3 floats, and dprime = NULL: the
    same bits per frame."""
    from inverse_audio_synthesis_amd.pitch import pitch_yin
    B, T, W, tmin, tau_max, hop = CASES[case]
    x = torch.from_numpy(_inputs(case)).to(dev)
    ref = _kernel(case)
    plain = pitch_yin(x, W, tmin, tau_max, hop, threshold=THR)
    assert len(plain) == 3
    for got, want in zip(plain, ref[:3]):
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    extra = torch.from_numpy(np.stack([pm.tone("noise", 0, RATE, T, seed=21), pm.tone("saw", 40.0, RATE, T)])).to(dev)
    perm = list(range(B))[::-1]
    mixed = torch.cat([extra[:1], x[perm], extra[1:]]).contiguous()
    got = pitch_yin(mixed, W, tmin, tau_max, hop, threshold=THR, return_dprime=True)
    for g, want in zip(got, ref):
        assert np.array_equal(_bits(g[1:1 + B].cpu().numpy()), _bits(want[perm]))
    for off in (1, 2, 3):
        b = off % B
        flat = torch.zeros(T + 8, dtype=torch.float32, device=dev)
        flat[off:off + T] = x[b]
        alone = flat[off:off + T].view(1, T)
        assert alone.is_contiguous() and alone.data_ptr() % 16 == 4 * off
        got = pitch_yin(alone, W, tmin, tau_max, hop, threshold=THR, return_dprime=True)
        for g, want in zip(got, ref):
            assert np.array_equal(_bits(g[0].cpu().numpy()), _bits(want[b]))


@functools.lru_cache(maxsize=None)
def _tones():
    T = 8000
    rows = [pm.tone(kind, midi, RATE, T, seed=i) for kind in pm.TONE_KINDS for i, midi in enumerate(pm.TONE_MIDIS)]
    truth = [midi for _kind in pm.TONE_KINDS for midi in pm.TONE_MIDIS]
    rows += [pm.tone("noise", 0, RATE, T, seed=31), np.zeros(T, dtype=np.float32)]
    return np.stack(rows), np.array(truth)


def test_estimate_pitch_on_tones_noise_and_silence(lib, dev):
    """The 16 kHz tones of the CPU test (sine, naive saw and square, saw + noise; MIDI 36 to 72) through ``estimate_pitch``
    with its defaults (lags of MIDI 21..108, hop 512): within 0.1 semitone; white noise and silence are unvoiced."""
    from inverse_audio_synthesis_amd.pitch import estimate_pitch
    x, truth = _tones()
    est = estimate_pitch(torch.from_numpy(x).to(dev), RATE)
    n = len(truth)
    assert est.frame_midi.shape == (n + 2, 14) and est.midi.dtype == torch.float32 and est.voiced.dtype == torch.bool
    assert est.voiced[:n].all() and not est.voiced[n:].any()
    err = (est.midi[:n].cpu().double().numpy() - truth)
    print(f"estimate_pitch on {n} tones: worst error {np.abs(err).max():.4f} semitone, lowest confidence "
          f"{float(est.confidence[:n].min()):.4f}")
    assert np.abs(err).max() <= 0.1
    assert torch.isnan(est.midi[n:]).all() and (est.confidence[n:] == 0).all() and (est.confidence[:n] > 0.85).all()
    assert not est.frame_voiced[n:].any()


VOICE_MIDI = (40.0, 49.5, 61.0, 70.0)
VOICE_TOL = 0.0285 + 0.02


def test_estimate_pitch_recovers_retuned_voices(lib, dev):
    """Centre parameters retuned to MIDI 40, 49.5, 61 and 70, rendered by the Voice at 16 kHz, 1 s, B = 4: ``estimate_pitch``
    gives the notes back.  Tolerance: the same four voices rendered by the CPU oracle (synth_oracle, "cr") and run through
    tests/pitch_model.py are off by 0.0059, 0.0066, 0.0130 and 0.0285 semitone (the centre voice mixes a sine with a
    square-saw under a 0.5 s attack, and its vco_2 is the naive wave whose bias the tones test describes); the worst of
    them, 0.0285, plus 0.02 semitone for the fp32 d' against the fp64 one gives 0.0485."""
    from inverse_audio_synthesis_amd.pitch import PitchEstimate, estimate_pitch, retune
    from inverse_audio_synthesis_amd.voice import SynthConfig, Voice
    midi = torch.tensor(VOICE_MIDI)
    yes = torch.ones(4, dtype=torch.bool)
    params = retune(torch.full((4, 78), 0.5), PitchEstimate(midi, yes, yes.float(), midi[:, None], yes[:, None]))
    voice = Voice(SynthConfig(batch_size=4, sample_rate=RATE, buffer_size_seconds=1.0, reproducible=False)).to(dev)
    audio = voice.render(params.to(dev))
    est = estimate_pitch(audio, RATE)
    err = (est.midi.cpu() - midi).abs()
    print(f"voices at {VOICE_MIDI}: estimated {est.midi.cpu().tolist()}, confidence {est.confidence.cpu().tolist()}")
    assert est.voiced.all() and err.max().item() <= VOICE_TOL, err.tolist()


def _write_pcm16(path, x, rate):
    pcm = np.clip(np.round(np.asarray(x, dtype=np.float64) * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.tobytes())


def test_match_audio_pitch_entry_point(lib, dev, tmp_path):
    from conftest import ROOT
    t = np.arange(RATE) / RATE
    _write_pcm16(tmp_path / "note.wav", 0.5 * np.sin(2 * np.pi * 220.0 * t) * np.exp(-2 * t), RATE)
    _write_pcm16(tmp_path / "hiss.wav", 0.2 * np.random.default_rng(3).standard_normal(RATE).clip(-3, 3), RATE)
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "match_audio.py"), str(tmp_path / "note.wav"), str(tmp_path / "hiss.wav"),
           "torchsynth.rate=16000", "torchsynth.buffer_size_seconds=1.0", "--steps", "2", "--out", str(out), "--pitch"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:]
    note = json.load(open(out / "note.params.json"))
    hiss = json.load(open(out / "hiss.params.json"))
    assert note["voiced"] is True and abs(note["estimated_midi"] - 57.0) <= 0.1 and note["pitch_confidence"] > 0.9
    assert hiss["voiced"] is False and hiss["estimated_midi"] is None and hiss["pitch_confidence"] == 0.0
    f0 = {(p["module"], p["name"]): p for p in note["params"]}[("keyboard", "midi_f0")]
    assert abs(f0["value"] - 57.0) < 3.0                                   # two Adam steps from the estimated note
    assert len(hiss["params"]) == 78 and os.path.exists(out / "note.match.wav")

"""Pitch estimator without a GPU: the fp64 model of the ias_pitch_yin contract on tones and noise, the aggregation and
``retune`` on CPU tensors, match_audio.py's --pitch flags, and the host-side half of the C ABI (frame count, refusals)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import pitch_model as pm

RATE, T, W, TAU_MIN, TAU_MAX, HOP, THR = 16000, 8000, 512, 8, 512, 256, 0.15


# ------------------------------------------------------------------------------------------------ the model on signals
@pytest.mark.parametrize("kind", pm.TONE_KINDS)
def test_model_finds_the_note_of_a_tone(kind):
    """MIDI 36 to 72 in steps of 3.7 at 16 kHz: the median frame pitch within 0.1 semitone of the truth and every frame
    periodic (aperiodicity < 0.15).  (Worst error of the model on this range: 0.041 semitone; above MIDI 76 the short
    periods bias the naive waves by up to 0.19, which is why the range ends at 72.)"""
    for i, midi in enumerate(pm.TONE_MIDIS):
        x = pm.tone(kind, midi, RATE, T, seed=i)
        period, aper, _e, _tau = pm.yin(x, W, TAU_MIN, TAU_MAX, HOP, THR)
        assert len(period) == 28
        fm = np.sort(pm.frame_midi(period, RATE))
        err = abs(fm[(len(fm) - 1) // 2] - midi)
        print(f"{kind} midi {midi:.1f}: error {err:.4f} semitone, max aperiodicity {aper.max():.4f}")
        assert err <= 0.1, (kind, midi, err)
        assert aper.max() < 0.15, (kind, midi, aper.max())


def test_model_calls_noise_unvoiced():
    x = pm.tone("noise", 0.0, RATE, T, seed=5)
    _p, aper, _e, _tau = pm.yin(x, W, TAU_MIN, TAU_MAX, HOP, THR)
    print(f"white noise: minimum aperiodicity {aper.min():.3f}")
    assert aper.min() > 0.5
    est = pm.estimate(np.stack([x, pm.tone("sine", 57.0, RATE, T)]), RATE, W, TAU_MIN, TAU_MAX, HOP, THR)
    assert est.voiced.tolist() == [False, True]
    assert math.isnan(float(est.midi[0])) and float(est.confidence[0]) == 0.0
    assert abs(float(est.midi[1]) - 57.0) <= 0.1 and float(est.confidence[1]) > 0.99


def test_model_pick_follows_the_contract():
    """Hand-made d' rows: threshold crossing then descent, the global minimum without a crossing (first of equals), the
    refinement's conditions."""
    row = np.ones(12, dtype=np.float32)
    row[[4, 5, 6, 7]] = [0.14, 0.10, 0.05, 0.08]
    row[9] = 0.01                                                       # lower, but behind the first dip
    tau, period, aper = pm.pick(row[None], 2, 11, 0.15)
    assert tau[0] == 6 and aper[0] == np.float32(0.05)
    y0, y1, y2 = float(row[5]), float(row[6]), float(row[7])
    assert period[0] == 6 + (y0 - y2) / (2 * (y0 - 2 * y1 + y2))
    tau, period, _a = pm.pick(row[None], 6, 11, 0.15)                  # the pick at tau_min: no refinement
    assert tau[0] == 6 and period[0] == 6.0
    row2 = np.full(12, 0.6, dtype=np.float32)
    row2[[3, 8]] = 0.4                                                  # no crossing: first global minimum
    tau, period, aper = pm.pick(row2[None], 2, 11, 0.15)
    assert tau[0] == 3 and aper[0] == np.float32(0.4) and period[0] == 3.0 + 0.0
    flat = np.ones((1, 12), dtype=np.float32)                           # silence: d' = 1 everywhere
    tau, period, aper = pm.pick(flat, 4, 11, 0.15)
    assert tau[0] == 4 and period[0] == 4.0 and aper[0] == 1.0
    row3 = np.ones(12, dtype=np.float32)
    row3[[9, 10, 11]] = [0.1, 0.05, 0.01]                               # descent runs into tau_max: no refinement
    tau, period, _a = pm.pick(row3[None], 2, 11, 0.15)
    assert tau[0] == 11 and period[0] == 11.0


def test_model_dprime_edges():
    x = np.zeros(40, dtype=np.float32)
    dp, c, e = pm.dprime(x, 8, 6, 5)
    assert dp.shape == (6, 7) and (dp == 1.0).all() and (c == 0.0).all() and (e == 0.0).all()
    x = np.arange(20, dtype=np.float32)                                  # a ramp: d(tau) = W tau^2
    dp, c, e = pm.dprime(x, 4, 3, 1)
    assert np.allclose(c[0], [0, 4, 20, 56]) and np.allclose(dp[0], [1, 1, 16 * 2 / 20, 36 * 3 / 56])
    assert e[0] == 0 + 1 + 4 + 9 and e[1] == 1 + 4 + 9 + 16


# ------------------------------------------------------------------------------------------------ aggregation
def _agg(period, aper, energy, **kw):
    from inverse_audio_synthesis_amd.pitch import aggregate_pitch
    f = lambda a: torch.tensor(a, dtype=torch.float32)                  # noqa: E731
    return aggregate_pitch(f(period), f(aper), f(energy), 16000, **kw)


def _midi(period):
    return 69.0 + 12.0 * math.log2(16000 / period / 440.0)


def test_aggregate_gates_by_energy_and_takes_the_lower_median():
    # row 0: four voiced frames (an even count: the lower median is the 2nd smallest note = the 2nd largest period), one
    # quiet frame (40 dB down) and one aperiodic frame, both with wild periods that must not count
    period = [[100.0, 50.0, 102.0, 98.0, 101.0, 20.0], [80.0] * 6]
    aper = [[0.01, 0.02, 0.03, 0.04, 0.05, 0.5], [0.05, 0.06, 0.2, 0.3, 0.4, 0.5]]
    energy = [[1.0, 1e-4, 1.0, 0.5, 2.0, 2.0], [1.0] * 6]
    est = _agg(period, aper, energy, min_voiced=3)
    assert est.frame_voiced.tolist() == [[True, False, True, True, True, False], [True, True, False, False, False, False]]
    assert est.voiced.tolist() == [True, False]
    assert float(est.midi[0]) == pytest.approx(_midi(101.0), abs=1e-4)
    assert float(est.confidence[0]) == pytest.approx(1.0 - 0.03, abs=1e-6)     # lower median of .01 .03 .04 .05
    assert math.isnan(float(est.midi[1])) and float(est.confidence[1]) == 0.0
    assert est.frame_midi.shape == (2, 6) and float(est.frame_midi[1, 0]) == pytest.approx(_midi(80.0), abs=1e-4)
    assert est.midi.dtype == torch.float32 and est.voiced.dtype == torch.bool
    # min_voiced: two voiced frames are enough when asked so; the rows do not affect one another
    est2 = _agg(period, aper, energy, min_voiced=2)
    assert est2.voiced.tolist() == [True, True] and float(est2.midi[1]) == pytest.approx(_midi(80.0), abs=1e-4)
    assert torch.equal(est2.midi[0], est.midi[0]) and torch.equal(est2.confidence[0], est.confidence[0])
    alone = _agg(period[:1], aper[:1], energy[:1], min_voiced=3)
    assert torch.equal(alone.midi[0], est.midi[0]) and torch.equal(alone.frame_voiced[0], est.frame_voiced[0])
    # the gate is relative to the row's loudest frame: at -50 dB the quiet frame counts (odd count: the middle one)
    est3 = _agg(period, aper, energy, gate_db=-50.0)
    assert est3.frame_voiced[0].tolist() == [True, True, True, True, True, False]
    assert float(est3.midi[0]) == pytest.approx(_midi(100.0), abs=1e-4)


def test_aggregate_silence_is_unvoiced():
    est = _agg([[8.0] * 4, [100.0] * 4], [[1.0] * 4, [0.01] * 4], [[0.0] * 4, [0.0] * 4])
    # row 1 looks periodic but its loudest frame has no energy
    assert est.voiced.tolist() == [False, False] and not est.frame_voiced.any()
    assert torch.isnan(est.midi).all() and (est.confidence == 0.0).all()
    with pytest.raises(ValueError):
        _agg([[8.0] * 4], [[1.0] * 3], [[0.0] * 4])
    with pytest.raises(ValueError):
        _agg([[8.0] * 4], [[1.0] * 4], [[0.0] * 4], min_voiced=0)


# ------------------------------------------------------------------------------------------------ retune
def _estimate(midi, voiced):
    from inverse_audio_synthesis_amd.pitch import PitchEstimate
    m = torch.tensor(midi, dtype=torch.float32)
    v = torch.tensor(voiced)
    return PitchEstimate(midi=torch.where(v, m, torch.full_like(m, float("nan"))), voiced=v,
                         confidence=v.float(), frame_midi=m[:, None], frame_voiced=v[:, None])


def test_retune_from_the_centre_and_with_tuning():
    from inverse_audio_synthesis_amd import voice_spec as S
    from inverse_audio_synthesis_amd.pitch import retune
    F0, T1, T2 = S.INDEX[("keyboard", "midi_f0")], S.INDEX[("vco_1", "tuning")], S.INDEX[("vco_2", "tuning")]
    M1, M2 = S.INDEX[("mixer", "vco_1")], S.INDEX[("mixer", "vco_2")]
    midi = [40.0, 57.3, 69.0, 61.25, 2.0, 126.0]
    est = _estimate(midi, [True, True, False, True, True, True])
    p = torch.full((6, 78), 0.5)
    out = retune(p, est)
    want = torch.tensor(midi, dtype=torch.float32) / 127.0
    for n in (0, 1, 3, 4, 5):
        assert out[n, F0] == want[n]                                    # exactly midi / 127
    assert out[2, F0] == 0.5                                            # unvoiced: untouched
    rest = [c for c in range(78) if c != F0]
    assert torch.equal(out[:, rest], p[:, rest]) and torch.equal(p, torch.full((6, 78), 0.5))

    g = torch.Generator().manual_seed(1)
    p = torch.rand((6, 78), generator=g)
    p[0, [M1, M2]] = torch.tensor([0.9, 0.2])                           # vco_1 louder
    p[1, [M1, M2]] = torch.tensor([0.1, 0.7])                           # vco_2 louder
    p[3, [M1, M2, T1, T2]] = torch.tensor([0.4, 0.4, 0.25, 0.75])       # a tie: vco_1
    p[4, [M1, M2, T1]] = torch.tensor([0.8, 0.1, 1.0])                  # midi 2 - 24 semitones: clamps at 0
    p[5, [M1, M2, T2]] = torch.tensor([0.1, 0.8, 0.0])                  # midi 126 + 24 semitones: clamps at 127
    out = retune(p, est)
    tun = lambda u: -24.0 + 48.0 * float(u)                             # noqa: E731
    assert float(out[0, F0]) == pytest.approx((40.0 - tun(p[0, T1])) / 127.0, abs=1e-6)
    assert float(out[1, F0]) == pytest.approx((57.3 - tun(p[1, T2])) / 127.0, abs=1e-6)
    assert float(out[3, F0]) == pytest.approx((61.25 - tun(p[3, T1])) / 127.0, abs=1e-6)
    assert abs(tun(p[3, T1]) - tun(p[3, T2])) > 1.0                     # the tie case tells the oscillators apart
    assert float(out[4, F0]) == 0.0 and float(out[5, F0]) == 1.0
    assert torch.equal(out[2], p[2]) and torch.equal(out[:, rest], p[:, rest])


def test_retune_several_starts_and_refusals():
    from inverse_audio_synthesis_amd import voice_spec as S
    from inverse_audio_synthesis_amd.pitch import retune
    F0 = S.INDEX[("keyboard", "midi_f0")]
    est = _estimate([48.0, 60.0], [True, False])
    p = torch.rand((2, 3, 78), generator=torch.Generator().manual_seed(2))
    out = retune(p, est)
    assert out.shape == p.shape and torch.equal(out[1], p[1])
    rest = [c for c in range(78) if c != F0]
    assert torch.equal(out[..., rest], p[..., rest])
    for s in range(3):
        assert torch.equal(out[0, s], retune(p[:, s].contiguous(), est)[0])
        assert out[0, s, F0] != p[0, s, F0]
    with pytest.raises(ValueError):
        retune(torch.rand(3, 78), est)
    with pytest.raises(ValueError):
        retune(torch.rand(2, 77), est)
    with pytest.raises(ValueError):
        retune(torch.rand(78), est)


def test_yin_plan():
    from inverse_audio_synthesis_amd.pitch import yin_plan, lds_bytes, LDS_BUDGET_BYTES
    assert yin_plan(44100) == (1604, 10, 1604)                          # 27.5 Hz .. 4186 Hz
    assert yin_plan(16000) == (582, 3, 582)
    assert yin_plan(16000, 36.0, 72.0) == (245, 30, 245)
    assert yin_plan(4000, 60.0, 120.0) == (16, 2, 16)                   # tau_min never under 2
    assert lds_bytes(1604, 1604) == 20 * 1604 + 44 <= LDS_BUDGET_BYTES
    with pytest.raises(ValueError):
        yin_plan(16000, 60.0, 60.0)


# ------------------------------------------------------------------------------------------------ match_audio.py flags
def test_match_audio_pitch_flags():
    import match_audio
    args, files, _o = match_audio.parse_args(["a.wav", "--out", "o"])
    assert args.pitch is False and (args.pitch_lo, args.pitch_hi) == (21.0, 108.0)
    args, files, _o = match_audio.parse_args(["a.wav", "--out", "o", "--pitch", "--pitch-lo", "36", "--pitch-hi", "84.5",
                                              "--init", "bank", "--starts", "4"])
    assert args.pitch is True and (args.pitch_lo, args.pitch_hi) == (36.0, 84.5) and files == ["a.wav"]
    for lo, hi in (("60", "60"), ("61", "60")):
        with pytest.raises(SystemExit) as e:
            match_audio.parse_args(["a.wav", "--out", "o", "--pitch", "--pitch-lo", lo, "--pitch-hi", hi])
        assert e.value.code == 2


# ------------------------------------------------------------------------------------------------ host-only C ABI
YIN_ARGS = ["const float* audio", "int B", "int T", "int W", "int tau_min", "int tau_max", "int hop", "float threshold",
            "float* period", "float* aperiodicity", "float* energy", "float* dprime", "void* stream"]


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "ias_hip.h")).read()
    m = re.search(r"\bint\s+ias_pitch_yin\s*\(([^)]*)\)\s*;", text)
    assert m, "include/ias_hip.h does not declare ias_pitch_yin"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == YIN_ARGS
    m = re.search(r"\blong long\s+ias_pitch_frames\s*\(([^)]*)\)\s*;", text)
    assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == ["int T", "int W", "int tau_max", "int hop"]


def test_pitch_frames(lib):
    assert lib.ias_pitch_frames(845, 512, 333, 1) == 1                  # T == W + tau_max: exactly one frame
    assert lib.ias_pitch_frames(846, 512, 333, 1) == 2
    assert lib.ias_pitch_frames(845, 512, 333, 97) == 1
    assert lib.ias_pitch_frames(4099, 200, 333, 97) == (4099 - 533) // 97 + 1 == 37
    assert lib.ias_pitch_frames(8000, 512, 512, 256) == 28
    assert lib.ias_pitch_frames(176400, 1604, 1604, 512) == 339
    assert lib.ias_pitch_frames(2 ** 31 - 1, 1, 1, 1) == 2 ** 31 - 2
    for a in ((844, 512, 333, 1), (0, 1, 1, 1), (100, 0, 10, 1), (100, 10, 0, 1), (100, 10, 10, 0), (-5, 1, 1, 1),
              (100, 2 ** 31 - 1, 2 ** 31 - 1, 1)):
        assert lib.ias_pitch_frames(*a) == -1, a


def test_pitch_yin_refuses_before_touching_the_device(lib):
    """Every refusal is decided on the host from the arguments alone: the pointers are never followed, nothing is
    launched, no GPU is needed."""
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(audio=p, B=2, T=4099, W=200, tau_min=5, tau_max=333, hop=97, thr=0.15, period=p, aper=p, energy=p,
             dprime=None):
        return lib.ias_pitch_yin(audio, B, T, W, tau_min, tau_max, hop, thr, period, aper, energy, dprime, None)
    bad = [dict(audio=None), dict(period=None), dict(aper=None), dict(energy=None), dict(B=0), dict(B=-1), dict(T=0),
           dict(W=0), dict(W=-4), dict(hop=0), dict(hop=-1), dict(tau_min=1), dict(tau_min=0), dict(tau_min=-3),
           dict(tau_min=334), dict(tau_max=4), dict(tau_max=0), dict(T=532), dict(T=200), dict(thr=0.0), dict(thr=-0.1),
           dict(thr=1.0000001), dict(thr=math.nan), dict(thr=math.inf), dict(W=2 ** 31 - 1, T=2 ** 31 - 1)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert call(dprime=p, **kw) == -1, kw
    # the LDS budget: 8 (tau_max + 1) + 4 (W + tau_max + 8) + 4 (tau_max + 1) <= 65536 bytes
    from inverse_audio_synthesis_amd.pitch import lds_bytes, LDS_BUDGET_BYTES
    assert lds_bytes(3274, 3274) < lds_bytes(3277, 3274) == LDS_BUDGET_BYTES < lds_bytes(3278, 3274) == lds_bytes(3274, 3275)
    assert LDS_BUDGET_BYTES < lds_bytes(16000, 100) and LDS_BUDGET_BYTES < lds_bytes(10, 4100)
    unsupported = [dict(W=3278, tau_max=3274, T=20000), dict(W=3274, tau_max=3275, T=20000),
                   dict(W=16000, tau_max=100, T=20000), dict(W=10, tau_max=4100, T=20000), dict(B=65536),
                   dict(dprime=p, B=65535, T=2 ** 30, hop=1),            # B F (tau_max + 1) past INT_MAX
                   dict(dprime=p, B=1, T=6429739 + 533, hop=1)]          # 6429740 frames x 334 = INT_MAX + 1513
    for kw in unsupported:
        assert call(**kw) == -2, kw
    # an argument error wins over a shape the kernel does not take
    assert call(B=65536, thr=2.0) == -1 and call(W=16000, tau_max=100, T=20000, tau_min=1) == -1

#!/usr/bin/env python3
"""Times the pitch estimator (inverse-audio-synthesis_amd/pitch.py) on one GPU and prints one JSON line.

    python scripts/bench_pitch.py [--reps 20] [--quality]

* ias_pitch_yin at (B, T) = (128, 176400) (128 sounds of 4 s @ 44.1 kHz) with ``estimate_pitch``'s defaults (lags of MIDI
  21..108: W = tau_max = 1604, tau_min = 10, hop 512: 339 frames per row), against its compute floor: 2 VALU instructions
  (a subtract and a fused multiply-add) per (lag, sample) pair on 256 CUs x 4 SIMD x 32 lanes at 2.4 GHz; and the whole
  ``estimate_pitch`` (the launch plus the aggregation's torch operations).
``--quality``: fit the 16 targets of DESIGN.md section 4.6 (rendered from a batch outside the bank) for 200 steps of mel-L1
from the centre, the centre retuned to the estimated note, the 4 nearest voices of a 4,096-voice bank, and those retuned;
report the final losses (median, range, wins and losses of the retuned starts) and the estimator's own error against the
targets' true sounding pitch (``keyboard.midi_f0`` plus the tuning of the louder oscillator) over the voiced ones.
Kernel-level figures: run it under ``rocprofv3 --kernel-trace --stats``."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_PER_S = 256 * 4 * 32 * 2.4e9


def _events_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def _summary(loss):
    return {"median": round(float(loss.median()), 4), "best": round(float(loss.min()), 4),
            "worst": round(float(loss.max()), 4), "all": [round(float(x), 4) for x in loss]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="launches per timing")
    ap.add_argument("--quality", action="store_true", help="also compare plain and retuned starts over 16 targets")
    args = ap.parse_args()

    import torch
    from inverse_audio_synthesis_amd import _lib
    from inverse_audio_synthesis_amd import voice_spec as S
    from inverse_audio_synthesis_amd.pitch import estimate_pitch, num_frames, retune, yin_plan
    from inverse_audio_synthesis_amd.voice import SynthConfig, Voice
    dev = torch.device("cuda:0")
    lib = _lib.load()
    B, rate, hop, thr = 128, 44100, 512, 0.15
    voice = Voice(SynthConfig(batch_size=B, sample_rate=rate, buffer_size_seconds=4.0, reproducible=False)).to(dev)
    T = voice.synthconfig.buffer_size
    audio = voice.render(torch.rand((B, 78), generator=torch.Generator().manual_seed(0)).to(dev))
    W, tau_min, tau_max = yin_plan(rate)
    F = num_frames(T, W, tau_max, hop)
    period = torch.empty((B, F), dtype=torch.float32, device=dev)
    aper, energy = torch.empty_like(period), torch.empty_like(period)

    def run():
        lib.ias_pitch_yin(_lib.ptr(audio), B, T, W, tau_min, tau_max, hop, thr, _lib.ptr(period), _lib.ptr(aper),
                          _lib.ptr(energy), None, _lib.stream())
    ms = _events_ms(run, args.reps)
    pairs = float(B) * F * W * tau_max
    out = {"bench": "pitch", "shape": [B, T], "W": W, "tau_min": tau_min, "tau_max": tau_max, "hop": hop, "frames": F,
           "pairs": pairs, "ias_pitch_yin_ms": round(ms, 3), "compute_floor_ms": round(2.0 * pairs / VALU_PER_S * 1e3, 3),
           "estimate_pitch_ms": round(_events_ms(lambda: estimate_pitch(audio, rate), max(2, args.reps // 4)), 3),
           "device": torch.cuda.get_device_name(dev)}
    out["floor_fraction"] = round(out["compute_floor_ms"] / out["ias_pitch_yin_ms"], 3)

    if args.quality:
        from inverse_audio_synthesis_amd.match import SoundMatcher
        from inverse_audio_synthesis_amd.retrieval import SpectralBank
        matcher = SoundMatcher(voice, loss="mel_l1", mel_kwargs=dict(n_fft=1024, hop_length=512, n_mels=128, power=2.0))
        truth01 = torch.rand((B, 78), generator=torch.Generator().manual_seed(10_000))[:16]
        tgt = voice.render(torch.rand((B, 78), generator=torch.Generator().manual_seed(10_000)).to(dev))[:16].contiguous()
        est = estimate_pitch(tgt, rate)
        second = truth01[:, S.INDEX[("mixer", "vco_2")]] > truth01[:, S.INDEX[("mixer", "vco_1")]]
        tuning01 = torch.where(second, truth01[:, S.INDEX[("vco_2", "tuning")]], truth01[:, S.INDEX[("vco_1", "tuning")]])
        true_midi = 127.0 * truth01[:, S.INDEX[("keyboard", "midi_f0")]] + (-24.0 + 48.0 * tuning01)
        voiced = est.voiced.cpu()
        err = (est.midi.cpu() - true_midi)[voiced].abs()
        steps = 200
        centre = torch.full((16, 78), 0.5, device=dev)
        bank = SpectralBank(voice, matcher.loss, range(32))
        _d, nb = bank.nearest(target_audio=tgt, k=4)
        starts = bank.params01[nb.reshape(-1)].reshape(16, 4, 78)
        fits = {"center": matcher.fit(tgt, steps=steps).loss.cpu(),
                "center_pitch": matcher.fit(tgt, init_params01=retune(centre, est), steps=steps).loss.cpu(),
                "bank": matcher.fit(tgt, init_params01=starts, steps=steps).loss.cpu(),
                "bank_pitch": matcher.fit(tgt, init_params01=retune(starts, est), steps=steps).loss.cpu()}
        q = {"targets": 16, "steps": steps, "bank_voices": 4096, "starts": 4, "voiced": int(voiced.sum()),
             "true_midi": [round(float(x), 2) for x in true_midi],
             "estimated_midi": [round(float(x), 2) if v else None for x, v in zip(est.midi.cpu(), voiced)],
             "confidence": [round(float(x), 3) for x in est.confidence.cpu()],
             "estimate_abs_error_median": round(float(err.median()), 3) if len(err) else None,
             "estimate_abs_error_max": round(float(err.max()), 3) if len(err) else None,
             "estimate_within_half_semitone": int((err <= 0.5).sum())}
        for k, v in fits.items():
            q[k] = _summary(v)
        for a, b in (("center", "center_pitch"), ("bank", "bank_pitch")):
            q[b + "_wins"] = int((fits[b] < fits[a]).sum())
            q[b + "_losses"] = int((fits[b] > fits[a]).sum())
        out["quality"] = q
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

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

import bench_common as bc

VALU_PER_S = 256 * 4 * 32 * 2.4e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="launches per timing")
    ap.add_argument("--quality", action="store_true", help="also compare plain and retuned starts over 16 targets")
    args = ap.parse_args()

    import torch
    from inverse_audio_synthesis_amd import _lib
    from inverse_audio_synthesis_amd import voice_spec as S
    from inverse_audio_synthesis_amd.pitch import estimate_pitch, num_frames, retune, yin_plan
    dev = torch.device("cuda:0")
    lib = _lib.load()
    B, rate, hop, thr = 128, 44100, 512, 0.15
    voice = bc.design_voice(dev)
    T = voice.synthconfig.buffer_size
    audio = voice.render(torch.rand((B, 78), generator=torch.Generator().manual_seed(0)).to(dev))
    W, tau_min, tau_max = yin_plan(rate)
    F = num_frames(T, W, tau_max, hop)
    period = torch.empty((B, F), dtype=torch.float32, device=dev)
    aper, energy = torch.empty_like(period), torch.empty_like(period)

    def run():
        lib.ias_pitch_yin(_lib.ptr(audio), B, T, W, tau_min, tau_max, hop, thr, _lib.ptr(period), _lib.ptr(aper),
                          _lib.ptr(energy), None, _lib.stream())
    ms = bc.event_ms(run, args.reps)[0]
    pairs = float(B) * F * W * tau_max
    out = {"bench": "pitch", "shape": [B, T], "W": W, "tau_min": tau_min, "tau_max": tau_max, "hop": hop, "frames": F,
           "pairs": pairs, "ias_pitch_yin_ms": round(ms, 3), "compute_floor_ms": round(2.0 * pairs / VALU_PER_S * 1e3, 3),
           "estimate_pitch_ms": round(bc.event_ms(lambda: estimate_pitch(audio, rate), max(2, args.reps // 4))[0], 3),
           "device": torch.cuda.get_device_name(dev)}
    out["floor_fraction"] = round(out["compute_floor_ms"] / out["ias_pitch_yin_ms"], 3)

    if args.quality:
        from inverse_audio_synthesis_amd.retrieval import SpectralBank
        matcher = bc.mel_matcher(voice)
        truth01, tgt = bc.target_params01(), bc.targets(voice)
        est = estimate_pitch(tgt, rate)
        second = truth01[:, S.INDEX[("mixer", "vco_2")]] > truth01[:, S.INDEX[("mixer", "vco_1")]]
        tuning01 = torch.where(second, truth01[:, S.INDEX[("vco_2", "tuning")]], truth01[:, S.INDEX[("vco_1", "tuning")]])
        true_midi = 127.0 * truth01[:, S.INDEX[("keyboard", "midi_f0")]] + (-24.0 + 48.0 * tuning01)
        voiced = est.voiced.cpu()
        err = (est.midi.cpu() - true_midi)[voiced].abs()
        centre = torch.full((bc.TARGETS, 78), 0.5, device=dev)
        _d, starts = bc.nearest_starts(SpectralBank(voice, matcher.loss, range(bc.BANK_BATCHES)), tgt)
        _fits, summaries = bc.fit_starts(matcher, tgt, {"center": None, "center_pitch": retune(centre, est), "bank": starts,
                                                        "bank_pitch": retune(starts, est)},
                                         pairs=[("center", "center_pitch"), ("bank", "bank_pitch")])
        q = {"targets": bc.TARGETS, "steps": bc.FIT_STEPS, "bank_voices": bc.BANK_BATCHES * B, "starts": bc.STARTS,
             "voiced": int(voiced.sum()),
             "true_midi": [round(float(x), 2) for x in true_midi],
             "estimated_midi": [round(float(x), 2) if v else None for x, v in zip(est.midi.cpu(), voiced)],
             "confidence": [round(float(x), 3) for x in est.confidence.cpu()],
             "estimate_abs_error_median": round(float(err.median()), 3) if len(err) else None,
             "estimate_abs_error_max": round(float(err.max()), 3) if len(err) else None,
             "estimate_within_half_semitone": int((err <= 0.5).sum())}
        out["quality"] = {**q, **summaries}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

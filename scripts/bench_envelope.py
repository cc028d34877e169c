#!/usr/bin/env python3
"""Times the envelope stage (inverse-audio-synthesis_amd/envelope.py) on one GPU and prints one JSON line.

    python scripts/bench_envelope.py [--reps 200] [--passes 3] [--quality] [--no-headline]

128 sounds of 4 s @ 44.1 kHz with ``fit_envelope``'s defaults (W 1024, hop 256: 686 frames; 512 candidates per sound).
Isolated and by device events over ``--reps`` launches, ``--passes`` times (min / median / max reported):
* ias_envelope_frames, against the time its audio takes through HBM at 8 TB/s once;
* ias_envelope_score on a population drawn by ias_evolve_sample from the centre at sigma 0.3, against its fp64 floor:
  ``FP64_PER_PAIR`` fp64 vector instructions per (candidate, frame), counted in the kernel's ISA,
  at 16 lanes per clock on 256 CUs x 4 SIMDs at 2.4 GHz;
and the whole ``fit_envelope`` (16 generations), by a host clock around a device synchronise.
``--quality``: fit the 16 targets of DESIGN.md section 4.6 (rendered from a batch outside the bank) for 200 steps of mel-L1
from the centre, the centre reshaped by the fitted envelope, the 4 nearest voices of a 4,096-voice bank, and those reshaped;
report the final losses (median, best, worst, wins and losses of the reshaped starts) and the fits' envelope distances.
Unless ``--no-headline``: the headline step (``bench.py --gpus 1``) and one matcher iteration (``scripts/bench_match.py``)
on the same machine in the same run, each in a process of its own before this one opens the GPU.
Kernel-level figures: run it under ``rocprofv3 --kernel-trace --stats``."""
import argparse
import json
import os
import time

import bench_common as bc
from bench_common import ROOT

HBM_BYTES_PER_S = 8e12
FP64_LANES_PER_S = 256 * 4 * 16 * 2.4e9
FP64_PER_PAIR = 195                # fp64 vector instructions of the scorer's frame loop, the one pow included


def _events_us(fn, reps, passes):
    return bc.spread(bc.event_ms(fn, reps, passes), 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="launches per timing window")
    ap.add_argument("--passes", type=int, default=3, help="timing windows per figure")
    ap.add_argument("--quality", action="store_true", help="also compare plain and reshaped starts over 16 targets")
    ap.add_argument("--no-headline", action="store_true", help="skip the headline step and the matcher iteration")
    args = ap.parse_args()

    out = {"bench": "envelope"}
    if not args.no_headline:
        head = bc.json_line([os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "100", "--warmup", "5"])
        out["headline_step_ms"] = head["ms_per_step"]
        out["matcher_iter_ms"] = bc.json_line([os.path.join(ROOT, "scripts", "bench_match.py")])["iter_ms"]

    import torch
    from inverse_audio_synthesis_amd import _lib
    from inverse_audio_synthesis_amd import voice_spec as S
    from inverse_audio_synthesis_amd.envelope import envelope_score, fit_envelope, num_frames, reshape
    from inverse_audio_synthesis_amd.evolve import evolve_sample
    dev = torch.device("cuda:0")
    lib = _lib.load()
    B, rate, W, hop, M = 128, 44100, 1024, 256, 512
    voice = bc.design_voice(dev)
    T = voice.synthconfig.buffer_size
    audio = voice.render(torch.rand((B, 78), generator=torch.Generator().manual_seed(0)).to(dev))
    F = num_frames(T, W, hop)
    rms = torch.empty((B, F), dtype=torch.float32, device=dev)

    def frames():
        lib.ias_envelope_frames(_lib.ptr(audio), B, T, W, hop, _lib.ptr(rms), _lib.stream())
    frames_us = _events_us(frames, args.reps, args.passes)
    pop = torch.empty((B, M, 6), dtype=torch.float32, device=dev)
    evolve_sample(torch.full((B, 6), 0.5, device=dev), torch.full((B, 6), 0.3, device=dev),
                  torch.ones(6, dtype=torch.uint8, device=dev), 0, 0, pop)
    dist = torch.empty((B, M), dtype=torch.float32, device=dev)
    t0, dt = (W / 2.0) / rate, hop / rate
    score_us = _events_us(lambda: envelope_score(rms, pop, t0, dt, out=dist), max(1, args.reps // 4), args.passes)

    def fit_ms():
        torch.cuda.synchronize()
        start = time.perf_counter()
        fit_envelope(audio, rate)
        torch.cuda.synchronize()
        return (time.perf_counter() - start) * 1e3
    fit_ms()
    fits_ms = [fit_ms() for _ in range(args.passes)]
    pairs = float(B) * M * F
    out.update({"shape": [B, T], "W": W, "hop": hop, "frames": F, "population": M, "device": torch.cuda.get_device_name(dev),
                "reps": args.reps, "passes": args.passes, "ias_envelope_frames_us": frames_us,
                "audio_bytes": 4.0 * B * T, "audio_hbm_us": round(4.0 * B * T / HBM_BYTES_PER_S * 1e6, 2),
                "ias_envelope_score_us": score_us, "pairs": pairs, "fp64_per_pair": FP64_PER_PAIR,
                "score_fp64_floor_us": round(pairs * FP64_PER_PAIR / FP64_LANES_PER_S * 1e6, 2),
                "fit_envelope_ms": bc.spread(fits_ms, digits=3)})

    if args.quality:
        from inverse_audio_synthesis_amd.retrieval import SpectralBank
        matcher = bc.mel_matcher(voice)
        tgt = bc.targets(voice)
        fit = fit_envelope(tgt, rate)
        u = bc.target_params01()[:, S.INDEX[("keyboard", "duration")]]
        centre = torch.full((bc.TARGETS, 78), 0.5, device=dev)
        _d, starts = bc.nearest_starts(SpectralBank(voice, matcher.loss, range(bc.BANK_BATCHES)), tgt)
        _fits, summaries = bc.fit_starts(matcher, tgt, {"center": None, "center_envelope": reshape(centre, fit),
                                                        "bank": starts, "bank_envelope": reshape(starts, fit)},
                                         pairs=[("center", "center_envelope"), ("bank", "bank_envelope")])
        q = {"targets": bc.TARGETS, "steps": bc.FIT_STEPS, "bank_voices": bc.BANK_BATCHES * B, "starts": bc.STARTS,
             "sounding": int(fit.sounding.sum()),
             "envelope_distance": [round(float(x), 5) for x in fit.dist.cpu()],
             "envelope_start_distance": [round(float(x), 5) for x in fit.start_dist.cpu()],
             "true_duration_s": [round(float(x), 3) for x in 0.01 + 3.99 * u.double() ** 2],
             "fitted_duration_s": [round(float(x), 3) for x in fit.units[:, 0].cpu()]}
        out["quality"] = {**q, **summaries}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

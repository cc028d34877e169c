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
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
FP64_LANES_PER_S = 256 * 4 * 16 * 2.4e9
FP64_PER_PAIR = 195                # fp64 vector instructions of the scorer's frame loop, the one pow included


def _events_us(fn, reps, passes):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(passes):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return {"min": round(min(out), 2), "median": round(statistics.median(out), 2), "max": round(max(out), 2)}


def _json_line(cmd):
    """Run a benchmark of the project in a process of its own -> the last JSON line it printed."""
    r = subprocess.run([sys.executable] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or not lines:
        raise RuntimeError(f"{' '.join(cmd)} failed:\n{r.stdout[-2000:]}")
    return json.loads(lines[-1])


def _summary(loss):
    return {"median": round(float(loss.median()), 4), "best": round(float(loss.min()), 4),
            "worst": round(float(loss.max()), 4), "all": [round(float(x), 4) for x in loss]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="launches per timing window")
    ap.add_argument("--passes", type=int, default=3, help="timing windows per figure")
    ap.add_argument("--quality", action="store_true", help="also compare plain and reshaped starts over 16 targets")
    ap.add_argument("--no-headline", action="store_true", help="skip the headline step and the matcher iteration")
    args = ap.parse_args()

    out = {"bench": "envelope"}
    if not args.no_headline:
        head = _json_line([os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "100", "--warmup", "5"])
        out["headline_step_ms"] = head["ms_per_step"]
        out["matcher_iter_ms"] = _json_line([os.path.join(ROOT, "scripts", "bench_match.py")])["iter_ms"]

    import torch
    from inverse_audio_synthesis_amd import _lib
    from inverse_audio_synthesis_amd import voice_spec as S
    from inverse_audio_synthesis_amd.envelope import envelope_score, fit_envelope, num_frames, reshape
    from inverse_audio_synthesis_amd.evolve import evolve_sample
    from inverse_audio_synthesis_amd.voice import SynthConfig, Voice
    dev = torch.device("cuda:0")
    lib = _lib.load()
    B, rate, W, hop, M = 128, 44100, 1024, 256, 512
    voice = Voice(SynthConfig(batch_size=B, sample_rate=rate, buffer_size_seconds=4.0, reproducible=False)).to(dev)
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
                "fit_envelope_ms": {"min": round(min(fits_ms), 3), "median": round(statistics.median(fits_ms), 3),
                                    "max": round(max(fits_ms), 3)}})

    if args.quality:
        from inverse_audio_synthesis_amd.match import SoundMatcher
        from inverse_audio_synthesis_amd.retrieval import SpectralBank
        matcher = SoundMatcher(voice, loss="mel_l1", mel_kwargs=dict(n_fft=1024, hop_length=512, n_mels=128, power=2.0))
        tgt = voice.render(torch.rand((B, 78), generator=torch.Generator().manual_seed(10_000)).to(dev))[:16].contiguous()
        fit = fit_envelope(tgt, rate)
        u = torch.rand((B, 78), generator=torch.Generator().manual_seed(10_000))[:16, S.INDEX[("keyboard", "duration")]]
        steps = 200
        centre = torch.full((16, 78), 0.5, device=dev)
        bank = SpectralBank(voice, matcher.loss, range(32))
        _d, nb = bank.nearest(target_audio=tgt, k=4)
        starts = bank.params01[nb.reshape(-1)].reshape(16, 4, 78)
        fits = {"center": matcher.fit(tgt, steps=steps).loss.cpu(),
                "center_envelope": matcher.fit(tgt, init_params01=reshape(centre, fit), steps=steps).loss.cpu(),
                "bank": matcher.fit(tgt, init_params01=starts, steps=steps).loss.cpu(),
                "bank_envelope": matcher.fit(tgt, init_params01=reshape(starts, fit), steps=steps).loss.cpu()}
        q = {"targets": 16, "steps": steps, "bank_voices": 4096, "starts": 4, "sounding": int(fit.sounding.sum()),
             "envelope_distance": [round(float(x), 5) for x in fit.dist.cpu()],
             "envelope_start_distance": [round(float(x), 5) for x in fit.start_dist.cpu()],
             "true_duration_s": [round(float(x), 3) for x in 0.01 + 3.99 * u.double() ** 2],
             "fitted_duration_s": [round(float(x), 3) for x in fit.units[:, 0].cpu()]}
        for k, v in fits.items():
            q[k] = _summary(v)
        for a, b in (("center", "center_envelope"), ("bank", "bank_envelope")):
            q[b + "_wins"] = int((fits[b] < fits[a]).sum())
            q[b + "_losses"] = int((fits[b] > fits[a]).sum())
        out["quality"] = q
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

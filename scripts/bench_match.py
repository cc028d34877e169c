#!/usr/bin/env python3
"""Times sound matching (inverse-audio-synthesis_amd/match.py) on one GPU and prints one JSON line.

    python scripts/bench_match.py [--batch 128] [--rate 44100] [--seconds 4] [--steps 20] [--warmup 3] [--loss mel_l1]

* ms per matcher iteration: SoundMatcher.fit over one chunk of ``--batch`` sounds with W and W + K steps, the difference
  over K (render with its adjoint, per-sound loss and its adjoint, update: everything one iteration issues);
* the per-row L1 (ias_l1_rows: partials + fold) on the loss' [B, frames, n_out] values, against the time to read its two
  operands at 8 TB/s; with ``--loss multi_resolution_stft`` the per-row MR-STFT sums (ias_mrstft_rows) of the three
  resolutions against the same floor for their six operands, and the per-row coefficient (ias_mrstft_coef_rows, one per
  resolution) and total (ias_mrstft_rows_total) launches;
* the update kernel (ias_match_adam_step) on [B, 78].
Kernel-level figures: run it under ``rocprofv3 --kernel-trace --stats``."""
import argparse
import json
import time

import bench_common as bc


def _mrstft_parts(loss, audio, target, reps):
    """The per-row MR-STFT pieces alone on the loss' own shapes: ias_mrstft_rows of every resolution (partials + fold), one
    ias_mrstft_coef_rows and the ias_mrstft_rows_total launch."""
    import ctypes
    import torch
    from inverse_audio_synthesis_amd import _lib
    from inverse_audio_synthesis_amd.spectral import VALUE_MAG_CLAMPED
    lib = _lib.load()
    B = audio.shape[0]
    tgts = loss.target(target)
    vals = [plan.values(audio, VALUE_MAG_CLAMPED, loss.eps) for plan in loss.plans]
    sums = [plan.mrstft_rows(v, t) for plan, v, t in zip(loss.plans, vals, tgts)]
    rows_us = [bc.event_ms(lambda p=plan, v=v, t=t: p.mrstft_rows(v, t), reps)[0] * 1e3
               for plan, v, t in zip(loss.plans, vals, tgts)]
    nbytes = sum(2 * v.numel() * 4 for v in vals)
    g = torch.ones(B, device=audio.device)
    coef = torch.empty((B, 2), dtype=torch.float64, device=audio.device)
    count = float(tgts[0][0].numel())
    coef_us = bc.event_ms(lambda: lib.ias_mrstft_coef_rows(_lib.ptr(sums[0]), _lib.ptr(g), count, len(sums), B,
                                                          _lib.ptr(coef), _lib.stream()), reps)[0] * 1e3
    out = torch.empty(B, dtype=torch.float32, device=audio.device)
    ptrs = (ctypes.c_void_p * len(sums))(*[s.data_ptr() for s in sums])
    counts = (ctypes.c_double * len(sums))(*[float(t[0].numel()) for t in tgts])
    total_us = bc.event_ms(lambda: lib.ias_mrstft_rows_total(ptrs, counts, len(sums), B, _lib.ptr(out), _lib.stream()),
                          reps)[0] * 1e3
    return {"mrstft_rows_us": round(sum(rows_us), 2), "mrstft_rows_us_per_resolution": [round(u, 2) for u in rows_us],
            "mrstft_rows_bytes": nbytes, "mrstft_rows_hbm_floor_us": round(nbytes / 8e12 * 1e6, 2),
            "mrstft_coef_rows_us": round(coef_us, 2), "mrstft_rows_total_us": round(total_us, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loss", choices=("mel_l1", "stft_l1", "multi_resolution_stft"), default="mel_l1")
    ap.add_argument("--reps", type=int, default=200, help="launches per kernel timing")
    args = ap.parse_args()

    import torch
    from inverse_audio_synthesis_amd.match import SoundMatcher, match_adam_step
    from inverse_audio_synthesis_amd.voice import SynthConfig, Voice
    dev = torch.device("cuda:0")
    B = args.batch
    voice = Voice(SynthConfig(batch_size=B, sample_rate=args.rate, buffer_size_seconds=args.seconds,
                              reproducible=False)).to(dev)
    gen = torch.Generator().manual_seed(0)
    target = voice.render(torch.rand((B, 78), generator=gen).to(dev))
    init = torch.rand((B, 78), generator=gen).to(dev)
    matcher = SoundMatcher(voice, loss=args.loss, mel_kwargs=bc.MEL,
                           stft_kwargs=dict(n_fft=1024, hop_length=512, power=1.0), lr=0.01)

    def fit_s(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = matcher.fit(target, init_params01=init, steps=steps)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    fit_s(args.warmup)                                       # first use: allocations, tables
    t_w, _ = fit_s(args.warmup)
    t_wk, res = fit_s(args.warmup + args.steps)
    iter_ms = (t_wk - t_w) / args.steps * 1e3

    if args.loss == "multi_resolution_stft":
        rows = _mrstft_parts(matcher.loss, voice.render(init), target, args.reps)
    else:
        # the per-row L1 alone, on the loss' own value shapes
        plan = matcher.loss.mel.plan if args.loss == "mel_l1" else matcher.loss.plan
        vals = plan.values(voice.render(init), matcher.loss.mel.value_mode if args.loss == "mel_l1" else matcher.loss.value_mode)
        tgt = matcher.loss.target(target)
        l1_ms = bc.event_ms(lambda: plan.l1_rows(vals, tgt), args.reps)[0]
        floor_us = 2 * vals.numel() * 4 / 8e12 * 1e6
        rows = {"l1_rows_us": round(l1_ms * 1e3, 2), "l1_rows_bytes": 2 * vals.numel() * 4,
                "l1_rows_hbm_floor_us": round(floor_us, 2)}

    # the update kernel alone (all rows active, every column free, finite inputs)
    p = init.clone()
    grad = torch.randn((B, 78), generator=gen).to(dev) * 1e-3
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    step = torch.zeros(B, dtype=torch.int32, device=dev)
    skipped = torch.zeros(B, dtype=torch.int32, device=dev)
    best_loss = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)
    best_params = p.clone()
    loss = torch.ones(B, device=dev)
    free = torch.ones(78, dtype=torch.uint8, device=dev)
    active = torch.ones(B, dtype=torch.uint8, device=dev)
    adam_ms = bc.event_ms(lambda: match_adam_step(p, grad, m, v, step, loss, best_loss, best_params, free, active, skipped,
                                                 1e-4, (0.9, 0.999), 1e-8), args.reps)[0]
    out = {"workload": "match", "loss": args.loss, "batch": B, "T": voice.synthconfig.buffer_size, "steps": args.steps,
           "iter_ms": round(iter_ms, 4), **rows, "adam_step_us": round(adam_ms * 1e3, 2),
           "final_over_initial_median": round(float((res.loss / res.initial_loss).median()), 4),
           "device": torch.cuda.get_device_name(dev)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

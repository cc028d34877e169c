#!/usr/bin/env python3
"""Times the tied sound-matching step and iteration (inverse-audio-synthesis_amd/match.py: tied_adam_step, fit_tied) on one
GPU in one run, with device events, and prints one JSON line; ``--study`` adds a second line, the quality study of
DESIGN.md section 4.13.  No test asserts on it.

    python scripts/bench_tied.py [--reps 200] [--passes 5] [--steps 20] [--warmup 3] [--study] [--study-steps 200]

* ias_match_tied_step at N = 128, P = 78 with G = 128, 16 and 1 (every column free, the two keyboard columns own, finite
  inputs) against ias_match_adam_step at the same size: ``--passes`` windows of ``--reps`` launches each, the four
  timed in turn within every pass.  All four move a few hundred KB and are bound by launch latency; the figure of
  interest is whether G = 1, one workgroup walking 128 rows, stays near the others.
* one tied iteration at B = 128, 4 s @ 44.1 kHz, 16 groups of 8 (fit_tied with W and W + K steps, the difference over K,
  between two device events) against scripts/bench_match.py's iteration (fit, timed the same way here).
* ``--study``: a phrase of four notes (the MIDI notes of tests/onset_model.py: 48, 60, 55, 67) rendered from ONE hidden
  random preset at 16 kHz, 1 s, matched per note (fit) and shared (fit_tied) from the same start (the centre, every
  note's keyboard.midi_f0 and keyboard.duration at the truth), with the same steps, for ``--study-presets`` presets:
  final mel-L1 per note and the mean absolute error of the tied columns against the hidden preset."""
import argparse
import json

import bench_common as bc

NOTES_MIDI = (48.0, 60.0, 55.0, 67.0)


def _step_state(N, G, dev, gen):
    import torch
    p = torch.rand((N, 78), generator=gen).to(dev)
    st = dict(p=p, grad=(torch.randn((N, 78), generator=gen) * 1e-3).to(dev), m=torch.zeros_like(p), v=torch.zeros_like(p),
              best=p.clone(), loss=torch.ones(N, device=dev), step=torch.zeros(G, dtype=torch.int32, device=dev),
              skipped=torch.zeros(G, dtype=torch.int32, device=dev),
              best_loss=torch.full((G,), float("inf"), dtype=torch.float64, device=dev),
              group_loss=torch.zeros(G, dtype=torch.float64, device=dev),
              group_start=(torch.arange(G + 1, dtype=torch.int32) * (N // G)).to(dev),
              active=torch.ones(G, dtype=torch.uint8, device=dev))
    return st


def step_times(args, dev):
    import torch
    from inverse_audio_synthesis_amd.match import match_adam_step, tied_adam_step
    N = 128
    gen = torch.Generator().manual_seed(0)
    free = torch.ones(78, dtype=torch.uint8, device=dev)
    tied = free.clone()
    tied[:2] = 0
    calls = {}
    for G in (128, 16, 1):
        s = _step_state(N, G, dev, gen)
        calls[f"tied_step_us_G{G}"] = lambda s=s: tied_adam_step(
            s["p"], s["grad"], s["m"], s["v"], s["best"], s["loss"], s["group_start"], s["step"], s["skipped"], s["best_loss"],
            s["group_loss"], free, tied, s["active"], 1, 1e-4, (0.9, 0.999), 1e-8)
    s = _step_state(N, N, dev, gen)
    calls["adam_step_us"] = lambda: match_adam_step(s["p"], s["grad"], s["m"], s["v"], s["step"], s["loss"], s["best_loss"],
                                                    s["best"], free, s["active"], s["skipped"], 1e-4, (0.9, 0.999), 1e-8)
    times = {k: [] for k in calls}
    for _ in range(args.passes):                             # the four in turn within every pass
        for k, fn in calls.items():
            times[k] += bc.event_ms(fn, args.reps)
    return {k: bc.spread(t, 1e3) for k, t in times.items()}


def iteration_times(args, dev):
    import torch
    voice = bc.design_voice(dev)
    matcher = bc.mel_matcher(voice)
    gen = torch.Generator().manual_seed(0)
    target = voice.render(torch.rand((128, 78), generator=gen).to(dev))
    init = torch.rand((128, 78), generator=gen).to(dev)
    groups = torch.arange(128) // 8

    def ms(fn, steps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(steps)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    fits = {"tied_iter_ms": lambda n: matcher.fit_tied(target, groups, init_params01=init, steps=n),
            "untied_iter_ms": lambda n: matcher.fit(target, init_params01=init, steps=n)}
    out = {}
    for k, fn in fits.items():
        ms(fn, args.warmup)                                  # first use: allocations, tables
        per = []
        for _ in range(3):
            t_w = ms(fn, args.warmup)
            per.append((ms(fn, args.warmup + args.steps) - t_w) / args.steps)
        out[k] = bc.spread(per, 1.0, 4)
    return out


def study(args, dev):
    import torch
    from inverse_audio_synthesis_amd import voice_spec as S
    from inverse_audio_synthesis_amd.match import DEFAULT_OWN, SoundMatcher
    from inverse_audio_synthesis_amd.voice import SynthConfig, Voice
    voice = Voice(SynthConfig(batch_size=4, sample_rate=16000, buffer_size_seconds=1.0, reproducible=False)).to(dev)
    matcher = SoundMatcher(voice, loss="mel_l1", mel_kwargs=bc.MEL)
    own = [S.INDEX[k] for k in DEFAULT_OWN]
    tied = matcher.tied_mask().bool()
    rows = []
    for seed in range(args.study_presets):
        truth = torch.rand((1, 78), generator=torch.Generator().manual_seed(20_000 + seed)).repeat(4, 1)
        truth[:, S.INDEX[("keyboard", "midi_f0")]] = torch.tensor(NOTES_MIDI) / 127.0
        truth = truth.to(dev)
        target = voice.render(truth)
        init = torch.full((4, 78), 0.5, device=dev)
        init[:, own] = truth[:, own]
        per_note = matcher.fit(target, init_params01=init, steps=args.study_steps)
        shared = matcher.fit_tied(target, torch.zeros(4, dtype=torch.int64), init_params01=init, steps=args.study_steps)
        err = lambda p: float((p[:, tied] - truth[:, tied]).abs().mean())     # noqa: E731
        rows.append({"preset_seed": 20_000 + seed, "initial_loss": bc.rounded(per_note.initial_loss),
                     "per_note_loss": bc.rounded(per_note.loss), "shared_loss": bc.rounded(shared.loss),
                     "per_note_mean_loss": round(float(per_note.loss.double().mean()), 4),
                     "shared_mean_loss": round(float(shared.group_loss[0]), 4),
                     "start_tied_abs_err": round(err(init), 4), "per_note_tied_abs_err": round(err(per_note.params01), 4),
                     "shared_tied_abs_err": round(err(shared.params01), 4)})
    return {"workload": "tied_study", "steps": args.study_steps, "rate": 16000, "seconds": 1.0, "notes_midi": NOTES_MIDI,
            "presets": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="launches per timing window")
    ap.add_argument("--passes", type=int, default=5, help="timing windows per kernel")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--study", action="store_true")
    ap.add_argument("--study-steps", type=int, default=200)
    ap.add_argument("--study-presets", type=int, default=4)
    args = ap.parse_args()

    import torch
    dev = torch.device("cuda:0")
    out = {"workload": "tied", "N": 128, "P": 78, "reps": args.reps, "passes": args.passes, **step_times(args, dev),
           "batch": 128, "T": 176400, "groups": 16, "steps": args.steps, **iteration_times(args, dev),
           "device": torch.cuda.get_device_name(dev)}
    print(json.dumps(out), flush=True)
    if args.study:
        print(json.dumps(study(args, dev)), flush=True)


if __name__ == "__main__":
    main()

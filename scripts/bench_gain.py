#!/usr/bin/env python3
"""Times the output-gain entry points (include/ias_hip_gain.h) and a gained matcher iteration
(inverse-audio-synthesis_amd/match.py: SoundMatcher.fit(gain="fitted")) on one GPU in one run, with device events, and
prints one JSON line.  No test asserts on it.

    python scripts/bench_gain.py [--reps 50] [--passes 5] [--steps 20] [--warmup 3] [--rounds 3]

* ias_gain_apply, ias_gain_backward and ias_gain_solve alone at B = 128, T = 176400 (4 s @ 44.1 kHz): ``--passes`` windows
  of ``--reps`` launches each, the three timed in turn within every pass.  Every launch takes the next of ``SETS`` sets of
  buffers, so a window walks more bytes than the 256 MB last-level cache holds and times HBM.  The floors at 8 TB/s: apply
  and solve move two arrays of 90.3 MB (22.6 us), backward three (33.9 us); ``x_floor`` is the median over the floor.
* one matcher iteration at B = 128 with gain="fitted" against gain=None, in alternating runs on the same box: fit with W
  and W + K steps, the difference over K, between two device events (the method of scripts/bench_match.py)."""
import argparse
import json

import bench_common as bc

B, T, SETS = 128, 176400, 4
HBM_BYTES_PER_US = 8e6                               # 8 TB/s


def kernel_times(args, dev):
    import torch
    gen = torch.Generator(device=dev).manual_seed(0)
    audio = [torch.randn((B, T), device=dev, generator=gen) for _ in range(SETS)]
    g_out = [torch.randn((B, T), device=dev, generator=gen) for _ in range(SETS)]
    g01 = torch.rand(B, device=dev, generator=gen)
    # the entry points themselves, on buffers and pointers made beforehand: a Python wrapper's checks and allocations take
    # as long as one of these launches
    from inverse_audio_synthesis_amd import _lib
    lib, P, st = _lib.load(), _lib.ptr, _lib.stream()
    n = lib.ias_gain_partials_count(T)
    out, vec = torch.empty((B, T), device=dev), torch.empty(B, device=dev)
    partials = torch.empty((B, n, 2), dtype=torch.float64, device=dev)
    pa, pg = [P(t) for t in audio], [P(t) for t in g_out]
    pg01, pout, pvec, ppart = P(g01), P(out), P(vec), P(partials)
    turn = {"n": 0}

    def each(fn):
        def call():
            turn["n"] += 1
            _lib.check(fn(turn["n"] % SETS), "bench_gain")
        return call

    calls = {"apply_us": each(lambda i: lib.ias_gain_apply(pa[i], pg01, pout, B, T, st)),
             "backward_us": each(lambda i: lib.ias_gain_backward(pg[i], pa[i], pg01, pout, pvec, ppart, B, T, st)),
             "solve_us": each(lambda i: lib.ias_gain_solve(pg[i], pa[i], pvec, ppart, B, T, st))}
    arrays = {"apply_us": 2, "backward_us": 3, "solve_us": 2}
    times = {k: [] for k in calls}
    for _ in range(args.passes):                             # the three in turn within every pass
        for k, fn in calls.items():
            times[k] += bc.event_ms(fn, args.reps)
    out = {}
    for k, t in times.items():
        floor = arrays[k] * B * T * 4 / HBM_BYTES_PER_US
        out[k] = {**bc.spread(t, 1e3), "floor": round(floor, 1)}
        out[k]["x_floor"] = round(out[k]["median"] / floor, 2)
    return out


def iteration_times(args, dev):
    import torch
    voice = bc.design_voice(dev)
    matcher = bc.mel_matcher(voice)
    gen = torch.Generator().manual_seed(0)
    target = 0.125 * voice.render(torch.rand((B, 78), generator=gen).to(dev))
    init = torch.rand((B, 78), generator=gen).to(dev)

    def ms(fn, steps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(steps)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    fits = {"gain_fitted_iter_ms": lambda n: matcher.fit(target, init_params01=init, steps=n, gain="fitted"),
            "no_gain_iter_ms": lambda n: matcher.fit(target, init_params01=init, steps=n)}
    per = {k: [] for k in fits}
    for fn in fits.values():
        ms(fn, args.warmup)                                  # first use: allocations, tables
    for _ in range(args.rounds):                             # alternating: a drift of the box shows in both
        for k, fn in fits.items():
            t_w = ms(fn, args.warmup)
            per[k].append((ms(fn, args.warmup + args.steps) - t_w) / args.steps)
    out = {k: bc.spread(t, 1.0, 4) for k, t in per.items()}
    out["gain_overhead_ms"] = round(out["gain_fitted_iter_ms"]["median"] - out["no_gain_iter_ms"]["median"], 4)
    out["gain_overhead_rel"] = round(out["gain_overhead_ms"] / out["no_gain_iter_ms"]["median"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50, help="launches per timing window")
    ap.add_argument("--passes", type=int, default=5, help="timing windows per kernel")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="alternating runs of the two iterations")
    args = ap.parse_args()

    import torch
    dev = torch.device("cuda:0")
    out = {"workload": "gain", "batch": B, "T": T, "buffer_sets": SETS, "reps": args.reps, "passes": args.passes,
           **kernel_times(args, dev)}
    torch.cuda.empty_cache()
    out.update({"steps": args.steps, "rounds": args.rounds, **iteration_times(args, dev),
                "device": torch.cuda.get_device_name(dev)})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

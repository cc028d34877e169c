#!/usr/bin/env python3
"""Times the evolutionary search stage of sound matching (inverse-audio-synthesis_amd/evolve.py: evolve_search) on one GPU
and measures what it buys, and prints one JSON line.

    python scripts/bench_evolve.py [--steps time quality] [--timeout 600] [--generations 20] [--population 512]

* ``time``: seconds per generation of ``evolve_search`` at N = 16 and N = 128 targets, M = 512 candidates, k = 8 elites,
  4 s @ 44.1 kHz on a 128-row Voice with the mel loss (1024 / 512 / 128), against the sum of its own parts timed with
  events in the same process: one render, one value pass and one ias_l1_cdist (1 x 512 x K) times their count per
  generation, and one ias_topk_merge, ias_evolve_update and ias_evolve_sample.
* ``quality``: the 16 targets of section 4.6 (rendered from a batch outside the bank), bank(4,096) -> 4 nearest voices ->
  Adam 200 against bank(4,096) -> the same 4 voices as starts of ``evolve_search`` -> its 4 best elites -> Adam 200:
  median, best and worst final loss.
Each step runs in a child process of its own under ``--timeout`` seconds; a step that fails or runs out of time ends the run.
Nothing here asserts on a figure."""
import argparse
import json
import os
import subprocess
import sys
import time

import bench_common as bc


def _setup():
    import torch
    dev = torch.device("cuda:0")
    voice = bc.design_voice(dev)
    return dev, voice, bc.mel_matcher(voice)


def step_time(args):
    import torch
    from inverse_audio_synthesis_amd import _lib
    from inverse_audio_synthesis_amd.evolve import evolve_sample, evolve_search, evolve_update
    from inverse_audio_synthesis_amd.retrieval import EMPTY_INDEX, l1_cdist, topk_merge
    dev, voice, matcher = _setup()
    loss, B, M, k, P = matcher.loss, 128, args.population, 8, 78
    gen = torch.Generator().manual_seed(0)
    tv = loss.target(voice.render(torch.rand((B, P), generator=gen).to(dev)))
    K = tv[0].numel()
    out = {"M": M, "k": k, "K": K}

    params = torch.rand((B, P), generator=gen).to(dev)
    audio = voice.render(params, normalize=True)
    values = torch.empty((M,) + tuple(tv.shape[1:]), device=dev)
    ws = torch.empty(_lib.load().ias_l1_cdist_workspace_bytes(1, M, K), dtype=torch.uint8, device=dev)
    row = torch.empty((1, M), device=dev)
    parts = {"render_us": bc.event_ms(lambda: voice.render(params, normalize=True), args.reps)[0] * 1e3,
             "values_us": bc.event_ms(lambda: values[:B].copy_(loss.target(audio)), args.reps)[0] * 1e3,
             "cdist_1xM_us": bc.event_ms(lambda: l1_cdist(tv[:1].reshape(1, K), values.view(M, K), out=row, workspace=ws),
                                        args.reps)[0] * 1e3}
    free = torch.ones(P, dtype=torch.uint8, device=dev)
    for N in (16, 128):
        mean, sigma = torch.rand((N, P), device=dev), torch.full((N, P), 0.2, device=dev)
        pop = torch.empty((N, M, P), device=dev)
        block = torch.rand((N, M), device=dev)
        bd = torch.full((N, k), float("inf"), device=dev)
        bi = torch.full((N, k), EMPTY_INDEX, dtype=torch.int64, device=dev)
        ep, pp = torch.zeros((N, k, P), device=dev), torch.zeros((N, k, P), device=dev)
        evolve_sample(mean, sigma, free, 0, 0, pop)
        topk_merge(block, 0, bd, bi)
        pi = bi.clone()
        base = [0]

        def merge():
            base[0] += M
            topk_merge(block, base[0], bd, bi)
        p = {"sample_us": bc.event_ms(lambda: evolve_sample(mean, sigma, free, 0, 1, pop), 50)[0] * 1e3,
             "merge_us": bc.event_ms(merge, 50)[0] * 1e3}
        pi.copy_(bi)                                       # every elite is then found in prev: the gather reads pp
        p["update_us"] = bc.event_ms(lambda: evolve_update(pop, base[0] + M, bd, bi, pi, pp, ep, mean, sigma, free, 0.7,
                                                          0.005, 0.5), 50)[0] * 1e3
        nb = N * (M // B)
        p["parts_sum_ms"] = (nb * (parts["render_us"] + parts["values_us"]) + N * parts["cdist_1xM_us"] + p["sample_us"]
                             + p["merge_us"] + p["update_us"]) * 1e-3
        evolve_search(voice, loss, target_values=tv[:N], generations=1, population=M, elites=k)     # first use
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        evolve_search(voice, loss, target_values=tv[:N], generations=args.time_generations, population=M, elites=k)
        torch.cuda.synchronize()
        p["generation_ms"] = (time.perf_counter() - t0) * 1e3 / args.time_generations
        p["ratio"] = p["generation_ms"] / p["parts_sum_ms"]
        out[f"N{N}"] = {key: round(val, 3) for key, val in p.items()}
    out["parts"] = {key: round(val, 2) for key, val in parts.items()}
    return out


def step_quality(args):
    import torch
    from inverse_audio_synthesis_amd.evolve import evolve_search
    from inverse_audio_synthesis_amd.retrieval import SpectralBank
    dev, voice, matcher = _setup()
    tgt = bc.targets(voice)
    d, starts = bc.nearest_starts(SpectralBank(voice, matcher.loss, range(bc.BANK_BATCHES)), tgt)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    found = evolve_search(voice, matcher.loss, target_audio=tgt, generations=args.generations, population=args.population,
                          elites=8, init_params01=starts, seed=0)
    torch.cuda.synchronize()
    search_ms = (time.perf_counter() - t0) * 1e3
    _fits, q = bc.fit_starts(matcher, tgt, {"bank_adam": starts, "bank_evolve_adam": found.params01[:, :4].contiguous()},
                             pairs=[("bank_adam", "bank_evolve_adam")], every="final")
    return {"targets": bc.TARGETS, "steps": bc.FIT_STEPS, "starts": bc.STARTS, "generations": args.generations,
            "population": args.population,
            "bank_nearest_distance_median": round(float(d[:, 0].median()), 4),
            "evolve_distance_median": round(float(found.dist[:, 0].median()), 4),
            "evolve_history_median": [round(float(x), 4) for x in found.history.median(dim=1).values],
            "evolve_sigma_mean": round(float(found.sigma.mean()), 4), "search_ms": round(search_ms, 1),
            "bank_adam": q["bank_adam"], "bank_evolve_adam": q["bank_evolve_adam"],
            "evolve_better": q["bank_evolve_adam_wins"]}


STEPS = {"time": step_time, "quality": step_quality}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", nargs="+", choices=sorted(STEPS), default=["time", "quality"])
    ap.add_argument("--timeout", type=int, default=600, help="seconds each step may take")
    ap.add_argument("--reps", type=int, default=20, help="launches per timing of a part")
    ap.add_argument("--time-generations", type=int, default=3, help="generations timed per N")
    ap.add_argument("--generations", type=int, default=20, help="quality: generations of the search")
    ap.add_argument("--population", type=int, default=512, help="candidates per sound and generation")
    ap.add_argument("--child", choices=sorted(STEPS), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(STEPS[args.child](args)), flush=True)
        return
    out = {"bench": "evolve_search"}
    for name in args.steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name] + [a for a in sys.argv[1:]]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f"bench_evolve.py: step {name} did not finish within {args.timeout} s")
        if r.returncode != 0:
            sys.exit(f"bench_evolve.py: step {name} failed with status {r.returncode}")
        out[name] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

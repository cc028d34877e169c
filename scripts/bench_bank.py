#!/usr/bin/env python3
"""Times the spectral bank (inverse-audio-synthesis_amd/retrieval.py: SpectralBank) on one GPU and prints one JSON line.

    python scripts/bench_bank.py [--reps 20] [--quality] [--stream]

* ias_l1_cdist at (N, M, K) = (128, 4096, 44160) and (4, 4096, 44160) (K = 345 frames x 128 mels: a mel bank of 32 x 128
  voices of 4 s @ 44.1 kHz), against its compute floor (2 VALU instructions per (pair, k) on 256 CUs x 4 SIMD x 32 lanes
  at 2.4 GHz) and its memory floor (the bank read once at 8 TB/s), and torch.cdist(p=1) on the same operands;
* building that bank (32 renders and mel passes at B = 128, 4 s @ 44.1 kHz).
``--quality``: also fit 16 targets rendered from a batch outside the bank, 200 steps of mel-L1 from the centre and from
the 4 nearest bank voices, and report the final losses.
``--stream``: also time ``SpectralBank.search`` (chunks of 8 batches, k = 4) at N = 128 and N = 16 targets over banks of
4,096 / 65,536 / 1,048,576 voices (``--stream-sizes``, in batches of 128), each against the projection from the parts
timed above in the same run (the bank build per batch plus ias_l1_cdist per 4,096 voices), and ias_topk_merge alone at
(128, 1024, k = 4) with events over 50 launches.  ``--quality --stream``: the 16-target experiment from the 4 nearest
voices of each of those banks.  Kernel-level figures: run it under ``rocprofv3 --kernel-trace --stats``."""
import argparse
import json
import time

import bench_common as bc

VALU_PER_S = 256 * 4 * 32 * 2.4e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="launches per timing")
    ap.add_argument("--batches", type=int, default=32, help="voice batches of 128 in the bank")
    ap.add_argument("--quality", action="store_true", help="also compare centre and bank starts over 16 targets")
    ap.add_argument("--stream", action="store_true", help="also time the streamed search and ias_topk_merge")
    ap.add_argument("--stream-sizes", type=int, nargs="+", default=[32, 512, 8192],
                    help="--stream: bank sizes in batches of 128")
    args = ap.parse_args()

    import torch
    from inverse_audio_synthesis_amd import _lib
    from inverse_audio_synthesis_amd.retrieval import SpectralBank
    dev = torch.device("cuda:0")
    lib = _lib.load()
    B = 128
    voice = bc.design_voice(dev)
    matcher = bc.mel_matcher(voice)
    idx = range(args.batches)

    SpectralBank(voice, matcher.loss, [0])                     # first use: tables, allocations
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bank = SpectralBank(voice, matcher.loss, idx)
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    M, K = bank.values.shape[0], bank.values[0].numel()
    flat = bank.values.reshape(M, K)
    out = {"bench": "spectral_bank", "M": M, "K": K, "bank_bytes": M * K * 4, "build_ms": round(build_ms, 2)}

    gen = torch.Generator().manual_seed(0)
    for N in (128, 16, 4) if args.stream else (128, 4):
        q = matcher.loss.target(voice.render(torch.rand((B, 78), generator=gen).to(dev)))[:N].reshape(N, K).contiguous()
        ws = torch.empty(lib.ias_l1_cdist_workspace_bytes(N, M, K), dtype=torch.uint8, device=dev)
        dist = torch.empty((N, M), dtype=torch.float32, device=dev)

        def run():
            lib.ias_l1_cdist(_lib.ptr(q), _lib.ptr(flat), N, M, K, _lib.ptr(ws), _lib.ptr(dist), _lib.stream())
        ms = bc.event_ms(run, args.reps)[0]
        tc_ms = bc.event_ms(lambda: torch.cdist(q, flat, p=1.0), max(2, args.reps // 4))[0]
        ref = torch.cdist(q.double(), flat.double(), p=1.0) / K
        out[f"cdist_{N}"] = {
            "shape": [N, M, K], "ias_l1_cdist_us": round(ms * 1e3, 1),
            "compute_floor_us": round(2.0 * N * M * K / VALU_PER_S * 1e6, 1),
            "memory_floor_us": round((M + N) * K * 4 / 8e12 * 1e6, 1),
            "torch_cdist_p1_us": round(tc_ms * 1e3, 1),
            "max_rel_err_vs_fp64": float(((dist.double() - ref).abs() / ref.clamp_min(1e-30)).max())}
        del ws, dist, ref

    if args.stream:
        CH, KS = 8, 4
        dblock = torch.rand((128, CH * B), device=dev)
        bd = torch.full((128, KS), float("inf"), device=dev)
        bi = torch.full((128, KS), torch.iinfo(torch.int64).max, dtype=torch.int64, device=dev)
        base = [0]

        def merge():
            lib.ias_topk_merge(_lib.ptr(dblock), 128, CH * B, CH * B, base[0], KS, _lib.ptr(bd), _lib.ptr(bi),
                               _lib.stream())
            base[0] += CH * B
        out["topk_merge_128x1024_k4_us"] = round(bc.event_ms(merge, 50)[0] * 1e3, 2)
        qc = matcher.loss.target(voice.render(torch.rand((B, 78), generator=gen).to(dev))).reshape(B, K)
        wsc = torch.empty(lib.ias_l1_cdist_workspace_bytes(B, CH * B, K), dtype=torch.uint8, device=dev)

        def cdist_chunk():
            lib.ias_l1_cdist(_lib.ptr(qc), _lib.ptr(flat), B, CH * B, K, _lib.ptr(wsc), _lib.ptr(dblock), _lib.stream())
        out["cdist_128x1024_us"] = round(bc.event_ms(cdist_chunk, args.reps)[0] * 1e3, 1)
        t0 = time.perf_counter()
        from inverse_audio_synthesis_amd.voice import sample_params01
        for i in range(256):
            sample_params01(B, i)
        out["host_draw_us_per_batch"] = round((time.perf_counter() - t0) / 256 * 1e6, 1)
        del wsc
        tv = matcher.loss.target(voice.render(torch.rand((B, 78), generator=gen).to(dev)))
        SpectralBank.search(voice, matcher.loss, range(2 * CH), target_values=tv, k=KS, chunk_batches=CH)
        stream = []
        for nb in args.stream_sizes:
            for N in (128, 16):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                SpectralBank.search(voice, matcher.loss, range(nb), target_values=tv[:N], k=KS, chunk_batches=CH)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
                proj = nb / args.batches * build_ms + nb * B / M * out[f"cdist_{N}"]["ias_l1_cdist_us"] * 1e-3
                stream.append({"voices": nb * B, "N": N, "search_ms": round(ms, 1), "projected_ms": round(proj, 1),
                               "ratio": round(ms / proj, 3)})
        out["stream"] = stream

    if args.quality and args.stream:
        tgt = bc.targets(voice)
        qs = []
        for nb in args.stream_sizes:
            d, nbi, starts = SpectralBank.search(voice, matcher.loss, range(nb), target_audio=tgt, k=4, chunk_batches=8)
            fits, q = bc.fit_starts(matcher, tgt, {"bank": starts}, every="final")
            qs.append({"voices": nb * B, "nearest_distance_median": round(float(d[:, 0].median()), 4),
                       "final": q["bank"]["final"], "start": fits["bank"].start.tolist(),
                       "final_median": q["bank"]["median"], "final_best": q["bank"]["best"],
                       "final_worst": q["bank"]["worst"]})
        out["quality_stream"] = qs

    if args.quality:
        tgt = bc.targets(voice)
        d, starts = bc.nearest_starts(bank, tgt)
        fits, q = bc.fit_starts(matcher, tgt, {"center": None, "bank": starts}, pairs=[("center", "bank")])
        out["quality"] = {
            "targets": bc.TARGETS, "steps": bc.FIT_STEPS, "starts": bc.STARTS,
            "center_initial": bc.rounded(fits["center"].initial_loss),
            "center_final": q["center"]["all"],
            "bank_nearest_distance": bc.rounded(d[:, 0]),
            "bank_final": q["bank"]["all"],
            "bank_start": fits["bank"].start.tolist(),
            "center_final_median": q["center"]["median"],
            "bank_final_median": q["bank"]["median"],
            "bank_better": q["bank_wins"]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the band-limited resampler (inverse-audio-synthesis_amd/resample.py: ias_resample) on one GPU and prints one JSON
line.

    python scripts/bench_resample.py [--reps 50]

At B = 128 clips of 4 s for 48 kHz -> 44.1 kHz, 96 kHz -> 44.1 kHz and 44.1 kHz -> 48 kHz: ias_resample timed with device
events after a warm-up, beside its compute floor (B T_out K FMAs at 256 CUs x 4 SIMD x 32 lanes x 2.4 GHz, the fp32
vector peak) and its memory floor (input read and output written once at 8 TB/s); as a yardstick the same algorithm as
torch ops on the GPU (the F.pad + F.conv1d(stride=o) form torchaudio uses, with the same table), and the max abs
difference between the two.  Kernel-level figures: run it under ``rocprofv3 --kernel-trace --stats``."""
import argparse
import json

import bench_common as bc

FMA_PER_S = 256 * 4 * 32 * 2.4e9
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50, help="launches per timing")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--seconds", type=float, default=4.0)
    args = ap.parse_args()

    import torch
    import torch.nn.functional as F
    from inverse_audio_synthesis_amd import _lib
    from inverse_audio_synthesis_amd.resample import output_length, resample_kernel
    dev = torch.device("cuda:0")
    lib = _lib.load()
    B = args.batch
    out = {"bench": "resample", "B": B, "seconds": args.seconds}
    gen = torch.Generator().manual_seed(0)
    for orig, new in ((48000, 44100), (96000, 44100), (44100, 48000)):
        (o, n, width, K), taps = resample_kernel(orig, new)
        T = int(round(args.seconds * orig))
        T_out = output_length(T, o, n)
        x = (torch.rand((B, T), generator=gen) * 2 - 1).to(dev)
        taps_d = taps.to(dev)
        y = torch.empty((B, T_out), dtype=torch.float32, device=dev)

        def run():
            lib.ias_resample(_lib.ptr(x), _lib.ptr(taps_d), _lib.ptr(y), B, T, o, n, width, K, _lib.stream())
        _lib.check(lib.ias_resample(_lib.ptr(x), _lib.ptr(taps_d), _lib.ptr(y), B, T, o, n, width, K, _lib.stream()),
                   "ias_resample")
        ms = bc.event_ms(run, args.reps)[0]
        w = taps_d[:, None, :]

        def conv():
            r = F.conv1d(F.pad(x[:, None], (width, width + o)), w, stride=o)
            return r.transpose(1, 2).reshape(B, -1)[:, :T_out]
        with torch.no_grad():
            conv_ms = bc.event_ms(conv, max(2, args.reps // 5))[0]
            diff = float((conv() - y).abs().max())
        out[f"{orig}_{new}"] = {
            "o_n_K": [o, n, K], "T_in": T, "T_out": T_out, "ias_resample_us": round(ms * 1e3, 1),
            "compute_floor_us": round(B * T_out * K / FMA_PER_S * 1e6, 1),
            "memory_floor_us": round(B * (T + T_out) * 4 / HBM_BYTES_PER_S * 1e6, 1),
            "torch_conv1d_us": round(conv_ms * 1e3, 1), "max_abs_diff_vs_conv1d": diff}
        del x, y, taps_d
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

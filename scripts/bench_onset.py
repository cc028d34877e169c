#!/usr/bin/env python3
"""Times the onset stage (inverse-audio-synthesis_amd/onset.py) on one GPU and prints one JSON line.

    python scripts/bench_onset.py [--reps 200] [--passes 3] [--seconds 600]

Two shapes: 128 sounds of 4 s @ 44.1 kHz and one recording of ``--seconds`` (600 s) @ 44.1 kHz, ``detect_onsets``' defaults
(n_fft 1024, hop 256, 128 mels, lag 2).  Per shape, isolated and by device events over ``--reps`` launches, ``--passes``
times (min / median / max reported): the mel launch that feeds the stage, ias_onset_flux, ias_onset_pick, and
ias_segment_gather of as many 4 s notes as the shape holds, each starting at another 16-byte phase.  Next to them the time
the [B, F, M] mel tensor takes through HBM at 8 TB/s once (the flux kernel's compulsory read) and the gather's read plus
write.  If the STFT entry refuses the long row, the length is halved until it runs and the length that ran is reported.
The audio is white noise: none of the four kernels' times depends on the values, and noise gives the picker candidates.
Kernel-level figures: run it under ``rocprofv3 --kernel-trace --stats``."""
import argparse
import json

import bench_common as bc

HBM_BYTES_PER_S = 8e12


def _events_us(fn, reps, passes):
    return bc.spread(bc.event_ms(fn, reps, passes), 1e3)


def _shape(B, L, rate, reps, passes):
    import torch
    from inverse_audio_synthesis_amd import _lib
    from inverse_audio_synthesis_amd.onset import _mel_plan, onset_flux, onset_pick
    dev = torch.device("cuda:0")
    lib = _lib.load()
    audio = 0.1 * torch.randn((B, L), generator=torch.Generator().manual_seed(0)).to(dev)
    plan = _mel_plan(rate, 1024, 256, 128, dev)
    mel = plan.frames_major(audio)
    _B, F, M = mel.shape
    flux = onset_flux(mel)
    frames, _strength, count = onset_pick(flux)
    T = 4 * rate
    S = max(1, (B * L) // T)
    per_row = max(1, L // T)
    s = torch.arange(S)
    row = (s // per_row).to(torch.int32).to(dev)
    start = ((s % per_row) * T + s % 4).clamp_max(max(L - T, 0)).to(torch.int32).to(dev)
    length = torch.full((S,), min(T, L), dtype=torch.int32, device=dev)
    faded = (s % 2).to(torch.uint8).to(dev)
    notes = torch.empty((S, T), dtype=torch.float32, device=dev)
    fade = 220

    def gather():
        lib.ias_segment_gather(_lib.ptr(audio), B, L, _lib.ptr(row), _lib.ptr(start), _lib.ptr(length), _lib.ptr(faded), S, T,
                               fade, 1.0 / fade, _lib.ptr(notes), _lib.stream())
    mel_bytes = 4.0 * B * F * M
    return {"shape": [B, L], "frames": F, "mels": M, "onsets_max": int(count.max()),
            "mel_launch_us": _events_us(lambda: plan.frames_major(audio), reps, passes),
            "ias_onset_flux_us": _events_us(lambda: onset_flux(mel), reps, passes),
            "ias_onset_pick_us": _events_us(lambda: onset_pick(flux), reps, passes),
            "ias_segment_gather_us": _events_us(gather, reps, passes),
            "mel_tensor_bytes": mel_bytes, "mel_tensor_hbm_us": round(mel_bytes / HBM_BYTES_PER_S * 1e6, 2),
            "gather_notes": S, "gather_bytes": 8.0 * S * T,
            "gather_hbm_us": round(8.0 * S * T / HBM_BYTES_PER_S * 1e6, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="launches per timing window")
    ap.add_argument("--passes", type=int, default=3, help="timing windows per figure")
    ap.add_argument("--seconds", type=int, default=600, help="length of the long recording")
    args = ap.parse_args()
    import torch
    rate = 44100
    out = {"bench": "onset", "device": torch.cuda.get_device_name(0), "reps": args.reps, "passes": args.passes,
           "batch": _shape(128, 4 * rate, rate, args.reps, args.passes)}
    seconds = args.seconds
    while True:
        try:
            out["long"] = _shape(1, seconds * rate, rate, max(1, args.reps // 4), args.passes)
            break
        except RuntimeError as e:
            if "IAS_ERR" not in str(e):                  # only the library's own refusals are answered with a shorter row
                raise
            out.setdefault("long_refused", []).append({"seconds": seconds, "error": str(e)})
            seconds //= 2
            if seconds < 4:
                break
    out["long_seconds"] = seconds
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the match report (inverse-audio-synthesis_amd/report.py) on one GPU and prints one JSON line.

    python scripts/bench_report.py [--reps 200] [--passes 3] [--no-headline]

Isolated and by device events over ``--reps`` calls, ``--passes`` times (min / median / max reported):
* ias_spectral_report (both launches) at (B, F, K) = (128, 690, 513), no table, power 1: the linear plan of 128 sounds of
  4 s @ 44.1 kHz, 2 x 181 MB;
* ias_spectral_report at (128, 345, 128) with 13 cepstral coefficients, power 2: the mel plan, 2 x 22.6 MB;
  each against the time its two tensors take through HBM at 8 TB/s once;
* the whole ``Reporter`` call on 128 sounds of 4 s @ 44.1 kHz with a cached target (two STFTs, two reports, YIN, the envelope
  frames and the torch glue), by device events as well.
Unless ``--no-headline``: one matcher iteration (``scripts/bench_match.py``) on the same machine in the same run, in a
process of its own before this one opens the GPU, for scale.
Kernel-level figures: run it under ``rocprofv3 --kernel-trace --stats``."""
import argparse
import json
import os

import bench_common as bc
from bench_common import ROOT

HBM_BYTES_PER_S = 8e12
SHAPES = {"linear": (128, 690, 513, 0, 1), "mel": (128, 345, 128, 13, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="calls per timing window")
    ap.add_argument("--passes", type=int, default=3, help="timing windows per figure")
    ap.add_argument("--no-headline", action="store_true", help="skip the matcher iteration")
    args = ap.parse_args()

    out = {"bench": "report"}
    if not args.no_headline:
        out["matcher_iter_ms"] = bc.json_line([os.path.join(ROOT, "scripts", "bench_match.py")])["iter_ms"]

    import torch
    from inverse_audio_synthesis_amd import _lib
    from inverse_audio_synthesis_amd.report import Reporter, dct_table
    dev = torch.device("cuda:0")
    lib = _lib.load()
    out.update({"device": torch.cuda.get_device_name(dev), "reps": args.reps, "passes": args.passes})
    gen = torch.Generator().manual_seed(0)
    for name, (B, F, K, C, power) in SHAPES.items():
        t = (torch.randn((B, F, K), generator=gen) ** 2).to(dev)
        v = (t * torch.exp(0.5 * torch.randn((B, F, K), generator=gen).to(dev))).contiguous()
        fl = (1e-4 * t.reshape(B, -1).max(dim=1).values).contiguous()
        dct = dct_table(K, C).to(dev) if C else None
        partials = torch.empty((B, lib.ias_spectral_report_partials_count(F), 6), dtype=torch.float64, device=dev)
        res = torch.empty((B, 5), dtype=torch.float64, device=dev)

        def call():
            lib.ias_spectral_report(_lib.ptr(v), _lib.ptr(t), _lib.ptr(fl), _lib.ptr(dct), B, F, K, C, power,
                                    _lib.ptr(partials), _lib.ptr(res), _lib.stream())
        nbytes = 2.0 * 4.0 * B * F * K
        out[name] = {"shape": [B, F, K], "n_coef": C, "power": power, "bytes": nbytes,
                     "hbm_us": round(nbytes / HBM_BYTES_PER_S * 1e6, 2),
                     "ias_spectral_report_us": bc.spread(bc.event_ms(call, args.reps, args.passes), 1e3)}
        assert bool(torch.isfinite(res).all())
        del t, v

    voice = bc.design_voice(dev)
    rate = voice.synthconfig.sample_rate
    draws = torch.rand((2, 128, 78), generator=torch.Generator().manual_seed(1)).to(dev)
    target_audio, audio = voice.render(draws[0]).clone(), voice.render(draws[1]).clone()
    reporter = Reporter(rate, mel_kwargs=bc.MEL)
    cache = reporter.target(target_audio)
    whole = bc.event_ms(lambda: reporter(audio, target=cache), max(1, args.reps // 10), args.passes)
    rep = reporter(audio, target=cache)
    out["reporter"] = {"shape": list(audio.shape), "rate": rate, "call_ms": bc.spread(whole, digits=3),
                       "median_lsd_db": round(float(rep.lsd_db.median()), 3),
                       "median_mcd_db": round(float(rep.mcd_db.median()), 3), "voiced": int(rep.voiced.sum())}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

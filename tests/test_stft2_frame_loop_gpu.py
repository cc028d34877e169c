"""stft2_kernel's frame loop: the same bits as the kernel before the loop was restructured, and the oracle's values.

The n_fft 1024 / 2048 forward kernel (csrc/spectral_kernels.hip: stft2_kernel) deals the frames of the flat [B * F] list to
its waves and prefetches a wave's next frame while the current one is transformed.  At n_fft 1024 the loop now keeps ONE
set of frame registers (the next frame is loaded into the set pass 1 has just consumed), the unit twiddles of passes 1
and 2 are constants instead of LDS reads, and the workgroup stages its tables with all loads in flight at once, behind
the first frame's loads.  No arithmetic moved, so every output bit is what the kernel with two register sets gave:
tests/golden/stft2_frame_loop_parent.npz holds a fixed subset of that kernel's outputs for the inputs below
(scripts/diag/make_stft2_frame_loop_golden.py wrote it from the parent commit's library), and the tests ask for byte
equality with it, and for the oracle's values at the tolerances of tests/test_spectral_gpu.py.

The inputs put the loop's structure on the path.  The launcher caps the grid at 2 workgroups of 8 waves per CU, so with
B = CUs / 4 rows of T = 65573 samples at hop 512 (129 frames per row; 8256 frames on 4096 waves with 256 CUs) a few waves
run the loop three times and the rest twice: the prefetch into the consumed set, the guard of the last iteration and the
row peak that travels with the prefetch are all exercised, across row boundaries.  B = 1 with three frames runs the
loop once or not at all.  T is odd, so rows start at addresses that are not 16-byte aligned and the first and last two
frames of a row take the reflect loads; hop 128 gives frames that start at every alignment.  Every third row clips
(peak 1.53) and is normalised through rowpeak where the case passes one.  Cases: 128 mels, 80 mels (30 Hz .. 8 kHz: the
default range at 80 bands has three filters over a bin, which the segment tables refuse, and would run another kernel;
this one also has its first segment at s0 = 0 where the 128-band one has s0 = 1), linear bins at n_fft 1024, n_fft 2048
(two sub-transforms per frame), loss modes 0, 1 and 2.  The log-magnitude sum of mode 2 runs on the 80-band filterbank only:
the 128-band one has an empty filter, whose value and target are both 0 and whose log difference is not a number, before
this change and after.

The golden file was written on a 256-CU part.  The spectrogram of a row does not depend on the launch geometry, the
per-workgroup loss partials do: on a part with another CU count the batch is sized from that count, the stored rows
that exist are still compared and the partials are only checked against the oracle."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle import spectral_oracle as spo

pytestmark = pytest.mark.gpu
GOLDEN_FILE = "stft2_frame_loop_parent.npz"
VALUES_TOL = 1e-4       # tests/test_spectral_gpu.py: spectrogram values, of the spectrogram's maximum
LOSS_RTOL = 1e-3        # tests/test_spectral_gpu.py: spectral losses, relative
T_BIG = 65573
MRSTFT_EPS = 1e-8

# name -> plan arguments, batch (rows per 256 CUs, or a fixed B), T, rowpeak, loss modes
CASES = {
    "mel128": dict(n_fft=1024, hop=512, mel=dict(n_mels=128), per256=64, T=T_BIG, rowpeak=True, losses=(1,)),
    "mel128-norowpeak": dict(n_fft=1024, hop=512, mel=dict(n_mels=128), per256=64, T=T_BIG, rowpeak=False, losses=(1,)),
    "mel80": dict(n_fft=1024, hop=512, mel=dict(n_mels=80, f_min=30.0, f_max=8000.0), per256=64, T=T_BIG, rowpeak=True,
                  losses=(1, 2)),
    "mel128-hop128": dict(n_fft=1024, hop=128, mel=dict(n_mels=128), per256=16, T=T_BIG, rowpeak=True, losses=(1,)),
    "lin1024": dict(n_fft=1024, hop=512, mel=None, per256=64, T=T_BIG, rowpeak=True, losses=(1, 2)),
    "lin1024-hop128": dict(n_fft=1024, hop=128, mel=None, per256=16, T=T_BIG, rowpeak=False, losses=(2,)),
    "lin2048": dict(n_fft=2048, hop=512, mel=None, per256=64, T=T_BIG, rowpeak=True, losses=(1, 2)),
    "lin2048-hop128": dict(n_fft=2048, hop=128, mel=None, per256=16, T=T_BIG, rowpeak=False, losses=(1,)),
    "mel128-3frames": dict(n_fft=1024, hop=512, mel=dict(n_mels=128), B=1, T=1024, rowpeak=True, losses=(1,)),
    "mel80-3frames": dict(n_fft=1024, hop=512, mel=dict(n_mels=80, f_min=30.0, f_max=8000.0), B=1, T=1024, rowpeak=False,
                          losses=(2,)),
    "lin1024-3frames": dict(n_fft=1024, hop=512, mel=None, B=1, T=1024, rowpeak=False, losses=(1, 2)),
    "lin2048-3frames": dict(n_fft=2048, hop=512, mel=None, B=1, T=1025, rowpeak=True, losses=(1, 2)),
}


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def batch_of(case, ncu):
    return case["B"] if "B" in case else max(2, (case["per256"] * ncu) // 256)


@functools.lru_cache(maxsize=None)
def rows(B, T, seed):
    """[B, T] fp32 on the host: seeded noise plus three sines per row, peak 0.9; every third row (1, 4, ...) times 1.7.
    Row b depends on (seed, b, T) only, not on B."""
    t = torch.arange(T, dtype=torch.float32) / 44100.0
    out = torch.empty(B, T, dtype=torch.float32)
    for b in range(B):
        g = torch.Generator().manual_seed(1000 * seed + b)
        x = 0.1 * torch.randn(T, generator=g, dtype=torch.float32)
        for f, amp in ((110.0 * (b % 17 + 1), 0.3), (1760.0 + 37.0 * b, 0.2), (9000.0 - 50.0 * b, 0.1)):
            x += amp * torch.sin(2.0 * math.pi * f * t + 0.5 * b)
        x = 0.9 * x / x.abs().amax()
        out[b] = 1.7 * x if b % 3 == 1 else x
    return out


def subset(B, F, seed):
    """The (row, frame) pairs the golden file keeps: first and last row and two seeded ones, of each the first two and
    last two frames and four seeded ones."""
    g = torch.Generator().manual_seed(seed)
    rs = sorted({0, B - 1} | {int(v) for v in torch.randint(0, B, (2,), generator=g)})
    fs = sorted({0, 1 % F, max(F - 2, 0), F - 1} | {int(v) for v in torch.randint(0, F, (4,), generator=g)})
    return [(r, f) for r in rs for f in fs]


def run_case(name, dev, ncu):
    """The kernel's outputs for one case -> dict of host tensors: 'values' [B, F, n_out] for both value modes in use,
    'partials<mode>' [workgroups, 3] fp64, and the inputs the oracle needs."""
    from inverse_audio_synthesis_amd import _lib
    from inverse_audio_synthesis_amd.spectral import STFTPlan, VALUE_MAG, VALUE_MAG_CLAMPED, VALUE_POWER
    case = CASES[name]
    B, T = batch_of(case, ncu), case["T"]
    mel = case["mel"]
    plan = STFTPlan(case["n_fft"], None, case["hop"], sample_rate=44100, **(mel or {})).to(dev)
    assert mel is None or plan.segtab is not None, "the filterbank must run the segment-table kernel"
    a_host, t_host = rows(B, T, 1), rows(B, T, 2)
    a, tgt = a_host.to(dev), t_host.to(dev)
    rowpeak = a.abs().amax(dim=1).contiguous() if case["rowpeak"] else None
    if rowpeak is not None and B > 1:
        assert rowpeak[1].item() > 1.0 and rowpeak[0].item() <= 1.0
    vm0 = VALUE_POWER if mel is not None else VALUE_MAG
    res = {"B": B, "F": plan.num_frames(T), "audio": a_host, "target": t_host, "vm0": vm0,
           "values": plan.values(a, vm0, rowpeak=rowpeak).cpu()}
    lib = _lib.load()
    n = lib.ias_stft_partials_count(B, T, plan.n_fft, plan.hop_length,
                                    (0 if plan.mtables is None else 1) | (0 if mel is None else 2) |
                                    (0 if plan.segtab is None else 4))
    for mode in case["losses"]:
        vm, eps = (VALUE_MAG_CLAMPED, MRSTFT_EPS) if mode == 2 else (vm0, 0.0)
        tv = plan.values(tgt, vm, eps=eps)
        partials = torch.full((n, 3), float("nan"), dtype=torch.float64, device=dev)
        plan._call(a, None, tv, partials, vm, mode, eps, rowpeak)
        res[f"partials{mode}"] = partials.cpu()
    torch.cuda.synchronize()
    return res


def golden_entries(name, res):
    """What the golden file keeps of run_case's result."""
    case = CASES[name]
    sub = subset(res["B"], res["F"], 77)
    out = {f"{name}/values": np.stack([res["values"][r, f].numpy() for r, f in sub]),
           f"{name}/B": np.int64(res["B"])}
    for mode in case["losses"]:
        out[f"{name}/partials{mode}"] = res[f"partials{mode}"].numpy()
    return out


@functools.lru_cache(maxsize=None)
def _golden(golden_dir):
    with np.load(os.path.join(golden_dir, GOLDEN_FILE)) as z:
        return {k: z[k] for k in z.files}


def _oracle_values(case, x, power, clamp_eps=None):
    """[B, F, n_out] of the oracle for host audio x (already normalised): |X|^power per bin, or with clamp_eps the
    clamped magnitude sqrt(max(|X|^2, eps)); then the filterbank, if the case has one."""
    if clamp_eps is not None:
        spec = spo.spectrogram(x, case["n_fft"], None, case["hop"], 2.0).clamp_min(clamp_eps).sqrt()
    else:
        spec = spo.spectrogram(x, case["n_fft"], None, case["hop"], power)
    spec = spec.transpose(1, 2)
    if case["mel"] is not None:
        m = case["mel"]
        fb = spo.melscale_fbanks(case["n_fft"] // 2 + 1, m.get("f_min", 0.0), m.get("f_max", 22050.0), m["n_mels"], 44100)
        spec = torch.matmul(spec, fb)
    return spec.contiguous()


@pytest.mark.parametrize("name", list(CASES))
def test_frame_loop_bits_and_oracle(lib, dev, golden_dir, name):
    from inverse_audio_synthesis_amd.spectral import VALUE_POWER
    case = CASES[name]
    ncu = cu_count()
    res = run_case(name, dev, ncu)
    B, F = res["B"], res["F"]
    values = res["values"]
    assert torch.isfinite(values).all()

    # the oracle: values of every row, then the loss sums
    x = res["audio"]
    if case["rowpeak"]:
        peak = x.abs().amax(dim=1, keepdim=True)
        x = torch.where(peak > 1.0, x / peak, x)
    power = 2.0 if res["vm0"] == VALUE_POWER else 1.0
    ref = _oracle_values(case, x, power)
    assert values.shape == ref.shape
    err, scale = (values - ref).abs().max().item(), ref.abs().max().item()
    print(f"{name}: B {B} F {F} values max err {err:.3e} of max {scale:.3e} = {err / scale:.2e}")
    assert err <= VALUES_TOL * scale
    for mode in case["losses"]:
        got = res[f"partials{mode}"].sum(dim=0)
        assert torch.isfinite(got).all()
        if mode == 1:
            want = [(ref - _oracle_values(case, res["target"], power)).abs().double().sum().item()]
        else:
            v, t = _oracle_values(case, x, 1.0, MRSTFT_EPS).double(), _oracle_values(case, res["target"], 1.0, MRSTFT_EPS).double()
            want = [((t - v) ** 2).sum().item(), (t * t).sum().item(), (v.log() - t.log()).abs().sum().item()]
        for i, w in enumerate(want):
            rel = abs(got[i].item() - w) / abs(w)
            print(f"{name}: loss mode {mode} sum {i}: {got[i].item():.9e} oracle {w:.9e} rel {rel:.2e}")
            assert rel <= LOSS_RTOL

    # the kernel before the change, byte for byte
    gold = _golden(golden_dir)
    gB = int(gold[f"{name}/B"])
    sub = subset(gB, F, 77)
    gv = gold[f"{name}/values"]
    assert gv.shape == (len(sub), values.shape[2])
    compared = 0
    for i, (r, f) in enumerate(sub):
        if r < B:
            assert values[r, f].numpy().tobytes() == gv[i].tobytes(), (name, r, f)
            compared += 1
    assert compared >= len(sub) // 4
    if gB == B:
        for mode in case["losses"]:
            assert res[f"partials{mode}"].numpy().tobytes() == gold[f"{name}/partials{mode}"].tobytes(), (name, mode)

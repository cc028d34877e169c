"""The frame-gradient kernels of the spectral losses: the same bits as before they moved into a file of their own.

csrc/stft_frame_grad_kernels.hip holds the table-driven backward of the linear-bin and mel losses
(stft_grad_wave_kernel, stft_grad2k_kernel, stft_grad512_kernel).  When they were split off csrc/spectral_kernels.hip
their loss maths became one copy (BinLoss), the 2048- and 512-point kernels took shared bin-pair helpers and the host
dispatch became plain C++; no arithmetic moved.  tests/golden/stft_frame_grad_parent.npz holds d loss / d audio of the
cases below from the library of the commit before the split (scripts/diag/make_stft_frame_grad_golden.py wrote it), and
the test asks for byte equality with it.  tests/test_stft2_frame_loop_gpu.py is the forward's twin.

Shapes: B = 3 rows of spectral_inputs.tones (row 1 is quiet: clamped bins), T = 10 hop with hop = n_fft / 4, so 11
frames per row and, at the minimum chunk length of 3 frames, chunks of 3, 3, 3 and 2 frames: spans meet inside a row,
stft_grad512_kernel (two frames per trip) sees an odd chunk, the first and last frames take the reflect loads.  Where the
loss has per-row cotangents they are (1, 0.625, 0): the coefficient pairs of the MR-STFT rows differ, and the last row's
gradient must be exactly 0.  Kernels reached:
  l1-*            stft_grad512_kernel / stft_grad_wave_kernel<10, false, true> / stft_grad2k_kernel<8, true>, power 1 and 2
  mel-*           stft_grad_wave_kernel<10 | 9, true, true>; the odd hop: <9, true, false> and the overlap-add kernel
  mrstft*         the default three resolutions at T = 5120, batch loss and per_item (CROW: a pair per row)
  mrstft-oddhop*  no span plan: ias_stft_loss_backward(_mrstft_rows), the frames forms <9 | 10, false, false> and
                  stft_grad2k_kernel<8, false>
  *-hop510        n_fft 2048 with a hop that is no multiple of 4: spans of stft_grad_wave_kernel<11, false, true>

The chunk plan (frames per chunk, chunks per row, span length) enters the order of the overlap-add sums.  At these sizes
it does not depend on the CU count; the test still asks ias_stft_grad_span_plan and skips the byte comparison, with a
message, on a part where the plan is not the stored one."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from spectral_inputs import tones

pytestmark = pytest.mark.gpu
GOLDEN_FILE = "stft_frame_grad_parent.npz"
B = 3
RATE = 44100
ROW_WEIGHTS = (1.0, 0.625, 0.0)
DEFAULTS = dict(fft_sizes=(1024, 2048, 512), hop_sizes=(120, 240, 50), win_lengths=(600, 1200, 240))
ODDHOP = dict(fft_sizes=(512, 1024, 2048), hop_sizes=(125, 255, 511), win_lengths=(512, 1024, 2048))
HOP510 = dict(fft_sizes=(2048,), hop_sizes=(510,), win_lengths=(2048,))

# name -> kind, the loss's arguments, T, per-row cotangents (rows) or the batch loss
CASES = {}
for _n in (512, 1024, 2048):
    for _p in (1.0, 2.0):
        CASES[f"l1-{_n}-p{int(_p)}"] = dict(kind="l1", n_fft=_n, hop=_n // 4, power=_p, T=10 * (_n // 4), rows=True)
CASES.update({
    "l1-1024-batch": dict(kind="l1", n_fft=1024, hop=256, power=1.0, T=2560, rows=False),
    "mel-1024": dict(kind="mel", n_fft=1024, hop=256, n_mels=128, T=2560, rows=True),
    "mel-512": dict(kind="mel", n_fft=512, hop=128, n_mels=64, T=1280, rows=False),
    "mel-512-oddhop": dict(kind="mel", n_fft=512, hop=77, n_mels=64, T=1280, rows=True),
    "mrstft": dict(kind="mrstft", res=DEFAULTS, T=5120, rows=False),
    "mrstft-rows": dict(kind="mrstft", res=DEFAULTS, T=5120, rows=True),
    "mrstft-oddhop": dict(kind="mrstft", res=ODDHOP, T=5120, rows=False),
    "mrstft-oddhop-rows": dict(kind="mrstft", res=ODDHOP, T=5120, rows=True),
    "l1-2048-hop510": dict(kind="l1", n_fft=2048, hop=510, power=1.0, T=5100, rows=True),
    "mrstft-2048-hop510-rows": dict(kind="mrstft", res=HOP510, T=5100, rows=True),
})


def _module(case, dev):
    from inverse_audio_synthesis_amd.spectral import MelSpectrogramL1, MultiResolutionSTFTLoss, STFTL1
    if case["kind"] == "l1":
        return STFTL1(n_fft=case["n_fft"], hop_length=case["hop"], power=case["power"]).to(dev)
    if case["kind"] == "mel":
        return MelSpectrogramL1(sample_rate=RATE, n_fft=case["n_fft"], hop_length=case["hop"], n_mels=case["n_mels"]).to(dev)
    return MultiResolutionSTFTLoss(**case["res"]).to(dev)


def _plans_of(module, case):
    if case["kind"] == "l1":
        return [module.plan]
    if case["kind"] == "mel":
        return [module.mel.plan]
    return list(module.plans)


def span_plans(lib, module, case):
    """[resolutions, 4] int32: status of ias_stft_grad_span_plan and its (frames per chunk, chunks per row, span length)."""
    out = []
    for plan in _plans_of(module, case):
        hp = (ctypes.c_int * 3)()
        st = lib.ias_stft_grad_span_plan(B, case["T"], plan.n_fft, plan.hop_length, plan._mel_args()[4], plan.n_out, hp)
        out.append([st, hp[0], hp[1], hp[2]] if st == 0 else [st, 0, 0, 0])
    return np.asarray(out, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def inputs(T, seed):
    """(audio, target): fp32 [B, T] on the host."""
    return tones(B, T, RATE, seed), tones(B, T, RATE, seed + 1)


def run_case(name, lib, dev):
    """-> (d loss / d audio [B, T] on the host, the span plans of the case's resolutions)."""
    case = CASES[name]
    module = _module(case, dev)
    a_host, t_host = inputs(case["T"], 4000 + 2 * list(CASES).index(name))
    a = a_host.to(dev).requires_grad_(True)
    t = t_host.to(dev)
    if case["rows"]:
        w = torch.tensor(ROW_WEIGHTS, dtype=torch.float32, device=dev)
        loss = (module.per_item(a, t) * w).sum()
    else:
        loss = module(a, t)
    loss.backward()
    torch.cuda.synchronize()
    return a.grad.cpu(), span_plans(lib, module, case)


@functools.lru_cache(maxsize=None)
def _golden(golden_dir):
    with np.load(os.path.join(golden_dir, GOLDEN_FILE)) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(CASES))
def test_frame_grad_bits(lib, dev, golden_dir, name):
    case = CASES[name]
    grad, plans = run_case(name, lib, dev)
    assert grad.shape == (B, case["T"]) and torch.isfinite(grad).all()
    assert torch.count_nonzero(grad[0]).item() > 0 and torch.count_nonzero(grad[1]).item() > 0
    if case["rows"]:
        assert torch.count_nonzero(grad[2]).item() == 0, "a row with cotangent 0 gets exactly 0"
    spans = "oddhop" not in name
    assert bool((plans[:, 0] == 0).all()) == spans, plans
    gold = _golden(golden_dir)
    if not np.array_equal(plans, gold[f"{name}/plans"]):
        pytest.skip(f"chunk plans {plans.tolist()} are not the stored ones {gold[f'{name}/plans'].tolist()} "
                    f"(written on a part with {int(gold['ncu'])} CUs): the order of the overlap-add sums differs")
    want = gold[f"{name}/grad"]
    got = grad.numpy()
    assert got.shape == want.shape
    diff = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert diff.size == 0, f"{name}: {diff.size} of {got.size} words differ, first at {np.unravel_index(diff[0], got.shape)}"

"""The model the BatchNorm1d row-group kernels are tested against (tests/bn1d_model.py), checked on the CPU: its fp64 mode
is G sequential nn.BatchNorm1d calls, and its fp32 kernel-order mode holds half of every bound of
test_bn1d_groups_gpu.py on every case of the table -- an fp32 implementation of this design can meet them."""
import pytest
import torch
import torch.nn.functional as F_

import bn1d_model as bm


def _close(got, want, name):
    scale = max(1.0, want.abs().max().item())
    assert (got - want).abs().max().item() <= 1e-12 * scale, name


def _torch_reference(inp, G, n, F, relu, affine=True, track=True):
    """G calls of nn.BatchNorm1d(F).double().train() (+ relu) on z + lin_bias, in group order; autograd gradients of
    sum(y * dy)."""
    bn = torch.nn.BatchNorm1d(F, eps=bm.EPS, momentum=bm.MOMENTUM, affine=affine, track_running_stats=track).double().train()
    with torch.no_grad():
        if affine:
            bn.weight.copy_(inp.weight.double()); bn.bias.copy_(inp.bias.double())
        if track:
            bn.running_mean.copy_(inp.running_mean.double()); bn.running_var.copy_(inp.running_var.double())
            bn.num_batches_tracked.fill_(inp.nbt)
    z = inp.z.double().requires_grad_(True)
    lb = None if inp.lin_bias is None else inp.lin_bias.double().requires_grad_(True)
    x = z if lb is None else z + lb
    ys = []
    for g in range(G):
        v = bn(x[g * n:(g + 1) * n])
        ys.append(F_.relu(v) if relu else v)
    y = torch.cat(ys, 0)
    wrt = [z] + ([lb] if lb is not None else []) + (list(bn.parameters()) if affine else [])
    grads = list(torch.autograd.grad((y * inp.dy.double()).sum(), wrt))
    gz = grads.pop(0)
    glb = grads.pop(0) if lb is not None else None
    gw, gb = (grads if affine else (None, None))
    return y.detach(), bn, gz, glb, gw, gb


@pytest.mark.parametrize("case", bm.CASES, ids=bm.CASE_IDS)
def test_fp64_model_is_sequential_torch_batchnorm(case):
    G, n, F, relu, lb = case
    inp = bm.make_inputs(G, n, F, lb)
    y, bn, gz, glb, gw, gb = _torch_reference(inp, G, n, F, relu)
    fw = bm.forward(inp.z, inp.lin_bias, inp.weight, inp.bias, inp.running_mean, inp.running_var, inp.nbt, G, n, bm.EPS,
                    bm.MOMENTUM, relu, torch.float64)
    _close(fw.y, y, "y")
    _close(fw.running_mean, bn.running_mean, "running_mean")
    _close(fw.running_var, bn.running_var, "running_var")
    assert fw.nbt == int(bn.num_batches_tracked) == bm.NBT_START + G
    x = inp.z.double() + (0.0 if inp.lin_bias is None else inp.lin_bias.double())
    for g in range(G):
        rows = x[g * n:(g + 1) * n]
        _close(fw.save_mean[g], rows.mean(0), "save_mean")
        _close(fw.save_invstd[g], 1.0 / torch.sqrt(rows.var(0, unbiased=False) + bm.EPS), "save_invstd")
    bw = bm.backward(inp.z, inp.lin_bias, inp.weight, inp.dy, (fw.y > 0) if relu else None, G, n, bm.EPS, torch.float64)
    _close(bw.dx, gz, "dx")
    _close(bw.gw, gw, "gw")
    _close(bw.gb, gb, "gb")
    _close(bw.g_lin_bias, glb if glb is not None else gz.sum(0), "g_lin_bias")


def test_fp64_model_none_arguments_mean_one_zero_absent():
    """weight / bias None: an affine-free BatchNorm1d; running statistics and counter None: none tracked."""
    G, n, F = 3, 9, 65
    inp = bm.make_inputs(G, n, F, False)
    y, _, gz, _, _, _ = _torch_reference(inp, G, n, F, 1, affine=False, track=False)
    fw = bm.forward(inp.z, None, None, None, None, None, None, G, n, bm.EPS, bm.MOMENTUM, 1, torch.float64)
    _close(fw.y, y, "y")
    assert fw.running_mean is None and fw.running_var is None and fw.nbt is None
    bw = bm.backward(inp.z, None, None, inp.dy, fw.y > 0, G, n, bm.EPS, torch.float64)
    _close(bw.dx, gz, "dx")
    ones, zeros = torch.ones(F), torch.zeros(F)
    fw1 = bm.forward(inp.z, zeros, ones, zeros, None, None, None, G, n, bm.EPS, bm.MOMENTUM, 1, torch.float64)
    assert torch.equal(fw1.y, fw.y)


def test_small_n_columns_keep_their_spread():
    for G, n, F, _, lb in bm.CASES:
        if n <= 3:
            z = bm.make_inputs(G, n, F, lb).z.view(G, n, F)
            assert z.double().std(dim=1, unbiased=False).min().item() >= bm.MIN_SPREAD * (1 - 1e-5)


@pytest.mark.parametrize("case", bm.CASES, ids=bm.CASE_IDS)
def test_fp32_kernel_order_holds_half_of_every_bound(case):
    """The bounds are attainable: fp32 arithmetic in the kernel's summation order stays within HALF of each bound of the
    fp64 mode on the same fp32 inputs, with the same ReLU mask in both backward runs."""
    G, n, F, relu, lb = case
    inp = bm.make_inputs(G, n, F, lb)
    args = (inp.z, inp.lin_bias, inp.weight, inp.bias, inp.running_mean, inp.running_var, inp.nbt, G, n, bm.EPS, bm.MOMENTUM, relu)
    ref, got = bm.forward(*args, torch.float64), bm.forward(*args, torch.float32)
    assert got.y.dtype == torch.float32 and got.nbt == ref.nbt
    mask = (ref.y > 0) if relu else None
    bref = bm.backward(inp.z, inp.lin_bias, inp.weight, inp.dy, mask, G, n, bm.EPS, torch.float64)
    bgot = bm.backward(inp.z, inp.lin_bias, inp.weight, inp.dy, mask, G, n, bm.EPS, torch.float32)
    fr = {k: bm.fraction_of_bound(k, getattr(got, k), getattr(ref, k))
          for k in ("y", "save_mean", "save_invstd", "running_mean", "running_var")}
    fr.update({k: bm.fraction_of_bound(k, getattr(bgot, k), getattr(bref, k)) for k in ("dx", "gw", "gb")})
    fr["g_lin_bias"] = bm.fraction_of_bound("g_lin_bias", bgot.g_lin_bias, bref.g_lin_bias, bm.lin_bias_scale(bref.dx, n))
    print({k: round(v, 4) for k, v in fr.items()})
    for k, v in fr.items():
        assert v <= 0.5, (k, v)

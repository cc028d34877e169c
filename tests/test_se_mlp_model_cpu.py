"""The fp64 model and the inputs of test_se_mlp_gpu.py (tests/se_mlp_model.py), checked on the CPU: the model is torch's
own hardsigmoid(linear(relu(linear(.)))) with its autograd, and the inputs of every shape put enough gate elements into each
region of the hard sigmoid and on each side of the ReLU."""
import pytest
import torch
import torch.nn.functional as F

import se_mlp_model as sm


@pytest.mark.parametrize("shape", sm.SHAPES, ids=sm.SHAPE_IDS)
def test_inputs_reach_every_region(shape):
    inp = sm.make_inputs(*shape)
    shares = sm.region_shares(sm.forward(inp.pooled, inp.w1, inp.b1, inp.w2, inp.b2))
    print(shape, {k: round(v, 3) for k, v in shares.items()})
    for k, least in sm.MIN_SHARE.items():
        assert shares[k] >= least, (k, shares[k])
    if shape in sm.VARIANT_SHAPES:                          # the runs without biases reach every region too
        shares = sm.region_shares(sm.forward(inp.pooled, inp.w1, None, inp.w2, None))
        for k, least in sm.MIN_SHARE.items():
            assert shares[k] >= least, (k, shares[k])


@pytest.mark.parametrize("shape", sm.SHAPES[:6], ids=sm.SHAPE_IDS[:6])
def test_model_is_torchs_gate_and_its_autograd(shape):
    B, C, Cs = shape
    inp = sm.make_inputs(B, C, Cs)
    leaves = [t.double().requires_grad_(True) for t in (inp.pooled, inp.w1, inp.b1, inp.w2, inp.b2)]
    p, w1, b1, w2, b2 = leaves
    h = F.relu(F.linear(p, w1, b1))                 # (a 1x1 convolution on a 1x1 map)
    z = F.linear(h, w2, b2)
    s = torch.clamp(z + 3.0, 0.0, 6.0) / 6.0        # (F.hardsigmoid's fp64 backward multiplies by a float 1 / 6: 5e-9 off)
    assert (s - F.hardsigmoid(z)).abs().max().item() <= 1e-15
    fw = sm.forward(inp.pooled, inp.w1, inp.b1, inp.w2, inp.b2)
    for got, want in ((fw.h, h), (fw.z, z), (fw.s, s)):
        assert (got - want.detach().view(got.shape)).abs().max().item() <= 1e-12 * max(1.0, got.abs().max().item())
    gp, gw1, gb1, gw2, gb2 = torch.autograd.grad(s, leaves, inp.gs.double())
    bw = sm.backward(inp.gs, fw.z, fw.h, inp.pooled, inp.w1, inp.w2)
    for got, want in ((bw.gp, gp), (bw.gw1, gw1), (bw.gb1, gb1), (bw.gw2, gw2), (bw.gb2, gb2)):
        assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())

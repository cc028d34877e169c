"""tests/conv_model.py (the fp64 reference and the derived bounds the depthwise and stem C-ABI tests use) against the literal
nested-loop definition, its exact input sets against the model, and fp32 F.conv2d on the CPU through the bounds at every
shape of the GPU tests' tables: a correct fp32 convolution must sit at half of each bound or below, or the bound proves
nothing on the GPU.  tests/dw_geometry.py: every case still reaches the kernel form it is listed for."""
import pytest
import torch
import torch.nn.functional as F

import conv_model as cm
import dw_geometry as dg
from helpers import randn

TINY = [(B, C, H, W, K, S) for (B, C) in ((2, 3),) for H in (1, 2, 3, 4) for W in (1, 2, 5, 6) for K in (3, 5) for S in (1, 2)]


def _dw_inputs(shape, seed=11):
    B, C, H, W, K, S = shape
    Ho, Wo = cm.out_size(H, K, S), cm.out_size(W, K, S)
    return randn((B, C, H, W), seed), randn((C, 1, K, K), seed + 1), randn((B, C, Ho, Wo), seed + 2)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 8, 15, 16, 30, 31, 240, 245])
@pytest.mark.parametrize("K,S", [(3, 1), (3, 2), (5, 1), (5, 2)])
def test_output_sizes(n, K, S):
    P = (K - 1) // 2
    want = (n + 2 * P - K) // S + 1
    assert cm.out_size(n, K, S) == want == dg.out_size(n, K, S)
    assert F.conv2d(torch.zeros(1, 1, n, n), torch.zeros(1, 1, K, K), None, S, P).shape[-1] == want


@pytest.mark.parametrize("shape", TINY, ids=lambda s: "x".join(map(str, s)))
def test_depthwise_model_is_the_nested_loop_definition(shape):
    B, C, H, W, K, S = shape
    x, w, g = _dw_inputs(shape)
    m = cm.dw_model(x, w, g, S)
    assert tuple(m.y.shape) == (B, C, cm.out_size(H, K, S), cm.out_size(W, K, S))
    y, gx, gw = cm.loops(x, w, g, S, C)
    for got, ref in ((m.y, y), (m.gx, gx), (m.gw, gw)):
        assert got.dtype == torch.float64 and (got - ref).abs().max().item() <= 1e-13 * max(1.0, ref.abs().max().item())
    ay, agx, agw = cm.loops(x.abs(), w.abs(), g.abs(), S, C)
    n = B * g.shape[2] * g.shape[3]
    for got, ref in ((m.y_bound, (K * K + 1) * cm.U * ay), (m.gx_bound, (K * K + 1) * cm.U * agx), (m.gw_bound, 1.01 * n * cm.U * agw)):
        assert (got - ref).abs().max().item() <= 1e-13 * ref.abs().max().item()


@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (3, 5), (4, 6), (1, 4), (5, 1)])
def test_stem_model_is_the_nested_loop_definition(H, W):
    Ho, Wo = cm.out_size(H, 3, 2), cm.out_size(W, 3, 2)
    x, w, g = randn((2, 3, H, W), 5), randn((16, 3, 3, 3), 6), randn((2, 16, Ho, Wo), 7)
    m = cm.stem_model(x, w, g)
    y, gx, gw = cm.loops(x, w, g, 2, 1)
    for got, ref in ((m.y, y), (m.gx, gx), (m.gw, gw)):
        assert (got - ref).abs().max().item() <= 1e-13 * max(1.0, ref.abs().max().item())
    ay, _, agw = cm.loops(x.abs(), w.abs(), g.abs(), 2, 1)
    assert (m.y_bound - 28 * cm.U * ay).abs().max().item() <= 1e-13 * ay.abs().max().item() * 28 * cm.U
    assert (m.gw_bound - 1.01 * 2 * Ho * Wo * cm.U * agw).abs().max().item() <= 1e-13 * m.gw_bound.max().item()


@pytest.mark.parametrize("shape", TINY, ids=lambda s: "x".join(map(str, s)))
def test_exact_sets_are_what_the_model_gives(shape):
    """The shifted copies and the tap counts (no arithmetic) equal the model on the one-hot / all-ones inputs, for every
    tap."""
    B, C, H, W, K, S = shape
    Ho, Wo = cm.out_size(H, K, S), cm.out_size(W, K, S)
    x, g = cm.ramp((B, C, H, W)), cm.ramp((B, C, Ho, Wo), 17)
    assert x.max().item() < 4096 and bool((x == x.round()).all())
    seen = set()
    for offset in range(0, K * K, C):
        w, taps = cm.one_hot_dw(C, K, offset), cm.dw_taps(C, K, offset)
        assert all(w[c, 0, kh, kw] == 1 for c, kh, kw in taps) and w.sum().item() == C
        seen |= {(kh, kw) for _, kh, kw in taps}
        m = cm.dw_model(x, w, g, S)
        assert torch.equal(cm.shift_forward(x, taps, K, S).double(), m.y)
        assert torch.equal(cm.shift_backward(g, taps, K, S, H, W).double(), m.gx)
    assert len(seen) == K * K
    counts, valid = cm.tap_counts(H, W, K, S)
    m = cm.dw_model(torch.ones(B, C, H, W), torch.ones(C, 1, K, K), torch.ones(B, C, Ho, Wo), S)
    assert torch.equal(m.y, counts.expand(B, C, Ho, Wo)) and torch.equal(m.gw, (B * valid).expand(C, 1, K, K))


def test_stem_exact_sets_are_what_the_model_gives():
    B, H, W = 2, 5, 6
    Ho, Wo = cm.out_size(H, 3, 2), cm.out_size(W, 3, 2)
    x, g = cm.ramp((B, 3, H, W)), torch.ones(B, 16, Ho, Wo)
    seen = set()
    for offset in (0, 16):
        w, taps = cm.one_hot_stem(offset), cm.stem_taps(offset)
        seen |= set(taps)
        assert torch.equal(cm.shift_forward(x, taps, 3, 2).double(), cm.stem_model(x, w, g).y)
    assert len(seen) == 27
    counts, valid = cm.tap_counts(H, W, 3, 2)
    m = cm.stem_model(torch.ones(B, 3, H, W), torch.ones(16, 3, 3, 3), g)
    assert torch.equal(m.y, (3 * counts).expand(B, 16, Ho, Wo)) and torch.equal(m.gw, (B * valid).expand(16, 3, 3, 3))


def test_ratio_flags_what_it_must():
    ref, bound = torch.tensor([1.0, 0.0, 2.0], dtype=torch.float64), torch.tensor([1e-6, 0.0, 1e-6], dtype=torch.float64)
    assert cm.ratio(torch.tensor([1.0, 0.0, 2.0]), ref, bound) == 0.0
    assert 0.4 < cm.ratio(torch.tensor([1.0 + 2.0 ** -21, 0.0, 2.0]), ref, bound) < 0.6
    assert cm.ratio(torch.tensor([1.0, 1e-30, 2.0]), ref, bound) == float("inf")        # must be exactly zero there
    assert cm.ratio(torch.tensor([1.0, 0.0, float("nan")]), ref, bound) == float("inf")


@pytest.mark.parametrize("case", dg.CASES + [dg.LDS_CASE], ids=dg.case_id)
def test_depthwise_cases_reach_their_forms_and_fp32_sits_at_half_the_bound(case):
    dg.assert_forms(case)
    B, C, H, W, K, S = case[0]
    x, w, g = cm.dw_inputs(case[0])
    m = cm.dw_model(x, w, g, S)
    xf, wf = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(xf, wf, None, S, (K - 1) // 2, 1, C)
    gx, gw = torch.autograd.grad(y, (xf, wf), g)
    r = (cm.ratio(y.detach(), m.y, m.y_bound), cm.ratio(gx, m.gx, m.gx_bound), cm.ratio(gw, m.gw, m.gw_bound))
    print("CONV-CPU-FP32 dw", dg.case_id(case), "forward %.3f gx %.3f gw %.4f" % r)
    assert max(r) <= 0.5, r


@pytest.mark.parametrize("case", dg.STEM_CASES, ids=lambda c: "x".join(map(str, c[0])))
def test_stem_cases_reach_their_forms_and_fp32_sits_at_half_the_bound(case):
    shape, want = case
    forms = dg.stem_forms(*shape)
    for k, v in want.items():
        assert forms[k] == v, (shape, k, forms[k], v)
    x, w, g = cm.stem_inputs(shape)
    m = cm.stem_model(x, w, g)
    wf = w.clone().requires_grad_(True)
    y = F.conv2d(x, wf, None, 2, 1)
    gw = torch.autograd.grad(y, wf, g)[0]
    r = (cm.ratio(y.detach(), m.y, m.y_bound), cm.ratio(gw, m.gw, m.gw_bound))
    print("CONV-CPU-FP32 stem", shape, "forward %.3f gw %.4f" % r)
    assert max(r) <= 0.5, r

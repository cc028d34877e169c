"""ias_dwconv_forward, ias_dwconv_backward_data and ias_dwconv_backward_weight (csrc/conv_kernels.hip) through the C ABI
against the fp64 model and the derived bounds of tests/conv_model.py, in the harness of tests/conv_capi.py (guards around
every buffer, NaN around the inputs, every output element and exactly the returned partial rows written).

Shapes: one per kernel form (tests/dw_geometry.py re-asserts which), then the shapes whose work exceeds the wave grid, so
that a wave walks several groups -- prefetching the next while it computes, storing one iteration late -- in the
whole-plane and the row-tiled form, and the weight gradient's batch chunks of 2, 3, 4 and 8 samples with a ragged last
chunk (dead steps) and a moved-back channel group.

Three input sets per shape: (a) seeded randn against the bounds; (b) an integer ramp through one-hot weights, a different
tap per channel and all K K taps: forward and input gradient are shifted copies, bit for bit; (c) all ones: the forward
counts the in-range taps, the weight gradient the valid positions per tap, exactly.  (b) and (c) run on buffers that have
just been through a randn run, and that randn run repeats (a)'s bits: what a wave or a workgroup left in LDS or registers
would show, and the weight gradient is deterministic."""
import pytest
import torch

import conv_model as cm
import dw_geometry as dg
from conv_capi import ConvRun, same_bits

pytestmark = pytest.mark.gpu
ARG, UNSUPPORTED = -1, -2


def _check_case(lib, dev, case, weight_gradient=True):
    dg.assert_forms(case)
    shape = case[0]
    B, C, H, W, K, S = shape
    run = ConvRun(lib, dev, "dw", shape)
    assert run.s1.t.numel() == dg.weight_scratch_floats(*shape)
    rows = dg.backward_weight_form(*shape)["rows"] if weight_gradient else None
    names = ["y", "gx"] + (["gw", "gw_multi"] if weight_gradient else [])

    # (a) randn against the bounds
    x, w, g = cm.dw_inputs(shape)
    m = cm.dw_model(x, w, g, S)
    run.load(x, w, g)
    a = run.run(lib, weight_gradient, rows)
    ratios = {"y": cm.ratio(a["y"], m.y, m.y_bound), "gx": cm.ratio(a["gx"], m.gx, m.gx_bound)}
    if weight_gradient:
        ratios["gw"] = cm.ratio(a["gw"], m.gw, m.gw_bound)
        ratios["gw_multi"] = cm.ratio(a["gw_multi"], m.gw, m.gw_bound)
    print("CONV-RATIO dw", dg.case_id(case), "randn", " ".join(f"{k}={v:.4f}" for k, v in ratios.items()), "rows", a["rows"])
    for k, v in ratios.items():
        assert v <= 1.0, (shape, k, v)

    # (b) ramp through one-hot weights: every tap; C < K K: as many weight sets as that takes
    xr, gr = cm.ramp((B, C, H, W)), cm.ramp((B, C, run.Ho, run.Wo), 17)
    for offset in range(0, K * K if C < K * K else 1, C):
        run.load(x, w, g)
        same_bits(run.run(lib, weight_gradient, rows), a, names)
        taps = cm.dw_taps(C, K, offset)
        run.load(xr, cm.one_hot_dw(C, K, offset), gr)
        b = run.run(lib, weight_gradient, rows)
        assert torch.equal(b["y"], cm.shift_forward(xr, taps, K, S)), (shape, "shift forward", offset)
        assert torch.equal(b["gx"], cm.shift_backward(gr, taps, K, S, H, W)), (shape, "shift input gradient", offset)

    # (c) all ones: counts
    counts, valid = cm.tap_counts(H, W, K, S)
    one = cm.dw_model(torch.ones(1, 1, H, W), torch.ones(1, 1, K, K), torch.ones(1, 1, run.Ho, run.Wo), S)
    assert B * valid.max().item() < 2 ** 24
    run.load(x, w, g)
    same_bits(run.run(lib, weight_gradient, rows), a, names)
    run.load(torch.ones(B, C, H, W), torch.ones(C, 1, K, K), torch.ones(B, C, run.Ho, run.Wo))
    c = run.run(lib, weight_gradient, rows)
    assert torch.equal(c["y"].double(), counts.expand(B, C, -1, -1)), (shape, "counts forward")
    assert torch.equal(c["gx"].double(), one.gx.expand(B, C, -1, -1)), (shape, "counts input gradient")
    if weight_gradient:
        assert torch.equal(c["gw"].double(), (B * valid).expand(C, 1, -1, -1)), (shape, "counts weight gradient")
        assert torch.equal(c["gw_multi"].double(), (B * valid).expand(C, 1, -1, -1)), (shape, "counts weight gradient, multi")


@pytest.mark.parametrize("case", dg.SMALL_CASES, ids=dg.case_id)
def test_one_shape_per_kernel_form(lib, dev, case):
    _check_case(lib, dev, case)


@pytest.mark.parametrize("case", dg.LOOPED_CASES, ids=dg.case_id)
def test_looped_waves_and_ragged_batch_chunks(lib, dev, case):
    _check_case(lib, dev, case)


def test_tiles_beyond_64_kb_of_lds_are_refused(lib, dev):
    """(1, 1, 3, 2100), K 5: the weight gradient's tile asks for 67 680 bytes of dynamic LDS -> IAS_ERR_UNSUPPORTED before any
    launch, nothing written; forward and input gradient (42 180 bytes) run and pass the model."""
    shape = dg.LDS_CASE[0]
    run = ConvRun(lib, dev, "dw", shape)
    run.load(*cm.dw_inputs(shape))
    assert run.backward_weight(lib, True) == UNSUPPORTED
    assert run.backward_weight(lib, False) == UNSUPPORTED
    assert run.untouched()
    _check_case(lib, dev, dg.LDS_CASE, weight_gradient=False)


def test_bad_arguments_are_refused_before_any_launch(lib, dev):
    shape = (2, 3, 8, 8, 3, 1)
    run = ConvRun(lib, dev, "dw", shape)
    run.load(*cm.dw_inputs(shape))
    for null in ("x", "w", "y"):
        assert run.forward(lib, null=null) == ARG, null
    for null in ("g", "w", "gx"):
        assert run.backward_data(lib, null=null) == ARG, null
    for null in ("x", "g", "scratch"):
        assert run.backward_weight(lib, True, null=null) == ARG, null
        assert run.backward_weight(lib, False, null=null) == ARG, null
    bad = [((0, 3, 8, 8, 3, 1), ARG), ((2, 0, 8, 8, 3, 1), ARG), ((2, 3, 0, 8, 3, 1), ARG), ((2, 3, 8, 0, 3, 1), ARG),
           ((65536, 32768, 8, 8, 3, 1), ARG), ((2, 3, 8, 8, 4, 1), UNSUPPORTED), ((2, 3, 8, 8, 3, 3), UNSUPPORTED)]
    for dims, status in bad:
        assert run.forward(lib, dims=dims) == status, dims
        assert run.backward_data(lib, dims=dims) == status, dims
        assert run.backward_weight(lib, True, dims=dims) == status, dims
        assert run.backward_weight(lib, False, dims=dims) == status, dims
    assert run.untouched()
    stem = ConvRun(lib, dev, "stem", (2, 9, 9))
    stem.load(*cm.stem_inputs((2, 9, 9)))
    for dims in ((65536, 9, 9), (0, 9, 9), (2, 0, 9), (2, 9, 0)):
        assert stem.forward(lib, dims=dims) == ARG, dims
        assert stem.backward_weight(lib, True, dims=dims) == ARG, dims
        assert stem.backward_weight(lib, False, dims=dims) == ARG, dims
    for null in ("x", "w", "y"):
        assert stem.forward(lib, null=null) == ARG, null
    for null in ("x", "g", "scratch"):
        assert stem.backward_weight(lib, True, null=null) == ARG, null
    assert stem.untouched()

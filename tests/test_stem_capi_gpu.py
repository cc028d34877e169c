"""ias_stem_forward and ias_stem_backward_weight (csrc/conv_kernels.hip) through the C ABI against the fp64 model and the
derived bounds of tests/conv_model.py, in the harness of tests/conv_capi.py.  Shapes at the edges of the staged forms
(Wo 65 and 128, W 255 / 256 / 257, Ho 59 / 60 / 61 around the forward's 60 chunks, Ho 17 and 33 around the backward's 16
and 32 chunks); the forms only a switch of the diagnostic library reaches (the VALU forward, which the product library
takes for images of 2^31 / 3 pixels and more, both gather forms, the LDS weight gradient) at two of them.

Input sets as in tests/test_dwconv_capi_gpu.py: (a) seeded randn against the bounds (28 terms forward); (b) an integer
ramp through one-hot weights, one of the 27 taps per output channel and all 27 over two weight sets: the forward is a
shifted copy, bit for bit; (c) all ones: exact counts, forward and weight gradient.  (b) and (c) follow a randn run on
the same buffers, which repeats (a)'s bits."""
import os

import pytest
import torch

import conv_model as cm
import dw_geometry as dg
from conv_capi import ConvRun, same_bits

pytestmark = pytest.mark.gpu
NAMES = ("y", "gw", "gw_multi")


def _check_shape(lib, dev, shape, rows, tag):
    B, H, W = shape
    run = ConvRun(lib, dev, "stem", shape)
    x, w, g = cm.stem_inputs(shape)
    m = cm.stem_model(x, w, g)
    run.load(x, w, g)
    a = run.run(lib, True, rows)
    ratios = {"y": cm.ratio(a["y"], m.y, m.y_bound), "gw": cm.ratio(a["gw"], m.gw, m.gw_bound),
              "gw_multi": cm.ratio(a["gw_multi"], m.gw, m.gw_bound)}
    print("CONV-RATIO stem", "x".join(map(str, shape)), tag, "randn", " ".join(f"{k}={v:.4f}" for k, v in ratios.items()),
          "rows", a["rows"])
    for k, v in ratios.items():
        assert v <= 1.0, (shape, tag, k, v)

    xr = cm.ramp((B, 3, H, W))
    seen = set()
    for offset in (0, 16):
        run.load(x, w, g)
        same_bits(run.run(lib, True, rows), a, NAMES)
        taps = cm.stem_taps(offset)
        seen |= set(taps)
        run.load(xr, cm.one_hot_stem(offset), g)
        b = run.run(lib, True, rows)
        assert torch.equal(b["y"], cm.shift_forward(xr, taps, 3, 2)), (shape, tag, "shift forward", offset)
    assert len(seen) == 27

    counts, valid = cm.tap_counts(H, W, 3, 2)
    assert B * valid.max().item() < 2 ** 24
    run.load(x, w, g)
    same_bits(run.run(lib, True, rows), a, NAMES)
    run.load(torch.ones(B, 3, H, W), torch.ones(16, 3, 3, 3), torch.ones(B, 16, run.Ho, run.Wo))
    c = run.run(lib, True, rows)
    assert torch.equal(c["y"].double(), (3 * counts).expand(B, 16, -1, -1)), (shape, tag, "counts forward")
    for k in ("gw", "gw_multi"):
        assert torch.equal(c[k].double(), (B * valid).expand(16, 3, -1, -1)), (shape, tag, "counts", k)


@pytest.mark.parametrize("case", dg.STEM_CASES, ids=lambda c: "x".join(map(str, c[0])))
def test_stem_shapes_at_the_edges_of_the_staged_forms(lib, dev, case):
    shape, want = case
    forms = dg.stem_forms(*shape)
    for k, v in want.items():
        assert forms[k] == v, (shape, k, forms[k], v)
    _check_shape(lib, dev, shape, forms["rows"], "product")


# switch -> partial rows per sample of the weight gradient under it (None: the product's choice)
SWITCHES = {"IAS_STEM_VALU": None, "IAS_STEM_FWD_GATHER": None, "IAS_STEM_GW_GATHER": 32, "IAS_STEM_GW_LDS": 32}


@pytest.mark.parametrize("switch", list(SWITCHES))
@pytest.mark.parametrize("shape", [(2, 7, 129), (3, 17, 10)], ids=lambda s: "x".join(map(str, s)))
def test_stem_forms_behind_diagnostic_switches(dev, shape, switch):
    """The diagnostic library reads its switches at every call: set around the calls, removed afterwards."""
    from inverse_audio_synthesis_amd import _lib
    diag = _lib.load_diag()
    per_sample = SWITCHES[switch]
    rows = shape[0] * per_sample if per_sample else dg.stem_forms(*shape)["rows"]
    assert switch not in os.environ
    os.environ[switch] = "1"
    try:
        _check_shape(diag, dev, shape, rows, switch)
    finally:
        del os.environ[switch]

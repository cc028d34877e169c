"""ias_pwconv_forward, ias_pwconv_backward_data and ias_pwconv_backward_weight (csrc/pointwise_kernels.hip) through the C ABI
against the fp64 model and the derived bounds of tests/pw_model.py, in the harness of tests/pw_capi.py (guards around every
buffer, NaN around the inputs, every output element and exactly the returned partial rows written).

Shapes (tests/pw_geometry.py re-asserts what each reaches): the degenerate forms small batches take, then the forms of a
training batch -- several row tiles per wave with a ragged last group, the grid-stride loop on the capped grid, launches
with more than 64 KB of dynamic LDS, several 64-position chunks per weight-gradient split with a short last split, splits
past the last chunk, dead waves.  Every case runs without and with the squeeze-excitation scale.

Input sets per shape: (a) seeded randn against the bounds, twice on the same buffers for the same bits; (b) small integers
with power-of-two scales: all four results equal the fp64 model bit for bit; (c) one-hot weight rows on ramps, two column
offsets: the forward is a row copy, the input gradient an exact sum of rows.  The exact sets run on buffers that have just
been through the randn run."""
import pytest
import torch

import pw_geometry as pg
import pw_model as pm
from pw_capi import PwRun, same_bits

pytestmark = pytest.mark.gpu
ARG, UNSUPPORTED = -1, -2


def _ratios(res, m):
    return {"y": pm.ratio(res["y"], m.y, m.y_bound), "gx": pm.ratio(res["gx"], m.gx, m.gx_bound),
            "gw": pm.ratio(res["gw"], m.gw, m.gw_bound), "gw_multi": pm.ratio(res["gw_multi"], m.gw, m.gw_bound)}


def _check_randn(lib, run, scaled, tag):
    """(a): two runs on the same buffers -> the first run's results."""
    x, s, w, g = pm.randn_inputs(run.shape)
    m = pm.model(x, s if scaled else None, w, g)
    run.load(x, s, w, g)
    a = run.run(lib, scaled)
    ratios = _ratios(a, m)
    print("PW-RATIO", "x".join(map(str, run.shape)), tag, "scaled" if scaled else "plain", "randn",
          " ".join(f"{k}={v:.3g}" for k, v in ratios.items()), "rows", a["rows"])
    for k, v in ratios.items():
        assert v <= 1.0, (run.shape, tag, scaled, k, v)
    same_bits(run.run(lib, scaled), a)
    return a


def _check_integers(lib, run, scaled, tag):
    """(b): every result equals the fp64 model."""
    x, s, w, g = pm.integer_inputs(run.shape)
    y, gx, gw = pm.values(x, s if scaled else None, w, g)
    run.load(x, s, w, g)
    b = run.run(lib, scaled)
    for k, ref in (("y", y), ("gx", gx), ("gw", gw), ("gw_multi", gw)):
        wrong = (b[k].double() != ref).nonzero()
        assert wrong.numel() == 0, (run.shape, tag, scaled, k, "integer set: first wrong index", wrong[0].tolist(), len(wrong))


def _check_case(lib, dev, case, scaled):
    pg.assert_forms(case)
    shape = case[0]
    B, Cin, Cout, HW = shape
    run = PwRun(lib, dev, shape)
    assert run.vecs() == (case[1],) * 3
    a = _check_randn(lib, run, scaled, "aligned")
    x, s, w, g = pm.randn_inputs(shape)

    if scaled:      # the header: same bits as ias_se_scale followed by ias_pwconv_forward
        run.load(x * s[:, :, None], s, w, g)
        assert torch.equal(run.run(lib, False)["y"], a["y"]), (shape, "the scaled forward is not the forward of x * s")

    _check_integers(lib, run, scaled, "aligned")

    # (c) one-hot rows on ramps
    for offset in pm.ONE_HOT_OFFSETS:
        xr, wo, gr = pm.one_hot_inputs(shape, offset)
        si = pm.integer_inputs(shape)[1]
        y, gx = pm.one_hot_results(xr, si if scaled else None, gr, Cin, offset)
        run.load(xr, si, wo, gr)
        c = run.run(lib, scaled)
        assert torch.equal(c["y"].double(), y), (shape, scaled, "one-hot forward", offset)
        assert torch.equal(c["gx"].double(), gx), (shape, scaled, "one-hot input gradient", offset)

    run.load(x, s, w, g)
    same_bits(run.run(lib, scaled), a)


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("case", pg.CASES, ids=pg.case_id)
def test_every_form_against_the_model(lib, dev, case, scaled):
    _check_case(lib, dev, case, scaled)


def test_a_sample_has_the_same_bits_in_every_form(lib, dev):
    """Every output element of pw_apply receives its k-steps in the same order whatever cg, VEC, the grid or B: samples 0 and
    64 of the (65, 72, 72, 2044) call (cg 4, the stride loop) against a call on those two samples alone (cg 1, no loop)."""
    shape = (65, 72, 72, 2044)
    big, small = pg.forward_form(*shape), pg.forward_form(2, *shape[1:])
    assert (big["cg"], big["looped"], small["cg"], small["looped"]) == (4, True, 1, False)
    x, s, w, g = pm.randn_inputs(shape)
    run = PwRun(lib, dev, shape)
    run.load(x, s, w, g)
    pick = [0, 64]
    two = PwRun(lib, dev, (2,) + shape[1:])
    two.load(x[pick], s[pick], w, g[pick])
    for scaled in (False, True):
        a, b = run.run(lib, scaled), two.run(lib, scaled)
        assert torch.equal(a["y"][pick], b["y"]), scaled
        assert torch.equal(a["gx"][pick], b["gx"]), scaled


# buffer moved -> (forward, input gradient, weight gradient) VEC at an offset of 1 float; an offset of 2: 2 where this has 1
MOVED = {"x": (1, 4, 1), "y": (1, 4, 4), "g": (4, 1, 1), "gx": (4, 1, 4)}


@pytest.mark.parametrize("offset", [1, 2])
@pytest.mark.parametrize("name", list(MOVED))
def test_activations_off_16_byte_alignment(lib, dev, name, offset):
    """HW % 4 == 0, so VEC follows the pointers alone: 1 at an odd float offset, 2 at 2 floats (pw_geometry's prediction from
    the buffers' addresses); results, guards and written elements as in the aligned cases."""
    shape = pg.MISALIGNED_SHAPE
    assert shape[3] % 4 == 0 and pg.supported(shape[1], shape[2])
    run = PwRun(lib, dev, shape, offsets={name: offset})
    assert run.vecs() == tuple(v if v == 4 else offset for v in MOVED[name]), (name, offset, run.vecs())
    for scaled in (False, True):
        _check_randn(lib, run, scaled, f"{name}+{offset}")
        _check_integers(lib, run, scaled, f"{name}+{offset}")


def test_a_weight_off_16_byte_alignment_is_refused(lib, dev):
    shape = pg.MISALIGNED_SHAPE
    for offset in (1, 2, 3):
        run = PwRun(lib, dev, shape, offsets={"w": offset})
        run.load(*pm.randn_inputs(shape))
        for scaled in (False, True):
            assert run.forward(lib, scaled) == ARG, offset
        assert run.backward_data(lib) == ARG, offset
        assert run.untouched()


def test_bad_arguments_are_refused_before_any_launch(lib, dev):
    shape = (2, 8, 12, 9)
    run = PwRun(lib, dev, shape)
    run.load(*pm.randn_inputs(shape))
    for scaled in (False, True):
        for null in ("x", "w", "y"):
            assert run.forward(lib, scaled, null=null) == ARG, null
        for null in ("g", "x", "scratch"):
            assert run.backward_weight(lib, True, scaled, null=null) == ARG, null
            assert run.backward_weight(lib, False, scaled, null=null) == ARG, null
    for null in ("g", "w", "gx"):
        assert run.backward_data(lib, null=null) == ARG, null
    bad = [((0, 8, 12, 9), ARG), ((-1, 8, 12, 9), ARG), ((2, 8, 12, 0), ARG), ((2, 8, 12, -3), ARG),
           ((2, 6, 8, 9), UNSUPPORTED), ((2, 8, 6, 9), UNSUPPORTED), ((2, 244, 16, 9), UNSUPPORTED),
           ((2, 132, 128, 9), UNSUPPORTED), ((2, 64, 260, 9), UNSUPPORTED)]
    for dims, status in bad:
        for scaled in (False, True):
            assert run.forward(lib, scaled, dims=dims) == status, dims
            assert run.backward_weight(lib, True, scaled, dims=dims) == status, dims
            assert run.backward_weight(lib, False, scaled, dims=dims) == status, dims
        assert run.backward_data(lib, dims=dims) == status, dims
    for dims in bad[:4]:
        assert lib.ias_pwconv_weight_scratch(*dims[0]) == ARG == pg.weight_scratch_floats(*dims[0]), dims
    assert run.untouched()


def test_supported_is_the_stated_rule(lib):
    """Host calls only: channel counts multiples of 4, both 16-padded orientations of the weight within 16384 floats,
    Cin <= 240."""
    for cin in range(1, 321):
        for cout in range(1, 321):
            assert lib.ias_pwconv_supported(cin, cout) == pg.supported(cin, cout), (cin, cout)
    for pair in ((0, 16), (16, 0), (-4, 16), (16, -4)):
        assert lib.ias_pwconv_supported(*pair) == 0 == pg.supported(*pair), pair

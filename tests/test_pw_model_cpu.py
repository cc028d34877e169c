"""tests/pw_model.py (the fp64 reference and the derived bounds the 1x1 convolutions' C-ABI tests use) against the literal
triple-loop definition, its exact input sets against the model, and fp32 arithmetic on the CPU through the bounds at every
shape of the GPU tests' table: the reference alone must satisfy them, or they prove nothing on the GPU.
tests/pw_geometry.py: every case still reaches the kernel forms it is listed for."""
import pytest
import torch

import pw_geometry as pg
import pw_model as pm

TINY = [(1, 4, 4, 1), (2, 4, 8, 3), (3, 8, 4, 5), (2, 12, 20, 2)]
SCALED = pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])


def _close(got, ref):
    return got.dtype == torch.float64 and (got - ref).abs().max().item() <= 1e-13 * max(1e-30, ref.abs().max().item())


@SCALED
@pytest.mark.parametrize("shape", TINY, ids=lambda s: "x".join(map(str, s)))
def test_model_is_the_triple_loop_definition(shape, scaled):
    B, Cin, Cout, HW = shape
    x, s, w, g = pm.randn_inputs(shape, seed=7)
    s = s if scaled else None
    m = pm.model(x, s, w, g)
    assert tuple(m.y.shape) == (B, Cout, HW) and tuple(m.gx.shape) == (B, Cin, HW) and tuple(m.gw.shape) == (Cout, Cin)
    y, gx, gw = pm.loops(x, s, w, g)
    assert _close(m.y, y) and _close(m.gx, gx) and _close(m.gw, gw)
    ay, agx, agw = pm.loops(x.abs(), s, w.abs(), g.abs())
    u = 2.0 ** -24
    ny, ngx, ngw = (3 if scaled else 2) * Cin + 2, 2 * Cout + 2, 2 * B * HW + (3 if scaled else 2)
    assert _close(m.y_bound, ny * u / (1 - ny * u) * ay)
    assert _close(m.gx_bound, ngx * u / (1 - ngx * u) * agx)
    assert _close(m.gw_bound, ngw * u / (1 - ngw * u) * agw)


def test_gamma_needs_n_u_below_one():
    assert pm.gamma(1) == 2.0 ** -24 / (1 - 2.0 ** -24)
    with pytest.raises(AssertionError):
        pm.gamma(2 ** 24)


@SCALED
@pytest.mark.parametrize("case", pg.CASES, ids=pg.case_id)
def test_cases_reach_their_forms_and_cpu_fp32_satisfies_the_bounds(case, scaled):
    pg.assert_forms(case)
    x, s, w, g = pm.randn_inputs(case[0])
    assert 0.0 < s.min().item() and s.max().item() <= 1.0
    s = s if scaled else None
    m = pm.model(x, s, w, g)
    xs = x if s is None else x * s[:, :, None]
    y, gx, gw = torch.einsum("mk,bkp->bmp", w, xs), torch.einsum("mk,bmp->bkp", w, g), torch.einsum("bmp,bkp->mk", g, xs)
    r = (pm.ratio(y, m.y, m.y_bound), pm.ratio(gx, m.gx, m.gx_bound), pm.ratio(gw, m.gw, m.gw_bound))
    print("PW-CPU-FP32", pg.case_id(case), "scaled" if scaled else "plain", "forward %.4f gx %.4f gw %.5f" % r)
    assert max(r) <= 1.0, r


@SCALED
@pytest.mark.parametrize("case", pg.CASES, ids=pg.case_id)
def test_integer_set_is_exact_in_fp32(case, scaled):
    """Every sum of magnitudes stays below 2^24 halves, and plain fp32 arithmetic on the CPU gives the fp64 model's values."""
    shape = case[0]
    assert pm.integer_set_halves(shape) < 2 ** 24
    x, s, w, g = pm.integer_inputs(shape)
    assert x.abs().max() <= 4 and g.abs().max() <= 4 and w.abs().max() <= 3 and set(s.unique().tolist()) <= {0.5, 1.0, 2.0}
    assert all(bool((t == t.round()).all()) for t in (x, w, g))
    s = s if scaled else None
    ref = pm.values(x, s, w, g)
    xs = x if s is None else x * s[:, :, None]
    got = (torch.einsum("mk,bkp->bmp", w, xs), torch.einsum("mk,bmp->bkp", w, g), torch.einsum("bmp,bkp->mk", g, xs))
    for a, b in zip(got, ref):
        assert a.dtype == torch.float32 and torch.equal(a.double(), b)
    assert bool((ref[2] * 2 == (ref[2] * 2).round()).all()) and ref[2].abs().max().item() * 2 < 2 ** 24
    assert ref[2].abs().max().item() > 0


def test_integer_set_refuses_a_shape_whose_sums_could_round():
    with pytest.raises(AssertionError):
        pm.integer_inputs((128, 16, 16, 4096))


@SCALED
@pytest.mark.parametrize("shape", TINY + [(7, 8, 12, 9), (3, 16, 24, 132)], ids=lambda s: "x".join(map(str, s)))
def test_one_hot_set_is_what_the_model_gives(shape, scaled):
    B, Cin, Cout, HW = shape
    seen = set()
    for offset in pm.ONE_HOT_OFFSETS:
        x, w, g = pm.one_hot_inputs(shape, offset)
        assert bool((w.sum(dim=1) == 1).all()) and all(w[m, (7 * m + offset) % Cin] == 1 for m in range(Cout))
        seen |= set(pm.one_hot_columns(Cout, Cin, offset).tolist())
        s = pm.integer_inputs(shape)[1] if scaled else None
        y, gx, _ = pm.values(x, s, w, g)
        ry, rgx = pm.one_hot_results(x, s, g, Cin, offset)
        assert torch.equal(ry, y) and torch.equal(rgx, gx)
        assert gx.abs().max().item() < 2 ** 23
    assert Cout < Cin or seen == set(range(Cin))


def test_supported_rule_on_the_shapes_the_tests_name():
    assert all(pg.supported(*c[0][1:3]) == 1 for c in pg.CASES) and pg.supported(*pg.MISALIGNED_SHAPE[1:3]) == 1
    for pair in ((6, 8), (8, 6), (244, 16), (132, 128), (64, 260), (0, 4), (4, 0)):
        assert pg.supported(*pair) == 0, pair
    assert pg.supported(240, 40) == 1 and pg.supported(128, 128) == 1 and pg.supported(64, 256) == 1


def test_vec_follows_pointer_bits_and_hw():
    assert pg.vec(0, 16, 132) == 4 and pg.vec(4, 0, 132) == 1 and pg.vec(0, 8, 132) == 2 and pg.vec(0, 12, 132) == 1
    assert pg.vec(0, 0, 130) == 2 and pg.vec(0, 0, 9) == 1 and pg.vec(8, 8, 130) == 2

"""ias_bn1d_groups_forward / _backward (csrc/bn_kernels.hip) through the C ABI against the fp64 model of
tests/bn1d_model.py on the same fp32 inputs: every case of the model's table (all kernel forms, their row-count
boundaries, dead lanes), writes outside the outputs, the counter, the ReLU mask on the kink, nullable pointers, refused
arguments, determinism, stacked against separate calls, constant columns; and the Python gates in front of the kernels
(vicreg.project_pair, paramembed.linear_norm).  Every output lives inside a larger buffer filled with a sentinel, so
every test also sees a write outside its outputs."""
import copy

import pytest
import torch

import bn1d_model as bm
from helpers import Guarded, SENT, randn

pytestmark = pytest.mark.gpu

OUTPUTS = ("y", "save_mean", "save_invstd", "running_mean", "running_var", "nbt", "dx", "gw", "gb", "g_lin_bias")


class Run:
    """The device side of one call pair: inputs, guarded outputs.  `null`: names passed as NULL."""

    def __init__(self, dev, inp, G, n, F, null=(), share=None):
        def up(name):
            t = getattr(inp, name)
            return None if (name in null or t is None) else t.to(dev)
        self.G, self.n, self.F = G, n, F
        self.z, self.dy = inp.z.to(dev), inp.dy.to(dev)
        self.lin_bias, self.weight, self.bias = up("lin_bias"), up("weight"), up("bias")
        self.y, self.dx = Guarded(dev, (G * n, F)), Guarded(dev, (G * n, F))
        self.save_mean, self.save_invstd = Guarded(dev, (G, F)), Guarded(dev, (G, F))
        if share is not None:              # the running statistics and the counter of another Run (chained calls)
            self.running_mean, self.running_var, self.nbt = share.running_mean, share.running_var, share.nbt
        else:
            self.running_mean = None if "running_mean" in null else Guarded(dev, (F,), inp.running_mean)
            self.running_var = None if "running_var" in null else Guarded(dev, (F,), inp.running_var)
            self.nbt = None if "nbt" in null else Guarded(dev, (1,), torch.tensor([inp.nbt]), dtype=torch.int64)
        self.gw, self.gb, self.g_lin_bias = (None if k in null else Guarded(dev, (F,)) for k in ("gw", "gb", "g_lin_bias"))

    @staticmethod
    def _p(g):
        from inverse_audio_synthesis_amd import _lib
        return None if g is None else _lib.ptr(g.t if isinstance(g, Guarded) else g)

    def forward(self, lib, relu, eps=bm.EPS, momentum=bm.MOMENTUM, G=None, n=None, F=None, null=()):
        from inverse_audio_synthesis_amd import _lib
        p = lambda k: None if k in null else self._p(getattr(self, k))
        return lib.ias_bn1d_groups_forward(p("z"), p("lin_bias"), p("weight"), p("bias"), p("running_mean"), p("running_var"),
                                           p("nbt"), p("y"), p("save_mean"), p("save_invstd"), self.G if G is None else G,
                                           self.n if n is None else n, self.F if F is None else F, eps, momentum, relu,
                                           _lib.stream())

    def backward(self, lib, relu, G=None, n=None, F=None, null=(), stats=None):
        from inverse_audio_synthesis_amd import _lib
        p = lambda k: None if k in null else self._p(getattr(self, k))
        mean, invstd = (p("save_mean"), p("save_invstd")) if stats is None else (_lib.ptr(stats[0]), _lib.ptr(stats[1]))
        return lib.ias_bn1d_groups_backward(p("z"), p("lin_bias"), p("dy"), p("weight"), p("bias"), mean, invstd, p("dx"),
                                            p("gw"), p("gb"), p("g_lin_bias"), self.G if G is None else G,
                                            self.n if n is None else n, self.F if F is None else F, relu, _lib.stream())

    def guarded(self):
        return {k: getattr(self, k) for k in OUTPUTS if getattr(self, k) is not None}

    def guards_intact(self):
        torch.cuda.synchronize()
        return all(g.guards_intact() for g in self.guarded().values())

    def out(self):
        torch.cuda.synchronize()
        return {k: g.cpu() for k, g in self.guarded().items()}


def _both(lib, dev, inp, G, n, F, relu, null=()):
    run = Run(dev, inp, G, n, F, null)
    assert run.forward(lib, relu) == 0
    assert run.backward(lib, relu) == 0
    assert run.guards_intact()
    return run, run.out()


def _reference(inp, G, n, F, relu, y_kernel, eps=bm.EPS):
    """The fp64 model on the fp32 inputs; the backward's ReLU mask is the kernel's own y > 0."""
    fw = bm.forward(inp.z, inp.lin_bias, inp.weight, inp.bias, inp.running_mean, inp.running_var, inp.nbt, G, n, eps,
                    bm.MOMENTUM, relu, torch.float64)
    bw = bm.backward(inp.z, inp.lin_bias, inp.weight, inp.dy, (y_kernel > 0) if relu else None, G, n, eps, torch.float64)
    return fw, bw


def _fractions(out, fw, bw, n):
    """Every quantity's largest error as a fraction of its bound."""
    fr = {k: bm.fraction_of_bound(k, out[k], getattr(fw, k)) for k in ("y", "save_mean", "save_invstd", "running_mean", "running_var")
          if k in out}
    fr.update({k: bm.fraction_of_bound(k, out[k], getattr(bw, k)) for k in ("dx", "gw", "gb") if k in out})
    if "g_lin_bias" in out:
        fr["g_lin_bias"] = bm.fraction_of_bound("g_lin_bias", out["g_lin_bias"], bw.g_lin_bias, bm.lin_bias_scale(bw.dx, n))
    return fr


def _assert_within_bounds(out, fw, bw, n, tag):
    fr = _fractions(out, fw, bw, n)
    print("BN1D-FRACTIONS", tag, {k: round(v, 4) for k, v in fr.items()})
    for k, v in out.items():
        assert bool(torch.isfinite(v.double()).all()), k
    for k, v in fr.items():
        assert v <= 1.0, (tag, k, v)
    if "nbt" in out:
        assert int(out["nbt"]) == fw.nbt


@pytest.mark.parametrize("case", bm.CASES, ids=bm.CASE_IDS)
def test_every_case_of_the_table_against_the_fp64_model(lib, dev, case):
    G, n, F, relu, lb = case
    inp = bm.make_inputs(G, n, F, lb)
    _, out = _both(lib, dev, inp, G, n, F, relu)
    fw, bw = _reference(inp, G, n, F, relu, out["y"])
    _assert_within_bounds(out, fw, bw, n, bm.CASE_IDS[bm.CASES.index(case)])


@pytest.mark.parametrize("F", [1, 63, 65, 130])
def test_nothing_is_written_outside_the_outputs(lib, dev, F):
    """Dead lanes (F not a multiple of the 64-feature workgroup) on each kernel form: 64 floats of guard on either side of
    every output are unchanged after both launches, and every element inside was written."""
    for G, n in ((2, 9), (3, 130), (1, 300), (4, 128)):
        inp = bm.make_inputs(G, n, F, True, seed=1)
        run = Run(dev, inp, G, n, F)
        assert run.forward(lib, 1) == 0 and run.backward(lib, 1) == 0
        assert run.guards_intact(), (G, n, F)
        for k in ("y", "save_mean", "save_invstd", "dx", "gw", "gb", "g_lin_bias"):
            assert not bool((getattr(run, k).t == SENT).any()), (k, G, n, F)


@pytest.mark.parametrize("G,n", [(3, 20), (2, 128), (4, 300)])
def test_counter_goes_up_by_G_per_call_with_three_workgroups(lib, dev, G, n):
    F = 130
    inp = bm.make_inputs(G, n, F, True, seed=2)
    run = Run(dev, inp, G, n, F)
    assert run.forward(lib, 1) == 0
    assert int(run.out()["nbt"]) == bm.NBT_START + G
    assert run.forward(lib, 1) == 0
    assert int(run.out()["nbt"]) == bm.NBT_START + 2 * G
    assert run.guards_intact()


@pytest.mark.parametrize("n", [128, 200, 300])
def test_relu_mask_on_the_kink_is_the_forwards_mask(lib, dev, n):
    """Pre-activation values within one rounding of zero: the bias of every column is moved by the kernel's own
    pre-activation value of one row of group 0, so that row's new value is (about) zero; dy is 1 at that row and at one
    row of group 1.  The backward recomputes the mask in another kernel instantiation; a mask that disagrees with the
    forward's y > 0 at such an element moves dx by O(weight * invstd), four orders above the bound.  Three columns are
    constant within each group: their centred rows are exactly 0, the same step leaves their bias exactly 0 and every
    pre-activation value of theirs exactly 0 -- shut by the forward (0 > 0 is false), so `>=` in the backward shows."""
    G, F = 2, 65
    inp = bm.make_inputs(G, n, F, True, seed=3)
    flat = torch.tensor([1, 33, 64])
    z = inp.z.view(G, n, F).clone()
    z[:, :, flat] = z[:, :1, flat]
    inp = inp._replace(z=z.view(G * n, F))
    pre = Run(dev, inp, G, n, F)
    assert pre.forward(lib, 0) == 0
    v = pre.out()["y"].view(G, n, F)
    cols = torch.arange(F)
    rows = torch.stack([(cols * 7 + 3) % n, (cols * 5 + 1) % n])                 # [G, F]: r* of each column and group
    bias = inp.bias - v[0, rows[0], cols]                                        # fp32
    dy = torch.zeros(G, n, F)
    dy[0, rows[0], cols] = 1.0
    dy[1, rows[1], cols] = 1.0
    inp = inp._replace(bias=bias, dy=dy.view(G * n, F))
    pre = Run(dev, inp, G, n, F)
    assert pre.forward(lib, 0) == 0
    assert bool((pre.out()["y"].view(G, n, F)[:, :, flat] == 0).all())          # exactly on the kink, both groups
    _, out = _both(lib, dev, inp, G, n, F, 1)
    y = out["y"].view(G, n, F)
    at = y[0, rows[0], cols]
    fw0 = bm.forward(inp.z, inp.lin_bias, inp.weight, inp.bias, None, None, None, G, n, bm.EPS, bm.MOMENTUM, 0, torch.float64)
    pre64 = fw0.y.view(G, n, F)[0, rows[0], cols]
    on_kink = bm.bound("y", fw0.y) + 1e-6            # the kernel's v is within the y bound of the model's, the new bias one rounding more
    print("BN1D-KINK", n, "elements on the kink:", F, "passed by the forward:", int((at > 0).sum()),
          "largest |pre-activation| (fp64 model):", pre64.abs().max().item())
    # the rows are on the kink: what is left of v - fl(v) after the bias took fl(bias - v), two roundings of values below 16
    assert pre64.abs().max().item() <= on_kink and at.max().item() <= 4e-6
    fw, bw = _reference(inp, G, n, F, 1, out["y"])
    _assert_within_bounds(out, fw, bw, n, f"kink-n{n}")
    # the backward saw what the forward saw: with the forward's row shut, group 0's column has no gradient at all
    dx0 = out["dx"].view(G, n, F)[0]
    shut = at <= 0
    assert bool(shut[flat].all()) and bool((dx0[:, shut] == 0).all())
    assert bool((out["dx"].view(G, n, F)[1][:, flat] == 0).all())
    assert bool((dx0[rows[0], cols][~shut] != 0).all())


def _same_bits(a, b, keys, tag):
    for k in keys:
        assert torch.equal(a[k], b[k]), (tag, k)


@pytest.mark.parametrize("G,n,F", [(2, 20, 65), (3, 257, 130), (1, 200, 63)])
def test_nullable_pointers(lib, dev, G, n, F):
    """Each nullable pointer alone: the remaining outputs carry the bits of the call with every pointer given (or with
    explicit ones / zeros where NULL stands for them)."""
    inp = bm.make_inputs(G, n, F, True, seed=4)
    _, full = _both(lib, dev, inp, G, n, F, 1)
    everything = set(full)
    for null in (("running_mean", "running_var"), ("nbt",), ("gw",), ("gb",), ("g_lin_bias",)):
        _, out = _both(lib, dev, inp, G, n, F, 1, null)
        assert set(out) == everything - set(null)
        _same_bits(out, full, out.keys(), null)
    ones, zeros = torch.ones(F), torch.zeros(F)
    _, explicit = _both(lib, dev, inp._replace(weight=ones, bias=zeros), G, n, F, 1)
    _, out = _both(lib, dev, inp, G, n, F, 1, ("weight", "bias"))
    _same_bits(out, explicit, everything, "weight, bias")
    fw, bw = _reference(inp._replace(weight=None, bias=None), G, n, F, 1, out["y"])
    _assert_within_bounds(out, fw, bw, n, f"null-affine-G{G}-n{n}-F{F}")
    _, explicit = _both(lib, dev, inp._replace(lin_bias=zeros), G, n, F, 1)
    _, out = _both(lib, dev, inp, G, n, F, 1, ("lin_bias",))
    _same_bits(out, explicit, everything - {"g_lin_bias"}, "lin_bias")
    assert torch.equal(out["g_lin_bias"], explicit["g_lin_bias"])        # still the column sums of dx
    fw, bw = _reference(inp._replace(lin_bias=None), G, n, F, 1, out["y"])
    _assert_within_bounds(out, fw, bw, n, f"null-lin-bias-G{G}-n{n}-F{F}")


def test_bad_arguments_are_refused_before_any_launch(lib, dev):
    """n = 1, G = 0, F = 0, a negative or NaN eps, z / y / save_mean NULL (and the backward's counterparts) -> IAS_ERR_ARG,
    and nothing was launched: every output still holds its sentinel, the running statistics and the counter what they held."""
    G, n, F = 2, 20, 65
    inp = bm.make_inputs(G, n, F, True, seed=5)
    run = Run(dev, inp, G, n, F)
    nan = float("nan")
    for kw in (dict(n=1), dict(G=0), dict(F=0), dict(G=-1), dict(eps=-1e-5), dict(eps=nan), dict(null=("z",)), dict(null=("y",)),
               dict(null=("save_mean",)), dict(null=("save_invstd",))):
        assert run.forward(lib, 1, **kw) == -1, kw
    for kw in (dict(n=1), dict(G=0), dict(F=0), dict(null=("z",)), dict(null=("dy",)), dict(null=("dx",)),
               dict(null=("save_mean",)), dict(null=("save_invstd",))):
        assert run.backward(lib, 1, **kw) == -1, kw
    torch.cuda.synchronize()
    for k in ("y", "save_mean", "save_invstd", "dx", "gw", "gb", "g_lin_bias"):
        assert getattr(run, k).untouched(), k
    out = run.out()
    assert torch.equal(out["running_mean"], inp.running_mean) and torch.equal(out["running_var"], inp.running_var)
    assert int(out["nbt"]) == bm.NBT_START
    assert run.guards_intact()


@pytest.mark.parametrize("G,n,F", [(2, 128, 130), (3, 100, 65), (2, 200, 65), (4, 300, 130)])
def test_two_calls_give_the_same_bits(lib, dev, G, n, F):
    inp = bm.make_inputs(G, n, F, True, seed=6)
    _, a = _both(lib, dev, inp, G, n, F, 1)
    _, b = _both(lib, dev, inp, G, n, F, 1)
    _same_bits(a, b, a.keys(), "determinism")


@pytest.mark.parametrize("G,n,F", [(2, 128, 65), (4, 20, 130), (3, 128, 65), (2, 129, 64), (3, 300, 65)])
def test_stacked_groups_against_separate_calls(lib, dev, G, n, F):
    """One call with G groups against G calls with one group, chained through the running statistics and the counter.
    Backward (the same instantiation, the same order; fed the stacked forward's statistics): the same bits in dx, and in
    gw / gb / g_lin_bias after adding the separate results in group order in fp32.  Forward: both within the bounds of
    the fp64 model; whether they are bit-equal as well is printed (an even G at n <= 128 runs two groups per pass,
    another instantiation)."""
    inp = bm.make_inputs(G, n, F, True, seed=7)
    stacked, out = _both(lib, dev, inp, G, n, F, 1)
    parts, first = [], None
    for g in range(G):
        rows = slice(g * n, (g + 1) * n)
        one = Run(dev, inp._replace(z=inp.z[rows], dy=inp.dy[rows]), 1, n, F, share=first)
        first = first or one
        assert one.forward(lib, 1) == 0
        stats = (stacked.save_mean.t[g].contiguous(), stacked.save_invstd.t[g].contiguous())
        assert one.backward(lib, 1, stats=stats) == 0
        assert one.guards_intact()
        parts.append(one.out())
    sep = {k: torch.cat([p[k] for p in parts], 0) for k in ("y", "dx", "save_mean", "save_invstd")}
    sep.update({k: parts[-1][k] for k in ("running_mean", "running_var", "nbt")})
    for k in ("gw", "gb", "g_lin_bias"):
        acc = torch.zeros(F)
        for p in parts:
            acc = acc + p[k]
        sep[k] = acc
    equal = {k: torch.equal(sep[k], out[k]) for k in ("y", "save_mean", "save_invstd", "running_mean", "running_var")}
    print("BN1D-STACKED", (G, n, F), "forward bit-equal to separate calls:", equal)
    assert int(sep["nbt"]) == int(out["nbt"]) == bm.NBT_START + G
    fw, bw = _reference(inp, G, n, F, 1, out["y"])
    _assert_within_bounds(out, fw, bw, n, f"stacked-G{G}-n{n}-F{F}")
    _same_bits(sep, out, ("dx", "gw", "gb", "g_lin_bias"), "stacked backward")
    fw_sep = {k: sep[k] for k in ("y", "save_mean", "save_invstd", "running_mean", "running_var")}
    _assert_within_bounds(fw_sep, fw, bw, n, f"separate-G{G}-n{n}-F{F}")


@pytest.mark.parametrize("G,n,F", [(2, 20, 65), (3, 200, 130), (1, 300, 63), (2, 3, 1)])
def test_constant_columns(lib, dev, G, n, F):
    """Every row of a group equal (eps 1e-5): the variance is exactly zero, so y is relu(bias) exactly, dx is finite, the
    running variance moves toward zero by the momentum; no NaN anywhere."""
    inp = bm.make_inputs(G, n, F, True, seed=8)
    z = inp.z.view(G, n, F)[:, :1].expand(G, n, F).reshape(G * n, F).contiguous()      # every group its own constant row
    inp = inp._replace(z=z)
    _, out = _both(lib, dev, inp, G, n, F, 1)
    for k, v in out.items():
        assert bool(torch.isfinite(v.double()).all()), k
    assert torch.equal(out["y"], torch.clamp_min(inp.bias, 0.0).expand(G * n, F))
    x = z.view(G, n, F)[:, 0] + inp.lin_bias
    assert torch.equal(out["save_mean"], x)
    want_var = inp.running_var.double() * (1.0 - bm.MOMENTUM) ** G
    assert (out["running_var"].double() - want_var).abs().max().item() <= 1e-5 * max(1.0, want_var.max().item())
    assert bool((out["running_var"] < inp.running_var).all())
    fw, bw = _reference(inp, G, n, F, 1, out["y"])
    _assert_within_bounds(out, fw, bw, n, f"constant-G{G}-n{n}-F{F}")


# ---- the Python gates in front of the kernels ----------------------------------------------------------------------------
def _projector(d0, d1, d2, dev, lin_bias=True, **bn):
    torch.manual_seed(5)
    return torch.nn.Sequential(torch.nn.Linear(d0, d1, bias=lin_bias), torch.nn.BatchNorm1d(d1, **bn), torch.nn.ReLU(True),
                               torch.nn.Linear(d1, d2, bias=False)).to(dev)


def _pair_and_reference(proj, a, b):
    """project_pair on `proj` and two calls of a deep copy, one training step each; -> outputs and modules."""
    from inverse_audio_synthesis_amd import vicreg
    ref = copy.deepcopy(proj)
    xa, xb = vicreg.project_pair(proj, a, b)
    ra, rb = ref(a), ref(b)
    return (xa, xb), (ra, rb), ref


GATES = {"eval": {}, "momentum_none": dict(momentum=None), "affine_false": dict(affine=False),
         "no_running_stats": dict(track_running_stats=False), "fp64": {}}


@pytest.mark.parametrize("gate", list(GATES))
def test_gates_fall_back_to_torch(lib, dev, gate, monkeypatch):
    """What the kernels do not implement goes to nn.BatchNorm1d and gives what two projector calls / norm(lin(x)) give; the
    C entry is not called (it would refuse or, worse, train an eval-mode module)."""
    from inverse_audio_synthesis_amd import paramembed, vicreg
    called = []
    real = lib.ias_bn1d_groups_forward
    monkeypatch.setattr(lib, "ias_bn1d_groups_forward", lambda *a: (called.append(1), real(*a))[1])
    n, d0, d1, d2 = 12, 10, 65, 6
    proj = _projector(d0, d1, d2, dev, **GATES[gate])
    dt = torch.float64 if gate == "fp64" else torch.float32
    proj = proj.to(dt)
    if gate == "eval":
        proj.eval()
    a, b = randn((n, d0), 1).to(dev, dt).requires_grad_(True), randn((n, d0), 2).to(dev, dt).requires_grad_(True)
    got, want, ref = _pair_and_reference(proj, a, b)
    for g, w in zip(got, want):          # (one GEMM on the stacked rows against two: the bounds of the fused path's own test)
        assert (g - w).abs().max().item() <= 2e-5 * max(1.0, w.abs().max().item())
    gg = torch.autograd.grad(got[0].sum() + (got[1] ** 2).sum(), [a, b] + list(proj.parameters()))
    gw = torch.autograd.grad(want[0].sum() + (want[1] ** 2).sum(), [a, b] + list(ref.parameters()))
    for g, w in zip(gg, gw):
        assert (g - w).abs().max().item() <= 2e-4 * max(1.0, w.abs().max().item())
    assert list(proj.state_dict()) == list(ref.state_dict())
    for (k, s), (_, r) in zip(proj.state_dict().items(), ref.state_dict().items()):
        assert torch.allclose(s.double(), r.double(), rtol=1e-5, atol=1e-6), k
    lin, norm = proj[0], proj[1]
    x = a.detach()
    y, r = paramembed.linear_norm(lin, norm, x), copy.deepcopy(norm)(lin(x))
    assert (y - r).abs().max().item() <= 2e-5 * max(1.0, r.abs().max().item())
    assert not called


def test_one_row_in_training_raises_torchs_error(lib, dev):
    from inverse_audio_synthesis_amd import paramembed, vicreg
    proj = _projector(10, 65, 6, dev)
    a, b = randn((1, 10), 1).to(dev), randn((1, 10), 2).to(dev)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        vicreg.project_pair(proj, a, b)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        paramembed.linear_norm(proj[0], proj[1], a)


def test_linear_without_bias_in_front(lib, dev):
    """Linear(bias=False) -> BatchNorm1d -> ReLU: the same output as the biased form with a zero bias (same bits: NULL and
    0.0f add the same), its input gradient too, and no gradient for a bias that does not exist."""
    from inverse_audio_synthesis_amd import vicreg
    n, d0, d1, d2 = 20, 10, 65, 6
    nobias, biased = _projector(d0, d1, d2, dev, lin_bias=False), _projector(d0, d1, d2, dev, lin_bias=True)
    with torch.no_grad():
        biased[0].weight.copy_(nobias[0].weight); biased[0].bias.zero_(); biased[3].weight.copy_(nobias[3].weight)
    a, b = randn((n, d0), 1).to(dev).requires_grad_(True), randn((n, d0), 2).to(dev).requires_grad_(True)
    xa, xb = vicreg.project_pair(nobias, a, b)
    ya, yb = vicreg.project_pair(biased, a, b)
    assert torch.equal(xa, ya) and torch.equal(xb, yb)
    assert nobias[0].bias is None
    g0 = torch.autograd.grad(xa.sum() + (xb ** 2).sum(), [a, b] + list(nobias.parameters()))
    g1 = torch.autograd.grad(ya.sum() + (yb ** 2).sum(), [a, b] + list(biased.parameters()))
    names1 = [k for k, _ in biased.named_parameters()]
    g1 = {k: g for k, g in zip(["a", "b"] + names1, g1)}
    for k, g in zip(["a", "b"] + [k for k, _ in nobias.named_parameters()], g0):
        assert torch.equal(g, g1[k]), k
    assert int(nobias[1].num_batches_tracked) == 2


def test_upstream_gradients_that_are_not_contiguous(lib, dev):
    """y.sum() (an expanded scalar: every stride 0) and a consumer of y.t() (a transposed cotangent) give the gradients of
    the contiguous cotangent with the same values."""
    from inverse_audio_synthesis_amd import paramembed
    n, d0, d1 = 20, 10, 65
    proj = _projector(d0, d1, 6, dev)
    lin, norm = proj[0], proj[1]
    x = randn((n, d0), 1).to(dev)
    wts = randn((d1, n), 2).to(dev)                                   # multiplies y.t()
    for strided, contiguous in ((lambda y: y.sum(), lambda y: (y * torch.ones_like(y)).sum()),
                                (lambda y: (y.t() * wts).sum(), lambda y: (y * wts.t().contiguous()).sum())):
        res = []
        for f in (strided, contiguous):
            nm = copy.deepcopy(norm)
            y = paramembed.linear_norm(lin, nm, x)
            res.append(torch.autograd.grad(f(y), [lin.weight, lin.bias, nm.weight, nm.bias]))
        for g, w in zip(*res):
            assert torch.equal(g, w)

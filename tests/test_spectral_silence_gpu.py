"""The linear-bin spectral losses on silence, faint noise and clamped bins, against the oracle in fp64.

Every other GPU test of MultiResolutionSTFTLoss, STFTL1, STFTPlan.values(VALUE_MAG_CLAMPED), ias_mrstft_rows and the span /
frames / tables = NULL backward entries feeds them full-scale white noise: no bin comes near eps = 1e-8, none is exactly 0.
These rows (spectral_inputs.SILENCE_ROWS: loud noise, noise of standard deviation 2e-7, exact zeros, and one row of tones
over a noise floor; T = 12001) run the clamp sqrt(max(|X|^2, eps)) of the forward kernels, `live = v > sqrt(eps)` of the
four MR-STFT backward kernels, `live = pv > 0` of the power-1 L1 backward, sg == 0 at V == T and the den > 0 guard of the
coefficient kernels.  test_spectral_silence_cpu.py proves what the comparison needs of the inputs (no power value within
a factor 4 of eps, no V within rounding of T) and that the oracle's own fp32 evaluation is ten times inside every bar.

Bars, the project's own, applied PER ROW (a loud row must not carry a wrong quiet one): 1e-3 relative for every sum and
loss, 2e-3 relative L2 for every gradient over the row, its first and its last n_fft / 2 samples, 1e-4 of a frame's own
maximum for values.  Exact where the mathematics is exact: clamped frames hold one bit pattern, silent frames are 0, the
sums and losses of `identical` and `both_silent` are 0, the gradient of an all-clamped prediction is 0, and so is the
gradient on the samples that only all-quiet frames read.  The gradient of `identical` is only required to be finite: at
V == T any sign is a subgradient, and the backward kernels recompute V with another FFT than the one that made T.

Resolution sets: each auraloss default alone (1024/120/600, 2048/240/1200, 512/50/240), the default triple, and the odd-hop
pair of test_match_mrstft_gpu.ODD (no span plan: frames fallback); gradients on the fused span path, with
fused_combine = False, and on the fallback.

Measured on an MI355X (worst over rows, resolution sets and paths):
  values     clamped bins hold 9.999999747378752e-05 at all three sizes; other frames within 4.64e-07 of their maximum
  sums       per row 1.33e-07 / 1.82e-07 / 7.03e-08 (sum (T - V)^2, sum T^2, log term); fused batch 9.99e-08
  losses     per row 9.93e-08, batch 7.80e-08
  gradients  per_item 1.83e-04 (span and unfused; 2048), 4.24e-04 (odd-hop frames fallback); forward 1.84e-04 / 4.26e-04;
             tables = NULL 2.31e-04 (1024/120/600), 5.54e-05 (512/125/512)
             |g| of `identical` 1.8e-02 .. 1.4e+00 beside 7.4e-02 .. 1.3e+00 of the same row against mid_gap's target
  L1         STFTL1 / mel loss 9.02e-08, gradient 1.43e-05 (2048/512, power 1), otherwise <= 2e-07
With `live = v > a.eps` in stft_grad_wave_kernel ten of the per_item / forward gradient tests fail (1024, defaults, oddhop),
while test_spectral_grad_gpu.py and test_match_mrstft_gpu.py pass."""
import pytest
import torch

from oracle import spectral_oracle as spo
import spectral_inputs as si
from spectral_inputs import EPS

pytestmark = pytest.mark.gpu
VALUE_BAR, LOSS_BAR, GRAD_BAR = 1e-4, 1e-3, 2e-3
NAMES = list(si.SILENCE_ROWS)
IDX = {n: i for i, n in enumerate(NAMES)}
ZERO_GRAD = ("pred_silent", "pred_faint", "both_silent")          # every bin of the prediction clamped
QUIET_STRETCH = ("mid_gap", "faint_gap", "faint_vs_loud", "identical")
# two sets of row cotangents: each has a 0 (that row's gradient is exactly 0) and non-unit values; every row is compared
# against the oracle under at least one non-zero cotangent
COTANGENTS = ([0.7, 1.9, 0.25, 1.0, 0.5, 1.3, 0.6, 2.0, 0.8, 0.0], [0.0, 0.4, 1.0, 2.5, 1.0, 0.9, 1.1, 0.3, 1.7, 0.6])
# (resolution set, fused_combine)
PATHS = [("1024", True), ("1024", False), ("2048", True), ("2048", False), ("512", True), ("512", False),
         ("defaults", True), ("defaults", False), ("oddhop", True)]
PATH_IDS = [f"{k}-{'span' if f else 'unfused'}" if k != "oddhop" else "oddhop-frames" for k, f in PATHS]


def _rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else (0.0 if a == 0 else float("inf"))


def _batch():
    return si.silence_batch(NAMES)


def _module(key, dev, fused=True):
    from inverse_audio_synthesis_amd.spectral import MultiResolutionSTFTLoss
    m = MultiResolutionSTFTLoss(eps=EPS, **si.RESOLUTION_SETS[key]).to(dev)
    m.fused_combine = fused
    return m


def _check_row_grad(tag, name, g, ref, n_fft, res=None, shrink=0):
    """One row's gradient against its fp64 reference; -> the worst ratio (0.0 for the rows judged exactly).  The samples
    that only all-quiet frames read are exactly 0 (``shrink``: that range less so many samples at either end)."""
    assert torch.isfinite(g).all(), (tag, name)
    if res is not None and name in QUIET_STRETCH:
        lo, hi = si.untouched_range_of(name, res)
        lo, hi = lo + shrink, hi - shrink
        assert torch.count_nonzero(g[lo:hi]).item() == 0, (tag, name, "samples that only all-quiet frames read")
    if name in ZERO_GRAD:
        assert torch.count_nonzero(g).item() == 0, (tag, name)
        return 0.0
    if name == "identical":
        return 0.0                     # finite (above): any sign at V == T is a subgradient, nothing more is asserted
    r = si.row_ratios(g, ref, n_fft)
    for k, v in r.items():
        assert v <= GRAD_BAR, (tag, name, k, v)
    return max(r.values())


# ---------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("n_fft,hop,win", [(512, 50, 240), (1024, 120, 600), (2048, 240, 1200)])
def test_values(lib, dev, n_fft, hop, win):
    from inverse_audio_synthesis_amd.spectral import STFTPlan, VALUE_MAG, VALUE_MAG_CLAMPED, VALUE_POWER
    plan = STFTPlan(n_fft, win, hop).to(dev)
    patterns, worst, seen = set(), 0.0, [False] * 3
    for batch in _batch():
        p64 = si.stft_power(batch.double(), n_fft, hop, win).transpose(1, 2)          # [B, frames, bins]
        quiet = p64.amax(dim=2) < EPS / 4              # every bin clamped (the dead zone: nothing in [eps / 4, 4 eps])
        silent = p64.amax(dim=2) == 0
        seen = [a or bool(b.any()) for a, b in zip(seen, (silent, quiet & ~silent, ~quiet))]
        out = plan.values(batch.to(dev), VALUE_MAG_CLAMPED, EPS).cpu()
        assert out.shape == p64.shape and torch.isfinite(out).all()
        patterns |= set(out[quiet].view(torch.int32).unique().tolist())
        for mode, ref, frames in ((VALUE_MAG_CLAMPED, p64.clamp(min=EPS).sqrt(), ~quiet), (VALUE_MAG, p64.sqrt(), ~silent),
                                  (VALUE_POWER, p64, ~silent)):
            o = out if mode == VALUE_MAG_CLAMPED else plan.values(batch.to(dev), mode).cpu()
            assert torch.isfinite(o).all()
            if mode != VALUE_MAG_CLAMPED:
                assert torch.count_nonzero(o[silent]).item() == 0, mode
            ratio = ((o.double() - ref).abs().amax(dim=2) / ref.amax(dim=2))[frames].max().item()
            worst = max(worst, ratio)
            assert ratio <= VALUE_BAR, (mode, ratio)
    assert all(seen)                                   # silent, faint and live frames
    assert len(patterns) == 1, patterns
    c = torch.tensor(list(patterns), dtype=torch.int32).view(torch.float32).item()
    print(f"values {n_fft}/{hop}/{win}: clamped bins hold {c!r}; other frames within {worst:.2e} of their maximum")
    assert abs(c - 1e-4) <= 1e-6 * 1e-4


# ------------------------------------------------------------------------------------------------- sums and losses
@pytest.mark.parametrize("n_fft,hop,win", si.ALL_RESOLUTIONS, ids=lambda v: str(v))
def test_row_sums(lib, dev, n_fft, hop, win):
    """ias_mrstft_rows per row and the fused ias_stft loss sums of the batch, each of the three sums on its own."""
    from inverse_audio_synthesis_amd.spectral import LOSS_MRSTFT, STFTPlan, VALUE_MAG_CLAMPED
    plan = STFTPlan(n_fft, win, hop).to(dev)
    x, y = _batch()
    ref = si.mrstft_sums(x.double(), y.double(), n_fft, hop, win)
    tv = plan.values(y.to(dev), VALUE_MAG_CLAMPED, EPS)
    vv = plan.values(x.to(dev), VALUE_MAG_CLAMPED, EPS)
    got = plan.mrstft_rows(vv, tv).cpu()
    assert got.shape == ref.shape and got.dtype == torch.float64
    worst = [0.0, 0.0, 0.0]
    for name, b in IDX.items():
        for j in range(3):
            r = _rel(got[b, j].item(), ref[b, j].item())
            worst[j] = max(worst[j], r)
            assert r <= LOSS_BAR, (name, j, got[b, j].item(), ref[b, j].item())
    for name in ("identical", "both_silent"):
        assert got[IDX[name]].tolist()[0] == 0.0 and got[IDX[name]].tolist()[2] == 0.0, (name, got[IDX[name]])
        assert ref[IDX[name], 0].item() == 0.0 and ref[IDX[name], 2].item() == 0.0
    # a silent target is count * c^2: 16 fp32 products per thread (2^-24 each), then fp64
    c = tv[IDX["tgt_silent"]].flatten()[0].item()
    count = tv[0].numel()
    assert torch.count_nonzero(tv[IDX["tgt_silent"]] - c).item() == 0
    assert abs(got[IDX["tgt_silent"], 1].item() - count * c * c) <= 1e-6 * count * c * c
    fused = plan.loss_sums(x.to(dev), tv, VALUE_MAG_CLAMPED, LOSS_MRSTFT, EPS).cpu()
    total = ref.sum(dim=0)
    rf = [_rel(fused[j].item(), total[j].item()) for j in range(3)]
    print(f"sums {n_fft}/{hop}/{win}: per row {worst[0]:.2e} {worst[1]:.2e} {worst[2]:.2e}; fused batch "
          f"{rf[0]:.2e} {rf[1]:.2e} {rf[2]:.2e}")
    assert max(rf) <= LOSS_BAR, rf


@pytest.mark.parametrize("key", list(si.RESOLUTION_SETS))
def test_losses(lib, dev, key):
    res = si.RESOLUTION_SETS[key]
    m = _module(key, dev)
    x, y = _batch()
    xd, yd = x.to(dev), y.to(dev)
    got = m.per_item(xd, yd)
    assert got.shape == (len(NAMES),) and torch.isfinite(got).all()
    assert torch.equal(m.per_item(xd, targets=m.target(yd)), got)
    worst = 0.0
    for name, b in IDX.items():
        ref = si.silence_ref(name, res).loss
        one = m(xd[b:b + 1].contiguous(), yd[b:b + 1].contiguous())
        assert torch.equal(m(xd[b:b + 1].contiguous(), targets=m.target(yd[b:b + 1].contiguous())), one)
        for what, v in (("per_item", got[b].item()), ("forward", one.item())):
            worst = max(worst, _rel(v, ref))
            assert _rel(v, ref) <= LOSS_BAR, (name, what, v, ref)
        if name in ("identical", "both_silent"):
            assert ref == 0.0 and got[b].item() == 0.0 and one.item() == 0.0
    whole = m(xd, yd)
    assert torch.equal(m(xd, targets=m.target(yd)), whole)
    ref = spo.mrstft_loss(x.double(), y.double(), eps=EPS, **res)[0].item()
    print(f"losses {key}: per row {worst:.2e}, batch {_rel(whole.item(), ref):.2e}")
    assert _rel(whole.item(), ref) <= LOSS_BAR, (whole.item(), ref)


# --------------------------------------------------------------------------------------------------------- gradients
def _per_item_grad(m, x, y, cot, dev):
    xa = x.to(dev).requires_grad_(True)
    per = m.per_item(xa, y.to(dev))
    per.backward(torch.tensor(cot, dtype=torch.float32, device=dev))
    return per.detach().cpu(), xa.grad.detach().cpu()


@pytest.mark.parametrize("key,fused", PATHS, ids=PATH_IDS)
def test_per_item_gradient(lib, dev, key, fused):
    res = si.RESOLUTION_SETS[key]
    n_fft = max(res["fft_sizes"])
    m = _module(key, dev, fused)
    x, y = _batch()
    worst = 0.0
    for cot in COTANGENTS:
        _loss, g = _per_item_grad(m, x, y, cot, dev)
        for name, b in IDX.items():
            if cot[b] == 0.0:
                assert torch.count_nonzero(g[b]).item() == 0, name
                continue
            r = _check_row_grad(f"per_item {key}", name, g[b], cot[b] * si.silence_ref(name, res).grad, n_fft, res)
            worst = max(worst, r)
    # `identical` next to the same prediction against another target
    b = IDX["identical"]
    other = y[IDX["mid_gap"]:IDX["mid_gap"] + 1]
    _l, go = _per_item_grad(m, x[b:b + 1], other, [1.0], dev)
    _l, gi = _per_item_grad(m, x[b:b + 1], y[b:b + 1], [1.0], dev)
    print(f"per_item gradient {key} {'fused' if fused else 'unfused'}: worst row / head / tail {worst:.2e}; |g| of identical "
          f"{gi.double().norm().item():.3e}, of the same row against mid_gap's target {go.double().norm().item():.3e}")
    assert torch.isfinite(gi).all() and torch.isfinite(go).all()


_BATCH_REFS = {}


def _batch_ref(key, names):
    """fp64 gradient of the batch loss (shared coefficients) of the given rows."""
    k = (key, tuple(names))
    if k not in _BATCH_REFS:
        x, y = si.silence_batch(names)
        a = x.double().requires_grad_(True)
        loss = spo.mrstft_loss(a, y.double(), eps=EPS, **si.RESOLUTION_SETS[key])[0]
        (g,) = torch.autograd.grad(loss, a)
        _BATCH_REFS[k] = (loss.item(), g)
    return _BATCH_REFS[k]


@pytest.mark.parametrize("key,fused", PATHS, ids=PATH_IDS)
def test_forward_gradient(lib, dev, key, fused):
    """The batch loss (one coefficient pair for all rows): the batch without tgt_silent, whose gradient of size 1e3 would
    set the scale, then tgt_silent alone."""
    res = si.RESOLUTION_SETS[key]
    n_fft = max(res["fft_sizes"])
    m = _module(key, dev, fused)
    worst = 0.0
    for names in ([n for n in NAMES if n != "tgt_silent"], ["tgt_silent"]):
        x, y = si.silence_batch(names)
        ref_loss, ref = _batch_ref(key, names)
        xa = x.to(dev).requires_grad_(True)
        loss = m(xa, y.to(dev))
        assert _rel(loss.item(), ref_loss) <= LOSS_BAR, (names, loss.item(), ref_loss)
        (2.0 * loss).backward()
        g = xa.grad.cpu() / 2.0
        for b, name in enumerate(names):
            worst = max(worst, _check_row_grad(f"forward {key}", name, g[b], ref[b], n_fft, res))
    print(f"forward gradient {key} {'fused' if fused else 'unfused'}: worst row / head / tail {worst:.2e}")


@pytest.mark.parametrize("n_fft,hop,win", [(1024, 120, 600), (512, 125, 512)])
def test_backward_entry_without_tables(lib, dev, n_fft, hop, win):
    """ias_stft_loss_backward_mrstft_rows with tables = NULL: the workgroup-per-frame-pair kernel of
    csrc/spectral_grad_kernels.hip, on the gapped and faint rows.  It transforms frames 2 p and 2 p + 1 as the real and
    imaginary part of one complex FFT, forward and inverse, so a quiet frame whose partner is not quiet receives the
    partner's rounding (measured: 1e-10 beside gradients of 1e-3).  That can be the first and the last all-quiet frame of
    a stretch: exact zeros are asserted on the samples that neither of them reads (one hop less at either end), where
    every frame and its partner is quiet; the bars hold everywhere."""
    from inverse_audio_synthesis_amd import _lib
    from inverse_audio_synthesis_amd.spectral import STFTPlan, VALUE_MAG_CLAMPED
    names = list(si.GAPPED) + ["pred_faint"]
    cot = [0.7, 1.9, 0.25, 1.0, 0.5, 1.3]
    res = dict(fft_sizes=(n_fft,), hop_sizes=(hop,), win_lengths=(win,))
    plan = STFTPlan(n_fft, win, hop).to(dev)
    x, y = si.silence_batch(names)
    xd = x.to(dev)
    B = len(names)
    tgt = plan.values(y.to(dev), VALUE_MAG_CLAMPED, EPS)
    sums = plan.mrstft_rows(plan.values(xd, VALUE_MAG_CLAMPED, EPS), tgt)
    g = torch.tensor(cot, dtype=torch.float32, device=dev)
    coef = torch.empty((B, 2), dtype=torch.float64, device=dev)
    _lib.check(lib.ias_mrstft_coef_rows(_lib.ptr(sums), _lib.ptr(g), float(tgt[0].numel()), 1, B, _lib.ptr(coef),
                                        _lib.stream()), "ias_mrstft_coef_rows")
    assert coef[names.index("identical"), 0].item() == 0.0            # den == 0
    frame_grad = torch.empty((B, plan.num_frames(si.SILENCE_T), n_fft), dtype=torch.float32, device=dev)
    out = torch.empty_like(xd)
    _lib.check(lib.ias_stft_loss_backward_mrstft_rows(
        _lib.ptr(xd), _lib.ptr(plan.window), None, _lib.ptr(tgt), _lib.ptr(coef), _lib.ptr(frame_grad), _lib.ptr(out), B,
        si.SILENCE_T, n_fft, hop, plan.n_out, EPS, _lib.stream()), "ias_stft_loss_backward_mrstft_rows")
    out = out.cpu()
    worst = 0.0
    for b, name in enumerate(names):
        worst = max(worst, _check_row_grad("tables = NULL", name, out[b], cot[b] * si.silence_ref(name, res).grad, n_fft,
                                           res, shrink=hop))
    print(f"tables = NULL {n_fft}/{hop}/{win}: worst row / head / tail {worst:.2e}")


@pytest.mark.parametrize("key", ["defaults", "oddhop"])
def test_a_row_does_not_depend_on_its_neighbours(lib, dev, key):
    """Loss and gradient of mid_gap and faint_gap: the same bits alone, between two silent rows and between two loud
    rows, with the resolutions on side streams or not."""
    m = _module(key, dev)
    for name in ("mid_gap", "faint_gap"):
        base = None
        for parallel in (True, False):
            m.parallel = parallel
            for left, right in ((None, None), ("both_silent", "both_silent"), ("tgt_silent", "tones_floor")):
                names = [name] if left is None else [left, name, right]
                x, y = si.silence_batch(names)
                loss, g = _per_item_grad(m, x, y, [1.0] * len(names), dev)
                mine = (loss[len(names) // 2], g[len(names) // 2])
                if base is None:
                    base = mine
                assert torch.equal(mine[0], base[0]) and torch.equal(mine[1], base[1]), (name, parallel, left)


# ---------------------------------------------------------------------------------------------------------- L1 losses
@pytest.mark.parametrize("kind,case", si.L1_KINDS, ids=lambda v: str(v))
def test_l1_losses(lib, dev, kind, case):
    """STFTL1 at power 1 (`live = pv > 0` stands between a silent bin and 0 * inf) and power 2, and the default
    MelSpectrogramL1, on the gapped rows and a silent prediction."""
    from inverse_audio_synthesis_amd.spectral import MelSpectrogramL1, STFTL1
    names = list(si.L1_ROWS)
    n_fft, hop, power = case
    m = (STFTL1(n_fft=n_fft, hop_length=hop, power=power) if kind == "stft" else MelSpectrogramL1()).to(dev)
    x, y = si.silence_batch(names)
    xa = x.to(dev).requires_grad_(True)
    per = m.per_item(xa, y.to(dev))
    per.sum().backward()
    g, per = xa.grad.cpu(), per.detach().cpu()
    assert torch.isfinite(g).all() and torch.isfinite(per).all()
    worst_l = worst_g = 0.0
    for b, name in enumerate(names):
        ref_loss, ref = si.l1_ref(kind, name, case)
        worst_l = max(worst_l, _rel(per[b].item(), ref_loss))
        assert _rel(per[b].item(), ref_loss) <= LOSS_BAR, (name, per[b].item(), ref_loss)
        if name == "pred_silent":
            assert torch.count_nonzero(g[b]).item() == 0
            continue
        if name in ("mid_gap", "faint_gap"):
            lo, hi = si.untouched_range(*si.quiet_region(name), n_fft, hop)
            if name == "mid_gap":          # silence: exactly 0 (faint noise has a gradient of its own)
                assert torch.count_nonzero(g[b, lo:hi]).item() == 0
        r = si.row_ratios(g[b], ref, n_fft)
        worst_g = max(worst_g, max(r.values()))
        for k, v in r.items():
            assert v <= GRAD_BAR, (name, k, v)
    # the batch form (one cotangent) on the same rows
    xb = x.to(dev).requires_grad_(True)
    loss = m(xb, y.to(dev))
    loss.backward()
    gb = xb.grad.cpu()
    ref_batch = sum(si.l1_ref(kind, n, case)[0] for n in names) / len(names)
    assert _rel(loss.item(), ref_batch) <= LOSS_BAR
    assert torch.isfinite(gb).all() and torch.count_nonzero(gb[names.index("pred_silent")]).item() == 0
    for b, name in enumerate(names):
        if name != "pred_silent":
            r = si.row_ratios(gb[b] * len(names), si.l1_ref(kind, name, case)[1], n_fft)
            worst_g = max(worst_g, max(r.values()))
            assert max(r.values()) <= GRAD_BAR, (name, r)
    print(f"L1 {kind} {case}: loss {worst_l:.2e}, gradient {worst_g:.2e}")

"""The ground that test_spectral_silence_gpu.py stands on, checked without a GPU: conditions on the committed inputs
(spectral_inputs.SILENCE_ROWS) and on the oracle, so that a bar that fails on the GPU is not the inputs' or the
reference's doing.  Edit a seed or a boundary into a trap and one of these fails.

1. Dead zone: no fp64 power value |X|^2 of any row (prediction or target) at any resolution lies in [eps / 4, 4 eps].
   A bin within rounding of eps is live in one precision and clamped in the other, and with 1 / V ~ 1e4 it then carries
   the gradient.  If this fails, change a boundary or a seed, never the interval.
2. Sign margin: no bin has V and T within spectral_inputs.SIGN_MARGIN of the frame's norm of each other (unless both are
   clamped, or the row is `identical`): the gradient carries sign(V - T), see sign_margin_violations.
3. Not vacuous: the share of clamped bins, and of bins that are non-zero yet below eps / 4, per row and resolution, in the
   fp64 oracle and in the fp32 oracle's own STFT (faint noise must not flush to zero in fp32).
4. The oracle evaluated in fp32 stays within ONE TENTH of every bar of the GPU test against the oracle in fp64: the three
   per-row sums and the per-row loss at 1e-3, the per-row gradient at 2e-3 relative L2 over the row, its first and its
   last n_fft / 2 samples; where the fp64 gradient is exactly 0 the fp32 one is too.  Measured here: sums <= 2.5e-7,
   losses <= 1.9e-5 (tgt_silent), gradients <= 1.3e-4 (tones_floor; every other row <= 6.7e-5); STFTL1 and mel L1 on
   their rows: losses <= 2e-7, gradients <= 2e-5.
5. The exact facts the GPU test asserts: loss and gradient of `identical` and `both_silent` are exactly 0, the gradient
   of `pred_silent` and `pred_faint` is exactly 0, the gradient of a row with a quiet stretch is exactly 0 on
   spectral_inputs.untouched_range_of (the samples that only all-quiet frames read) and is not 0 just outside it.

Shares measured here (prediction; share of clamped bins, lowest .. highest over the five resolutions; in the rows with
faint noise the non-zero bins below eps / 4 are the same share to three digits, elsewhere at most 1e-4):
  mid_gap 0.29-0.39    lead_tail 0.36-0.44    faint_gap 0.31-0.39    faint_vs_loud 0.31-0.39    identical 0.28-0.36
  pred_faint 1 (all non-zero)    pred_silent, both_silent 1 (all zero)    tgt_silent, tones_floor 0"""
import pytest
import torch

import spectral_inputs as si
from spectral_inputs import EPS

LOSS_BAR, GRAD_BAR = 1e-3, 2e-3
NAMES = list(si.SILENCE_ROWS)
ALL_CLAMPED = ("pred_silent", "pred_faint", "both_silent")
NONE_CLAMPED = ("tgt_silent", "tones_floor")
QUIET_STRETCH = ("mid_gap", "faint_gap", "faint_vs_loud", "identical")     # one quiet region away from both ends


def test_the_row_table_is_the_issue_s():
    assert NAMES == ["mid_gap", "lead_tail", "faint_gap", "faint_vs_loud", "tgt_silent", "pred_silent", "pred_faint",
                     "identical", "both_silent", "tones_floor"]
    assert si.SILENCE_T == 12001 and all(si.SILENCE_T % h for _n, h, _w in si.ALL_RESOLUTIONS)
    assert set(si.GAPPED) | set(ALL_CLAMPED) | set(NONE_CLAMPED) == set(NAMES)
    x, y = si.silence_pair("identical")
    assert torch.equal(x, y)
    assert si.SILENCE_ROWS["faint_gap"][0][1][0][1] == si.SILENCE_ROWS["faint_gap"][1][1][0][1]      # same boundaries
    assert si.SILENCE_ROWS["faint_gap"][0][1][1][1] == si.SILENCE_ROWS["faint_gap"][1][1][1][1]


@pytest.mark.parametrize("name", NAMES)
def test_dead_zone_and_sign_margin(name):
    x, y = si.silence_pair(name)
    for n_fft, hop, win in si.ALL_RESOLUTIONS:
        px, py = (si.stft_power(v.double()[None], n_fft, hop, win) for v in (x, y))
        for who, p in (("prediction", px), ("target", py)):
            near = ((p >= EPS / 4) & (p <= 4 * EPS)).sum().item()
            assert near == 0, (name, who, (n_fft, hop, win), near)
        if name != "identical":
            assert si.sign_margin_violations(px, py, n_fft, EPS) == 0, (name, (n_fft, hop, win))
    if name in si.L1_ROWS:
        for n_fft, hop, power in si.STFT_L1_CASES:
            px, py = (si.stft_power(v.double()[None], n_fft, hop, n_fft) for v in (x, y))
            assert si.sign_margin_violations(px, py, n_fft, None, power) == 0, (name, (n_fft, hop, power))


@pytest.mark.parametrize("name", NAMES)
def test_clamped_shares(name):
    x, _y = si.silence_pair(name)
    for n_fft, hop, win in si.ALL_RESOLUTIONS:
        shares = []
        for dtype in (torch.float64, torch.float32):
            p = si.stft_power(x.to(dtype)[None], n_fft, hop, win)
            shares.append(((p < EPS).double().mean().item(), ((p > 0) & (p < EPS / 4)).double().mean().item()))
        (clamped, faint), (clamped32, faint32) = shares
        print(f"{name} {n_fft}/{hop}/{win}: clamped {clamped:.3f}, non-zero below eps/4 {faint:.3f} (fp32 STFT: "
              f"{clamped32:.3f}, {faint32:.3f})")
        assert clamped32 == clamped                      # the dead zone: no bin changes sides in fp32
        if name in si.GAPPED:
            assert 0.1 <= clamped <= 0.9, (name, n_fft, clamped)
        elif name in ALL_CLAMPED:
            assert clamped == 1.0
        else:
            assert clamped == 0.0
        if name in si.WITH_FAINT:
            assert faint >= 0.05 and faint32 >= 0.05, (name, n_fft, faint, faint32)
            assert faint32 == faint


def _rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else (0.0 if a == 0 else float("inf"))


@pytest.mark.parametrize("key", list(si.RESOLUTION_SETS))
@pytest.mark.parametrize("name", NAMES)
def test_fp32_oracle_is_within_a_tenth_of_every_bar(name, key):
    res = si.RESOLUTION_SETS[key]
    r64, r32 = si.silence_ref(name, res), si.silence_ref(name, res, torch.float32)
    worst = max(_rel(a, b) for s32, s64 in zip(r32.sums, r64.sums) for a, b in zip(s32.tolist(), s64.tolist()))
    ratios = si.row_ratios(r32.grad, r64.grad, max(res["fft_sizes"]))
    print(f"{name} {key}: fp32 oracle sums {worst:.1e} loss {_rel(r32.loss, r64.loss):.1e} gradient "
          + " ".join(f"{k}={v:.1e}" for k, v in ratios.items()))
    assert worst <= 0.1 * LOSS_BAR
    assert _rel(r32.loss, r64.loss) <= 0.1 * LOSS_BAR
    for k, v in ratios.items():
        assert v <= 0.1 * GRAD_BAR, (k, v)


@pytest.mark.parametrize("name", si.L1_ROWS)
def test_fp32_oracle_of_the_l1_losses_and_their_exact_zeros(name):
    for kind, case in si.L1_KINDS:
        l64, g64 = si.l1_ref(kind, name, case, torch.float64)
        l32, g32 = si.l1_ref(kind, name, case, torch.float32)
        ratios = si.row_ratios(g32, g64, case[0])
        print(f"{name} {kind} {case}: fp32 oracle loss {_rel(l32, l64):.1e} gradient "
              + " ".join(f"{k}={v:.1e}" for k, v in ratios.items()))
        assert _rel(l32, l64) <= 0.1 * LOSS_BAR
        for k, v in ratios.items():
            assert v <= 0.1 * GRAD_BAR, (kind, case, k, v)
        if name == "pred_silent":
            assert torch.count_nonzero(g64).item() == 0
        elif name in QUIET_STRETCH and name != "faint_gap":
            lo, hi = si.untouched_range(*si.quiet_region(name), case[0], case[1])
            assert torch.count_nonzero(g64[lo:hi]).item() == 0 and torch.count_nonzero(g64[lo - 8:lo]).item() > 0


@pytest.mark.parametrize("key", list(si.RESOLUTION_SETS))
def test_exact_facts(key):
    res = si.RESOLUTION_SETS[key]
    for name in ("identical", "both_silent"):
        r = si.silence_ref(name, res)
        assert r.loss == 0.0 and torch.count_nonzero(r.grad).item() == 0
        assert all(s[0].item() == 0.0 and s[2].item() == 0.0 for s in r.sums)
    for name in ("pred_silent", "pred_faint"):
        assert torch.count_nonzero(si.silence_ref(name, res).grad).item() == 0
    for name in QUIET_STRETCH:
        lo, hi = si.untouched_range_of(name, res)
        a, b = si.quiet_region(name)
        assert hi - lo >= (b - a) // 2                                   # most of the stretch
        if name == "identical":
            continue                                                     # its gradient is 0 everywhere
        g = si.silence_ref(name, res).grad
        assert torch.count_nonzero(g[lo:hi]).item() == 0, name
        # tight: the last frame that starts before the stretch ends at lo, the first that leaves it starts at hi (its
        # first window sample is the periodic hann window's zero)
        assert torch.count_nonzero(g[lo - 8:lo]).item() > 0 and torch.count_nonzero(g[hi:hi + 8]).item() > 0, name

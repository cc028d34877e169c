"""The output gain of sound matching on the GPU: ias_gain_apply, ias_gain_backward and ias_gain_solve against the fp64 model
of their contract (tests/gain_model.py; include/ias_hip_gain.h), their bit guarantees, ``apply_gain``'s autograd,
``SoundMatcher.fit(gain=...)`` / ``fit_tied(gain=...)`` and ``match_audio.py --gain``."""
import json
import math
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import gain_model as gm
from oracle import synth_oracle as so

pytestmark = pytest.mark.gpu

# T: one sample; less than a wave's float4s; a partly filled chunk whose last vector straddles the end; two chunks.  An odd
# T puts the rows of B = 5 at every 16-byte phase.
LENGTHS = (1, 63, 4099, gm.CHUNK + 5)
G01 = np.array([0.75, 0.3, 0.9, 0.524, 1.0], np.float32)       # 0, -36, +12, -18.08, +20 dB
DB18 = 20.0 * math.log10(0.125)                                  # -18.0618


def _rows(T, seed):
    """(audio, g_out) [5, T] fp32.  audio: row 2 is +-1e15, row 4 holds a NaN; g_out: row 1 is zero, row 2 is +-1e15.  Row 3
    is ordinary in both: it is the row of the B = 1 case."""
    rng = np.random.default_rng(seed)
    audio = rng.standard_normal((5, T)).astype(np.float32)
    g_out = rng.standard_normal((5, T)).astype(np.float32)
    audio[2] = np.where(audio[2] < 0, -1e15, 1e15).astype(np.float32)
    g_out[2] = np.where(g_out[2] < 0, -1e15, 1e15).astype(np.float32)
    g_out[1] = 0.0
    audio[4, T // 2] = np.nan
    return audio, g_out


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _cases(T):
    audio, g_out = _rows(T, T)
    return [(audio, g_out, G01), (audio[3:4], g_out[3:4], G01[3:4])]


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("T", LENGTHS)
def test_apply_and_g_audio_match_the_model(lib, dev, T):
    """|err| <= 2^-22 |A x|: a is within one fp32 ulp (2^-23 relative) of the fp64 A, and the product rounds once
    (2^-24).  Zero stays zero, NaN stays NaN."""
    from inverse_audio_synthesis_amd.match import gain_backward, gain_forward
    for audio, g_out, g01 in _cases(T):
        for x in (audio, g_out):                     # g_out as an input too: its zero row
            want = gm.apply(x, g01)
            got = gain_forward(_t(x, dev), _t(g01, dev)).cpu().double().numpy()
            assert np.array_equal(np.isnan(got), np.isnan(want))
            ok = ~np.isnan(want)
            err = np.abs(got - want)[ok]
            assert (err <= 2.0 ** -22 * np.abs(want)[ok]).all(), (T, err.max())
        want, _g, _mag = gm.backward(g_out, audio, g01)
        got = gain_backward(_t(g_out, dev), _t(audio, dev), _t(g01, dev))[0].cpu().double().numpy()
        assert (np.abs(got - want) <= 2.0 ** -22 * np.abs(want)).all(), T
        if len(g01) == 5:
            assert not got[1].any()


@pytest.mark.parametrize("T", LENGTHS)
def test_g_gain01_matches_the_model(lib, dev, T):
    """D_b: the products are exact in fp64 and T - 1 additions round, each by at most 2^-53 of a partial sum that is at
    most sum |g x|: |err D| <= T 2^-52 sum |g x| with room.  The scaling by A K (two fp64 products, the device's exp10)
    and the rounding to fp32 (2^-24) add less than 2^-23 relative."""
    from inverse_audio_synthesis_amd.match import gain_backward
    for audio, g_out, g01 in _cases(T):
        _ga, want, mag = gm.backward(g_out, audio, g01)
        got = gain_backward(_t(g_out, dev), _t(audio, dev), _t(g01, dev))[1].cpu().double().numpy()
        tol = T * 2.0 ** -52 * mag * gm.amplitude(g01) * gm.K + 2.0 ** -23 * np.abs(want)
        for b in range(len(g01)):
            if np.isnan(want[b]):
                assert np.isnan(got[b]), (T, b)
                continue
            print(f"g_gain01 T={T} B={len(g01)} row {b}: |err| {abs(got[b] - want[b]):.3g} bound {tol[b]:.3g}")
            assert abs(got[b] - want[b]) <= tol[b], (T, b, got[b], want[b])
        if len(g01) == 5:
            assert got[1] == 0.0 and np.isnan(want[4])          # the zero cotangent; the NaN in audio reaches D alone


@pytest.mark.parametrize("T", LENGTHS)
def test_solve_matches_the_model(lib, dev, T):
    """|db - db_ref| <= 1e-4 dB: a relative T 2^-52 on two fp64 sums and one fp32 store of g01 move db by about 5e-6."""
    from inverse_audio_synthesis_amd.match import solve_gain
    for render, target, _g in _cases(T):
        target = target.copy()
        if len(_g) == 5:
            target[0] = render[0] * np.float32(0.125)            # -18.0618 dB exactly
            target[3] = render[3] * np.float32(1e-4)             # -80 dB: clamps to -60
        want01, want_db = gm.solve(target, render)
        got = solve_gain(_t(target, dev), _t(render, dev)).cpu().numpy()
        assert got.dtype == np.float32
        err = np.abs(gm.db_of(got) - want_db)
        print(f"solve T={T} B={len(_g)}: max |db - db_ref| = {err.max():.3g}")
        assert (err <= 1e-4).all(), (T, err)
        if len(_g) == 5:                             # a silent target, a NaN in the render: 0 dB exactly; the clamp
            assert got[1] == 0.75 and got[4] == 0.75 and got[3] == 0.0 and abs(gm.db_of(got)[0] - DB18) <= 1e-4
    up = solve_gain(_t(render * np.float32(100.0), dev), _t(render, dev)).cpu().numpy()
    assert up[0] == 1.0                              # +40 dB: clamps to +20


@pytest.mark.parametrize("T", LENGTHS)
def test_row_bits_do_not_depend_on_position(lib, dev, T):
    from inverse_audio_synthesis_amd.match import gain_backward, gain_forward, solve_gain
    (audio, g_out, g01), (audio1, g_out1, g011) = _cases(T)
    five = [_t(a, dev) for a in (audio, g_out, g01)]
    one = [_t(a, dev) for a in (audio1, g_out1, g011)]
    assert torch.equal(gain_forward(five[0], five[2])[3], gain_forward(one[0], one[2])[0])
    a5, g5 = gain_backward(five[1], five[0], five[2])
    a1, g1 = gain_backward(one[1], one[0], one[2])
    assert torch.equal(a5[3], a1[0]) and torch.equal(g5[3:4], g1)
    assert torch.equal(solve_gain(five[1], five[0])[3:4], solve_gain(one[1], one[0]))


def test_refusals_write_nothing(lib, dev):
    from inverse_audio_synthesis_amd import _lib
    B, T = 3, 100
    audio, g_out = (torch.randn((B, T), device=dev) for _ in range(2))
    g01 = torch.full((B,), 0.5, device=dev)
    out, vec = torch.full((B, T), 7.0, device=dev), torch.full((B,), 7.0, device=dev)
    scratch = torch.full((B, 2), 7.0, dtype=torch.float64, device=dev)
    P, st = _lib.ptr, _lib.stream()
    assert lib.ias_gain_partials_count(0) == -1 and lib.ias_gain_partials_count(-5) == -1
    assert lib.ias_gain_partials_count(gm.CHUNK) == 1 and lib.ias_gain_partials_count(gm.CHUNK + 1) == 2
    keep = audio.clone()
    flat = audio.reshape(-1)
    calls = [
        lib.ias_gain_apply(None, P(g01), P(out), B, T, st), lib.ias_gain_apply(P(audio), None, P(out), B, T, st),
        lib.ias_gain_apply(P(audio), P(g01), None, B, T, st), lib.ias_gain_apply(P(audio), P(g01), P(out), 0, T, st),
        lib.ias_gain_apply(P(audio), P(g01), P(out), B, 0, st), lib.ias_gain_apply(P(audio), P(g01), P(out), -1, T, st),
        lib.ias_gain_apply(P(audio), P(g01), P(audio), B, T, st),                   # out is audio
        lib.ias_gain_apply(P(flat[:T]), P(g01), P(flat[T - 1:]), 1, T, st),        # out overlaps audio's last sample
        lib.ias_gain_backward(None, P(audio), P(g01), P(out), P(vec), P(scratch), B, T, st),
        lib.ias_gain_backward(P(g_out), None, P(g01), P(out), P(vec), P(scratch), B, T, st),
        lib.ias_gain_backward(P(g_out), P(audio), None, P(out), P(vec), P(scratch), B, T, st),
        lib.ias_gain_backward(P(g_out), P(audio), P(g01), None, P(vec), P(scratch), B, T, st),
        lib.ias_gain_backward(P(g_out), P(audio), P(g01), P(out), None, P(scratch), B, T, st),
        lib.ias_gain_backward(P(g_out), P(audio), P(g01), P(out), P(vec), None, B, T, st),
        lib.ias_gain_backward(P(g_out), P(audio), P(g01), P(out), P(vec), P(scratch), 0, T, st),
        lib.ias_gain_backward(P(g_out), P(audio), P(g01), P(out), P(vec), P(scratch), B, 0, st),
        lib.ias_gain_backward(P(g_out), P(audio), P(g01), P(audio), P(vec), P(scratch), B, T, st),     # g_audio is audio
        lib.ias_gain_backward(P(audio), P(g_out), P(g01), P(audio), P(vec), P(scratch), B, T, st),     # g_audio is g_out
        lib.ias_gain_solve(None, P(audio), P(vec), P(scratch), B, T, st),
        lib.ias_gain_solve(P(g_out), None, P(vec), P(scratch), B, T, st),
        lib.ias_gain_solve(P(g_out), P(audio), None, P(scratch), B, T, st),
        lib.ias_gain_solve(P(g_out), P(audio), P(vec), None, B, T, st),
        lib.ias_gain_solve(P(g_out), P(audio), P(vec), P(scratch), 0, T, st),
        lib.ias_gain_solve(P(g_out), P(audio), P(vec), P(scratch), B, 0, st),
    ]
    assert calls == [-1] * len(calls)
    assert lib.ias_gain_apply(P(audio), P(g01), P(out), 65536, T, st) == -2
    torch.cuda.synchronize()
    assert torch.equal(audio, keep) and (out == 7.0).all() and (vec == 7.0).all() and (scratch == 7.0).all()


def test_apply_gain_autograd_is_the_entry_points(lib, dev):
    from inverse_audio_synthesis_amd.match import apply_gain, gain_backward, gain_forward
    audio, g_out, g01 = (_t(a, dev) for a in (*_rows(4099, 9)[:2], G01))
    audio[4] = torch.randn(4099, device=dev)         # finite: torch.equal below
    x, g = audio.clone().requires_grad_(True), g01.clone().requires_grad_(True)
    out = apply_gain(x, g)
    assert torch.equal(out, gain_forward(audio, g01)) and out.data_ptr() != x.data_ptr()
    out.backward(g_out)
    want_x, want_g = gain_backward(g_out, audio, g01)
    assert torch.equal(x.grad, want_x) and torch.equal(g.grad, want_g)
    assert torch.equal(apply_gain(audio, torch.full((5,), 0.75, device=dev)), audio)       # 0 dB: a = 1 exactly


# ------------------------------------------------------------------------------------------------ the matcher
def _voice(dev, B=4, sr=16000, sec=1.0):
    from inverse_audio_synthesis_amd.voice import SynthConfig, Voice
    return Voice(SynthConfig(batch_size=B, sample_rate=sr, buffer_size_seconds=sec, reproducible=False)).to(dev)


def _mel_kw():
    return dict(n_fft=1024, hop_length=512, n_mels=128, power=2.0)


def _params(dev, seed=7):
    return so.sample_params01(so.VoiceConfig(4, 16000, 1.0), seed).to(dev)


@pytest.mark.parametrize("steps", (0, 3))
def test_matcher_fixed_point_under_a_level_change(lib, dev, steps):
    """Target = 0.125 x the render of tp, start at tp, gain solved: the gain is -18.0618 dB, the parameters stay, and what
    is left of the loss is the rounding of a (about 1e-6 relative in power) where the mismatch without a gain is 1 - 1/64
    of the mel energy: three orders of margin below the factor 1e-3."""
    from inverse_audio_synthesis_amd.match import SoundMatcher
    v = _voice(dev)
    tp = _params(dev)
    target = 0.125 * v.render(tp)
    m = SoundMatcher(v, mel_kwargs=_mel_kw())
    res = m.fit(target, init_params01=tp, steps=steps, gain="solved", return_audio=True)
    plain = m.fit(target, init_params01=tp, steps=steps)
    print(f"fixed point, steps={steps}: gain_db {res.gain_db.tolist()}, loss / loss without a gain "
          f"{(res.loss.double() / plain.loss.double()).tolist()}")
    assert res.gain_db.dtype == torch.float32 and res.gain_db.shape == (4,)
    assert ((res.gain_db.double() - DB18).abs() <= 1e-3).all() and torch.equal(res.gain_db, res.initial_gain_db)
    assert torch.equal(res.params01, tp) and res.params01.shape == (4, 78)
    assert (res.loss.double() <= 1e-3 * plain.loss.double()).all()
    assert plain.gain_db is None and plain.initial_gain_db is None
    assert torch.equal(m.loss.per_item(res.audio, target_audio=target), res.loss)


def test_matcher_gain_only_descent(lib, dev):
    """All 78 columns frozen at the target's, the gain free from 0 dB, 50 steps at lr 0.02.  The mel-power loss is then
    exactly |a^2 - 1/64| mean(M): the fp64 model is a scalar Adam run (gain_model.gain_only_descent), which ends at best /
    initial = 6.2e-4 and 0.17 dB from the true gain.  Asserted: 0.01 and 0.5 dB, about 16 x and 3 x the model's figures."""
    from inverse_audio_synthesis_amd import voice_spec as S
    from inverse_audio_synthesis_amd.match import SoundMatcher, apply_gain, gain01_from_db
    v = _voice(dev)
    tp = _params(dev)
    target = 0.125 * v.render(tp)
    m = SoundMatcher(v, mel_kwargs=_mel_kw(), lr=0.02, frozen=[(mod, n) for (mod, n, *_r) in S.PARAMS])
    res = m.fit(target, init_params01=tp, steps=50, gain="fitted", init_gain_db=torch.zeros(4), return_audio=True)
    ratio = (res.loss.double() / res.initial_loss.double()).tolist()
    model_ratio, model_db = gm.gain_only_descent(DB18)
    print(f"gain-only descent: best / initial {[f'{r:.3g}' for r in ratio]} (model {model_ratio:.3g}); gain_db "
          f"{[f'{d:.4f}' for d in res.gain_db.tolist()]} (model {model_db:.4f}, true {DB18:.4f})")
    assert all(r <= 0.01 for r in ratio), ratio
    assert ((res.gain_db.double() - DB18).abs() <= 0.5).all(), res.gain_db
    assert res.initial_gain_db.tolist() == [0.0] * 4 and res.skipped.tolist() == [0] * 4
    assert torch.equal(res.params01, tp)
    assert torch.equal(m.loss.per_item(res.audio, target_audio=target), res.loss)
    again = apply_gain(v.render(res.params01), gain01_from_db(res.gain_db))      # gain_db is g01 to an fp32 ulp of dB
    assert torch.allclose(again, res.audio, rtol=1e-5, atol=0)


def test_matcher_mixer_levels_with_and_without_gain(lib, dev):
    """tests/test_match_gpu.py::test_matcher_descends_on_mixer_levels (three mixer levels free, started at 0.5, 50 steps at
    lr 0.02) against the target 18 dB down, with a fitted gain and without one.  With the gain every sound's loss is at
    least halved, and ends below the loss of the fit that has the mixer levels alone to pay for the level.
    The same two fits on the CPU through the oracle's fp64 render and torch.optim.Adam (scripts/gain_oracle_descent.py 7),
    seed 7: best / initial with the gain 0.1427, 0.0088, 0.0606, 0.0103 (bound 0.5: 3.5 x room at the least); best with /
    best without 0.0231, 0.0189, 0.0733, 0.0225 (bound 1: 13 x room).  Seeds 0 .. 3 meet both conditions in the oracle too
    (worst figures 0.19 / 0.05, 0.15 / 0.10, 0.03 / 0.04, 0.32 / 0.38); seed 4 does not halve one sound (0.51)."""
    from inverse_audio_synthesis_amd import voice_spec as S
    from inverse_audio_synthesis_amd.match import SoundMatcher
    v = _voice(dev)
    tp = _params(dev)
    target = 0.125 * v.render(tp)
    free = [("mixer", n) for n in ("vco_1", "vco_2", "noise")]
    cols = [S.INDEX[k] for k in free]
    init = tp.clone()
    init[:, cols] = 0.5
    frozen = [(mod, n) for (mod, n, *_r) in S.PARAMS if (mod, n) not in free]
    m = SoundMatcher(v, mel_kwargs=_mel_kw(), lr=0.02, frozen=frozen)
    with_gain = m.fit(target, init_params01=init, steps=50, gain="fitted")
    without = m.fit(target, init_params01=init, steps=50)
    ratio = (with_gain.loss.double() / with_gain.initial_loss.double()).tolist()
    against = (with_gain.loss.double() / without.loss.double()).tolist()
    print(f"mixer levels with a fitted gain: best / initial {[f'{r:.4f}' for r in ratio]}; best with / best without "
          f"{[f'{r:.4f}' for r in against]}; gain_db {[f'{d:.2f}' for d in with_gain.gain_db.tolist()]}")
    assert all(r <= 0.5 for r in ratio), ratio
    assert (with_gain.loss < without.loss).all(), against
    fcols = [S.INDEX[k] for k in frozen]
    assert torch.equal(with_gain.params01[:, fcols], tp[:, fcols]) and with_gain.skipped.tolist() == [0] * 4


def _six(v, dev, noise=None):
    """Six targets at six levels (two chunks at B = 4, the last padded) -> (their parameters [6, 78], audio [6, T])."""
    from inverse_audio_synthesis_amd import voice_spec as S
    tp = torch.cat([_params(dev, s) for s in (3, 4)])
    if noise is not None:
        tp[:, S.INDEX[("mixer", "noise")]] = noise
    audio = torch.cat([v.render(tp[:4]), v.render(tp[4:])])[:6]
    scale = torch.tensor([0.125, 1.0, 0.5, 2.0, 0.03, 0.25], device=dev)
    return tp[:6].contiguous(), (audio * scale.unsqueeze(1)).contiguous()


def test_matcher_gain_pads_the_last_chunk_and_keeps_the_chosen_starts_gain(lib, dev):
    from inverse_audio_synthesis_amd.match import SoundMatcher
    v = _voice(dev)
    tp, target = _six(v, dev)
    m = SoundMatcher(v, mel_kwargs=_mel_kw(), lr=0.02)
    six = m.fit(target, steps=4, gain="fitted", return_audio=True)
    four = m.fit(target[:4], steps=4, gain="fitted")
    assert six.params01.shape == (6, 78) and six.gain_db.shape == (6,) and six.audio.shape == (6, 16000)
    for k in ("params01", "loss", "initial_loss", "gain_db", "initial_gain_db"):
        assert torch.equal(getattr(six, k)[:4], getattr(four, k)), k
    assert torch.isfinite(six.gain_db).all() and len(set(six.initial_gain_db.tolist())) == 6
    # two starts per sound: a detuned, quieter copy and the target's own parameters, whose solved gain is the scale.  Row
    # n of the targets is fitted at rows 2 n and 2 n + 1 of the flattened fit: mixer.noise is 0 here, because the Voice's
    # noise is a row per batch position
    tp, target = _six(v, dev, noise=0.0)
    starts = torch.stack([(tp[:4] * 0.8).contiguous(), tp[:4]], dim=1)
    res = m.fit(target[:4], init_params01=starts, steps=2, gain="fitted")
    flat = m.fit(target[:4].repeat_interleave(2, dim=0), init_params01=starts.reshape(8, 78), steps=2, gain="fitted")
    rows = torch.arange(4, device=dev) * 2 + res.start
    assert res.start.tolist() == [1, 1, 1, 1] and res.start_loss.shape == (4, 2)
    for k in ("params01", "loss", "gain_db", "initial_gain_db"):
        assert torch.equal(getattr(res, k), getattr(flat, k)[rows]), k
    want = torch.tensor([20.0 * math.log10(s) for s in (0.125, 1.0, 0.5, 2.0)], dtype=torch.float64, device=dev)
    assert ((res.gain_db.double() - want).abs() <= 1e-3).all(), res.gain_db
    assert not torch.equal(flat.gain_db[0::2], flat.gain_db[1::2])


def _mean_in_row_order(losses):
    s = None
    for x in losses.tolist():
        s = x if s is None else s + x
    return s / len(losses)


def test_fit_tied_with_a_gain_per_note(lib, dev):
    """One preset at two notes, the second 12.04 dB down; mixer.noise is frozen at 0 (the Voice's noise is a row per batch
    position).  Solved from the true parameters the gains are 0 and -12.0412 dB.  Fitted from there for three steps, the
    start (whose loss is the rounding of a alone) stays the best: the gains stay 12 dB apart (0.5 dB: the margin of the
    gain-only test).  Fitted from mixer levels at 0.5, whatever iterate is kept, the notes agree in every tied column while
    each keeps a gain of its own."""
    from inverse_audio_synthesis_amd import voice_spec as S
    from inverse_audio_synthesis_amd.match import SoundMatcher
    v = _voice(dev)
    tp = _params(dev)[:1].repeat(2, 1)
    tp[:, S.INDEX[("keyboard", "midi_f0")]] = torch.tensor([0.35, 0.55], device=dev)
    tp[:, S.INDEX[("mixer", "noise")]] = 0.0
    target = v.render(torch.cat([tp, torch.full((2, 78), 0.5, device=dev)]))[:2].contiguous()
    target[1] *= 0.25
    m = SoundMatcher(v, mel_kwargs=_mel_kw(), frozen=[("mixer", "noise")])
    groups = torch.zeros(2, dtype=torch.int64)
    solved = m.fit_tied(target, groups, init_params01=tp, steps=0, gain="solved")
    want = torch.tensor([0.0, 20.0 * math.log10(0.25)], dtype=torch.float64, device=dev)
    assert ((solved.gain_db.double() - want).abs() <= 1e-3).all(), solved.gain_db
    assert torch.equal(solved.params01, tp) and torch.equal(solved.gain_db, solved.initial_gain_db)
    tied = m.tied_mask().bool().cpu()
    fitted = m.fit_tied(target, groups, init_params01=tp, steps=3, gain="fitted")
    apart = (fitted.gain_db[0] - fitted.gain_db[1]).item()
    print(f"tied fit with gains: gain_db {fitted.gain_db.tolist()}, apart {apart:.4f} dB")
    assert abs(apart - 12.0412) <= 0.5 and fitted.params01.shape == (2, 78)
    init = tp.clone()
    init[:, [S.INDEX[("mixer", n)] for n in ("vco_1", "vco_2")]] = 0.5
    moved = m.fit_tied(target, groups, init_params01=init, steps=4, gain="fitted")
    for res in (fitted, moved):
        rows = res.params01.cpu()
        assert torch.equal(rows[:, tied], rows[:1, tied].expand(2, -1))
        assert res.group_loss.tolist() == [_mean_in_row_order(res.loss.cpu())]
    print(f"tied fit from mixer levels 0.5: group loss / initial {(moved.group_loss / moved.initial_group_loss).tolist()}, "
          f"gain_db {moved.gain_db.tolist()} from {moved.initial_gain_db.tolist()}")
    assert (moved.group_loss <= moved.initial_group_loss).all() and moved.skipped.tolist() == [0]
    assert moved.gain_db[0] != moved.gain_db[1] and moved.gain_db.shape == (2,)


def test_fit_tied_with_singleton_groups_and_a_gain_is_fit(lib, dev):
    from inverse_audio_synthesis_amd.match import SoundMatcher
    v = _voice(dev)
    _tp, target = _six(v, dev)
    m = SoundMatcher(v, mel_kwargs=_mel_kw(), lr=0.02, frozen=[("lfo_1", "frequency")])
    init = torch.rand((6, 78), generator=torch.Generator().manual_seed(11)).to(dev)
    for mode in ("fitted", "solved"):
        want = m.fit(target, init_params01=init, steps=4, return_audio=True, gain=mode)
        got = m.fit_tied(target, torch.arange(6), init_params01=init, steps=4, return_audio=True, gain=mode)
        for k in ("params01", "gain_db", "initial_gain_db", "loss", "initial_loss", "skipped", "audio"):
            assert torch.equal(getattr(got, k), getattr(want, k)), (mode, k)
    with pytest.raises(ValueError):
        m.fit(target, steps=1, gain="free")
    with pytest.raises(ValueError):
        m.fit(target, steps=1, init_gain_db=torch.zeros(6))


# ------------------------------------------------------------------------------------------------ entry point
def _write_wav(path, x, sr):
    pcm = np.round(np.clip(x, -1, 1) * 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(pcm.tobytes())


def _rms_db(path):
    with wave.open(str(path), "rb") as w:
        x = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.float64) / 32768.0
    return 10.0 * math.log10(np.mean(x * x))


def test_match_audio_gain_entry_point(lib, dev, tmp_path):
    from conftest import ROOT
    v = _voice(dev, B=2)
    audio = v.render(so.sample_params01(so.VoiceConfig(2, 16000, 1.0), 13).to(dev)).cpu().numpy()
    _write_wav(tmp_path / "a.wav", 0.1 * audio[0], 16000)
    recs = {}
    for name, flags in (("gained", ["--gain", "fitted"]), ("plain", [])):
        out = tmp_path / name
        cmd = [sys.executable, os.path.join(ROOT, "match_audio.py"), str(tmp_path / "a.wav"), "torchsynth.rate=16000",
               "torchsynth.buffer_size_seconds=1.0", "--steps", "3", *flags, "--out", str(out)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-4000:]
        recs[name] = json.load(open(out / "a.params.json"))
    rec = recs["gained"]
    assert rec["gain_mode"] == "fitted" and math.isfinite(rec["fit_gain_db"]) and rec["fit_gain_db"] < 0.0
    assert math.isfinite(rec["initial_gain_db"]) and len(rec["params"]) == 78
    # one Adam step of the gain column is lr 80 dB = 0.8 dB: 6 dB is the slack around the solved start, which has the
    # target's energy
    got, want = _rms_db(tmp_path / "gained" / "a.match.wav"), _rms_db(tmp_path / "a.wav")
    print(f"match_audio --gain fitted: initial {rec['initial_gain_db']:.2f} dB, fitted {rec['fit_gain_db']:.2f} dB; RMS of "
          f"the match {got:.2f} dB, of the input {want:.2f} dB")
    assert abs(got - want) <= 6.0
    assert not {"gain_mode", "initial_gain_db", "fit_gain_db"} & set(recs["plain"])

"""ias_match_tied_step on the GPU against the fp64 model of its contract (tests/tied_model.py), its bit guarantees
(singleton groups are ias_match_adam_step; a group's bits do not depend on its place), ``SoundMatcher.fit_tied`` and
``match_audio.py --split --shared``."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import onset_model as om
import tied_model as tm
from oracle import synth_oracle as so

pytestmark = pytest.mark.gpu

ARRAYS = ("params01", "m", "v", "best_params", "step", "skipped", "best_loss", "group_loss")
P = 78
SIZES = (1, 4, 1, 5)                                 # rows per group: N = 11
FROZEN = [5, 17, 40, 77]
OWN = [0, 1, 30]                                     # the two keyboard columns and one more


def _masks():
    free = np.ones(P, np.uint8)
    free[FROZEN] = 0
    tied = np.ones(P, np.uint8)
    tied[OWN] = 0
    return free, tied


def _dev(st, dev):
    return {k: torch.from_numpy(a.copy()).to(dev) for k, a in st.items()}


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _step(st, grad, loss, group_start, free, tied, active, dev, update=1, lr=0.01, betas=(0.9, 0.999), eps=1e-8):
    from inverse_audio_synthesis_amd.match import tied_adam_step
    tied_adam_step(st["params01"], _t(grad, dev), st["m"], st["v"], st["best_params"], _t(loss, dev),
                   _t(np.asarray(group_start, np.int32), dev), st["step"], st["skipped"], st["best_loss"], st["group_loss"],
                   _t(free, dev), _t(tied, dev), _t(np.asarray(active, np.uint8), dev), update, lr, betas, eps)


def _inputs(N, seed, iters=5):
    """Per iteration (grad [N, P], loss [N]): random gradients; odd iterations are worse than the even ones before."""
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((N, P)).astype(np.float32),
             (rng.random(N) + (0.0 if it % 2 == 0 else 1.0)).astype(np.float32)) for it in range(iters)]


def _starts(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def _mean_in_row_order(losses):
    """fp32 losses -> their fp64 sum in row order over their number, as a Python float."""
    s = None
    for x in losses.tolist():                        # fp32 -> Python floats: exact
        s = x if s is None else s + x
    return s / len(losses)


# ------------------------------------------------------------------------------------------------ the step
def test_tied_step_matches_fp64_model(lib, dev):
    """Measured on an MI355X (max |device - model| over the max |model|, after five steps): params01 1.06e-07, m 3.8e-08,
    v 9.85e-08, best_params 6.5e-08; group_loss and best_loss equal the model's bit for bit (relative error 0).  The
    bound is the untied step's (tests/test_match_gpu.py::test_adam_step_matches_fp64_rule): the one extra rounding of the
    mean gradient to fp32 is 6e-8 relative on g and does not show in it."""
    N, G = sum(SIZES), len(SIZES)
    gs = _starts(SIZES)
    free, tied = _masks()
    active = [1, 1, 0, 1]
    host = tm.state(N, P, G, seed=1)
    st, ref = _dev(host, dev), tm.as_fp64(host)
    for grad, loss in _inputs(N, 2):
        _step(st, grad, loss, gs, free, tied, active, dev)
        tm.tied_step(ref, grad, loss, gs, free, tied, active)
    for k in ("params01", "m", "v", "best_params"):
        got, want = st[k].cpu().double().numpy(), ref[k]
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"tied step vs fp64 model: {k} max|err| / max|model| = {err:.3g}")
        assert err <= 1e-6, (k, err)
    for k in ("step", "skipped", "best_loss"):
        assert np.array_equal(st[k].cpu().numpy(), ref[k]), k
    got, want = st["group_loss"].cpu().numpy(), ref["group_loss"]
    rel = np.abs(got - want).max() / np.abs(want).max()
    print(f"tied step vs fp64 model: group_loss max relative error = {rel:.3g}")
    assert rel <= 1e-15
    assert st["step"].cpu().tolist() == [5, 5, 0, 5] and np.isinf(ref["best_loss"][2])      # the inactive group


def test_singleton_groups_are_the_untied_step_bit_for_bit(lib, dev):
    from inverse_audio_synthesis_amd.match import match_adam_step
    N = 7
    free, tied = _masks()
    active = np.array([1, 1, 1, 0, 1, 1, 1], np.uint8)
    host = tm.state(N, P, N, seed=3)
    a, b = _dev(host, dev), _dev(host, dev)
    hyper = dict(lr=0.02, betas=(0.8, 0.99), eps=1e-7)
    for it, (grad, loss) in enumerate(_inputs(N, 4, iters=6)):
        if it in (1, 4):
            grad[1, 10] = np.nan                     # a free column: row 1 skips
            grad[2, FROZEN[0]] = np.inf              # a frozen column: ignored
            loss[5] = np.nan                         # a non-finite loss: row 5 skips, and is never a best
        _step(a, grad, loss, np.arange(N + 1), free, tied, active, dev, **hyper)
        match_adam_step(b["params01"], _t(grad, dev), b["m"], b["v"], b["step"], _t(loss, dev), b["best_loss"],
                        b["best_params"], _t(free, dev), _t(active, dev), b["skipped"], hyper["lr"], hyper["betas"],
                        hyper["eps"])
        for k in ARRAYS[:-1]:
            assert torch.equal(a[k], b[k]), (it, k)
    assert a["skipped"].cpu().tolist() == [0, 2, 0, 0, 0, 2, 0] and a["step"].cpu().tolist() == [6, 4, 6, 0, 6, 4, 6]


def test_group_bits_do_not_depend_on_position(lib, dev):
    N, G = sum(SIZES), len(SIZES)
    free, tied = _masks()
    tied_free = torch.from_numpy((free != 0) & (tied != 0))
    # the first two groups' blocks of rows exchanged: rows 0 | 1..4 -> 1..4 | 0
    perm = np.array([1, 2, 3, 4, 0] + list(range(5, N)))
    sizes2, gperm = (4, 1, 1, 5), [1, 0, 2, 3]
    host = tm.state(N, P, G, seed=5)
    host["params01"][1:5, 9] += np.float32(0.01) * np.arange(4, dtype=np.float32)    # a start that disagrees in a tied column
    host2 = {k: (a[perm] if a.shape[0] == N else a[gperm]).copy() for k, a in host.items()}
    a, b = _dev(host, dev), _dev(host2, dev)
    for grad, loss in _inputs(N, 6):
        _step(a, grad, loss, _starts(SIZES), free, tied, [1] * G, dev)
        _step(b, grad[perm], loss[perm], _starts(sizes2), free, tied, [1] * G, dev)
        for k in ARRAYS:
            want = a[k].cpu()
            want = want[perm] if want.shape[0] == N else want[gperm]
            assert torch.equal(b[k].cpu(), want), k
        for r0, r1 in zip(_starts(SIZES)[:-1], _starts(SIZES)[1:]):
            for k in ("params01", "m", "v"):
                rows = a[k].cpu()[r0:r1][:, tied_free]
                assert torch.equal(rows, rows[:1].expand_as(rows)), (k, r0)
    assert not torch.equal(a["params01"][1:5, 0], a["params01"][1:2, 0].expand(4))         # own columns did go apart


def test_nonfinite_update0_and_refusals(lib, dev):
    from inverse_audio_synthesis_amd.match import tied_adam_step
    N, G = sum(SIZES), len(SIZES)
    gs = _starts(SIZES)
    free, tied = _masks()
    host = tm.state(N, P, G, seed=7)
    st = _dev(host, dev)
    (grad, loss), = _inputs(N, 8, iters=1)
    grad[0, FROZEN[1]] = np.inf                      # group 0: a frozen column, ignored
    grad[3, 12] = np.nan                             # group 1 (rows 1..4): one row's free column skips the whole group
    grad[8, OWN[2]] = -np.inf                        # group 3 (rows 6..10): an own column counts too ...
    loss[6:11] = 0.25
    loss[9] = np.inf                                 # ... and its L_g is not finite: no best either
    _step(st, grad, loss, gs, free, tied, [1] * G, dev)
    got = {k: t.cpu().numpy() for k, t in st.items()}
    assert got["skipped"].tolist() == [0, 1, 0, 1] and got["step"].tolist() == [1, 0, 1, 0]
    for k in ("params01", "m", "v"):
        assert np.array_equal(got[k][1:5], host[k][1:5]) and np.array_equal(got[k][6:11], host[k][6:11]), k
        assert np.array_equal(got[k][:, FROZEN], host[k][:, FROZEN]), k
    assert not np.array_equal(got["params01"][0], host["params01"][0])
    # best: the PRE-update parameters of every group with a finite L_g, the skipped group 1 included; not group 3
    assert np.array_equal(got["best_params"], host["params01"])
    want = [_mean_in_row_order(loss[0:1]), _mean_in_row_order(loss[1:5]), _mean_in_row_order(loss[5:6])]
    assert got["best_loss"][:3].tolist() == want and np.isinf(got["best_loss"][3]) and np.isinf(got["group_loss"][3])
    assert got["group_loss"][:3].tolist() == want
    # update = 0: only best_* and group_loss change; a tie keeps the stored best (strict), a lower L_g takes the rows
    before = {k: t.clone() for k, t in st.items()}
    loss2 = loss.copy()
    loss2[0] = loss[0] * np.float32(0.5)             # group 0: better
    loss2[6:11] = 0.125                              # group 3: finite now, better than +inf
    _step(st, np.full((N, P), np.nan, np.float32), loss2, gs, free, tied, [1] * G, dev, update=0)
    for k in ("params01", "m", "v", "step", "skipped"):
        assert torch.equal(st[k], before[k]), k
    assert torch.equal(st["best_params"][0], before["params01"][0]) and torch.equal(st["best_params"][6:], before["params01"][6:])
    assert torch.equal(st["best_params"][1:6], before["best_params"][1:6])
    assert st["best_loss"].cpu().tolist() == [float(np.float64(loss2[0])), want[1], want[2], 0.125]
    # refusals, each before any launch: the arrays are as they were
    before = {k: t.clone() for k, t in st.items()}
    with pytest.raises(RuntimeError, match="IAS_ERR_ARG"):
        _step(st, grad, loss, gs, free, tied, [1] * G, dev, eps=0.0)
    with pytest.raises(ValueError):
        _step(st, grad, loss, gs, free, tied, [1] * G, dev, update=2)
    args = [st["params01"], _t(grad, dev), st["m"], st["v"], st["best_params"], _t(loss, dev), _t(gs, dev), st["step"],
            st["skipped"], st["best_loss"], st["group_loss"], _t(free, dev), _t(tied, dev), torch.ones(G, dtype=torch.uint8, device=dev)]
    from inverse_audio_synthesis_amd import _lib
    raw = lambda N_, G_, P_, update: lib.ias_match_tied_step(      # noqa: E731
        *[_lib.ptr(t) for t in args], N_, G_, P_, update, 0.01, 0.9, 0.999, 1e-8, _lib.stream())
    assert raw(N, G, P, 2) == -1 and raw(N, G, P, -1) == -1 and raw(N, N + 1, P, 1) == -1 and raw(0, 0, P, 1) == -1
    assert raw(N, G, 0, 1) == -1
    assert raw(N, G, 129, 1) == -2 and raw(65536, 65536, P, 1) == -2 and raw(65536, 65535, 128, 3) == -1
    torch.cuda.synchronize()
    for k in ARRAYS:
        assert torch.equal(st[k], before[k]), k
    big = torch.zeros((3, 129), device=dev)           # through the wrapper: P = 129
    one = lambda dt, n=1: torch.zeros(n, dtype=dt, device=dev)     # noqa: E731
    with pytest.raises(RuntimeError, match="IAS_ERR_UNSUPPORTED"):
        tied_adam_step(big, big.clone(), big.clone(), big.clone(), big.clone(), one(torch.float32, 3),
                       torch.tensor([0, 3], dtype=torch.int32, device=dev), one(torch.int32), one(torch.int32),
                       one(torch.float64), one(torch.float64), one(torch.uint8, 129), one(torch.uint8, 129),
                       one(torch.uint8), 1, 0.01, (0.9, 0.999), 1e-8)


# ------------------------------------------------------------------------------------------------ fit_tied
def _voice(dev, B=4, sr=16000, sec=1.0):
    from inverse_audio_synthesis_amd.voice import SynthConfig, Voice
    return Voice(SynthConfig(batch_size=B, sample_rate=sr, buffer_size_seconds=sec, reproducible=False)).to(dev)


def _mel_kw():
    return dict(n_fft=1024, hop_length=512, n_mels=128, power=2.0)


def _six_targets(v, dev, noise=None):
    from inverse_audio_synthesis_amd import voice_spec as S
    tp = torch.cat([so.sample_params01(so.VoiceConfig(4, 16000, 1.0), s) for s in (3, 4)]).to(dev)       # [8, 78]
    if noise is not None:
        tp[:, S.INDEX[("mixer", "noise")]] = noise
    return torch.cat([v.render(tp[:4]), v.render(tp[4:])])[:6].contiguous()


def test_fit_tied_with_singleton_groups_is_fit(lib, dev):
    """Six targets at B = 4: a chunk boundary and a padded last chunk."""
    from inverse_audio_synthesis_amd.match import SoundMatcher
    v = _voice(dev)
    target = _six_targets(v, dev)
    m = SoundMatcher(v, mel_kwargs=_mel_kw(), lr=0.02, frozen=[("lfo_1", "frequency")])
    init = torch.rand((6, 78), generator=torch.Generator().manual_seed(11)).to(dev)
    want = m.fit(target, init_params01=init, steps=4, return_audio=True)
    got = m.fit_tied(target, torch.arange(6), init_params01=init, steps=4, return_audio=True)
    for k in ("params01", "loss", "initial_loss", "skipped", "audio"):
        assert torch.equal(getattr(got, k), getattr(want, k)), k
    assert torch.equal(got.group_loss, want.loss.double()) and torch.equal(got.initial_group_loss, want.initial_loss.double())
    assert got.params01.shape == (6, 78) and got.skipped.dtype == torch.int32
    with pytest.raises(ValueError):
        m.fit_tied(target, torch.tensor([0, 0, 1, 1, 0, 0]), steps=1)
    with pytest.raises(KeyError):
        m.fit_tied(target, torch.arange(6), own=[("keyboard", "velocity")], steps=1)


def test_fit_tied_group_across_the_chunk_boundary(lib, dev):
    """Groups [0, 0, 0, 1, 1, 1] at B = 4 against the same notes with the two groups' blocks exchanged: a group's rows sit
    in other chunks and at other batch positions.  The Voice's noise source is a row of noise per batch position (as
    torchsynth's), so a note's render depends on its position through it and on nothing else: the noise level is frozen
    at 0 here, on both sides."""
    from inverse_audio_synthesis_amd import voice_spec as S
    from inverse_audio_synthesis_amd.match import SoundMatcher
    v = _voice(dev)
    target = _six_targets(v, dev, noise=0.0)
    m = SoundMatcher(v, mel_kwargs=_mel_kw(), lr=0.02, frozen=[("mixer", "noise")])
    init = torch.rand((6, 78), generator=torch.Generator().manual_seed(12)).to(dev)
    init[:, S.INDEX[("mixer", "noise")]] = 0.0
    groups = torch.tensor([0, 0, 0, 1, 1, 1])
    swap = [3, 4, 5, 0, 1, 2]
    a = m.fit_tied(target, groups, init_params01=init, steps=3)
    b = m.fit_tied(target[swap].contiguous(), groups, init_params01=init[swap], steps=3)
    for k in ("params01", "loss", "initial_loss"):
        assert torch.equal(getattr(b, k), getattr(a, k)[swap]), k
    for k in ("group_loss", "initial_group_loss", "skipped"):
        assert torch.equal(getattr(b, k), getattr(a, k)[[1, 0]]), k
    tied = m.tied_mask().bool().cpu()
    for rows in (a.params01[:3].cpu(), a.params01[3:].cpu()):
        assert torch.equal(rows[:, tied], rows[:1, tied].expand(3, -1))
    assert a.group_loss.tolist() == [_mean_in_row_order(a.loss[:3].cpu()), _mean_in_row_order(a.loss[3:].cpu())]
    assert (a.group_loss <= a.initial_group_loss).all() and not torch.equal(a.params01, init)


MIDI01 = (0.35, 0.45, 0.55)                          # scripts/tied_oracle_descent.py: MIDI 44.45, 57.15, 69.85
PRESET_SEED = 7


def _phrase(v, dev):
    """Three targets from one preset (row 0 of the oracle's batch PRESET_SEED) at three notes -> (params [3, 78], audio)."""
    from inverse_audio_synthesis_amd import voice_spec as S
    tp = so.sample_params01(so.VoiceConfig(4, 16000, 1.0), PRESET_SEED)[:1].repeat(3, 1)
    tp[:, S.INDEX[("keyboard", "midi_f0")]] = torch.tensor(MIDI01)
    tp = tp.to(dev)
    pad = torch.cat([tp, torch.full((1, 78), 0.5, device=dev)])
    return tp, v.render(pad)[:3].contiguous()


def test_fit_tied_fixed_point(lib, dev):
    from inverse_audio_synthesis_amd.match import SoundMatcher
    v = _voice(dev)
    tp, target = _phrase(v, dev)
    res = SoundMatcher(v, mel_kwargs=_mel_kw()).fit_tied(target, torch.zeros(3, dtype=torch.int64), init_params01=tp, steps=3)
    assert res.group_loss.tolist() == [0.0] and res.initial_group_loss.tolist() == [0.0]
    assert torch.count_nonzero(res.loss).item() == 0 and torch.count_nonzero(res.initial_loss).item() == 0
    assert torch.equal(res.params01, tp) and res.skipped.tolist() == [0]


def test_fit_tied_descends_on_shared_mixer_levels(lib, dev):
    """One preset at three notes; the three mixer levels are the only free columns, tied, started at 0.5: 50 steps at lr
    0.02 must at least halve the group's mean mel L1, the condition of
    tests/test_match_gpu.py::test_matcher_descends_on_mixer_levels for the untied fit.
    Preset seed 7.  The same descent on the CPU through the oracle's fp64 render with torch.optim.Adam on the mean loss
    (scripts/tied_oracle_descent.py 7): best / initial = 0.0018 (seeds 0..7: 0.0166, 0.9576, 0.0027, 0.0015, 0.0015,
    0.0040, 0.0051, 0.0018: seed 1 does not descend in the oracle either).  Measured on an MI355X: 0.0018 (per note
    0.0030, 0.0012, 0.0008)."""
    from inverse_audio_synthesis_amd import voice_spec as S
    from inverse_audio_synthesis_amd.match import SoundMatcher
    v = _voice(dev)
    tp, target = _phrase(v, dev)
    free = [("mixer", n) for n in ("vco_1", "vco_2", "noise")]
    cols = [S.INDEX[k] for k in free]
    init = tp.clone()
    init[:, cols] = 0.5
    frozen = [(m, n) for (m, n, *_r) in S.PARAMS if (m, n) not in free]
    matcher = SoundMatcher(v, mel_kwargs=_mel_kw(), lr=0.02, frozen=frozen)
    res = matcher.fit_tied(target, [0, 0, 0], init_params01=init, steps=50)
    ratio = (res.group_loss / res.initial_group_loss).item()
    print(f"tied descent: final / initial group mel-L1 = {ratio:.4f} (per note: "
          f"{[f'{r:.4f}' for r in (res.loss.double() / res.initial_loss.double()).tolist()]})")
    assert ratio <= 0.5, ratio
    mix = res.params01[:, cols]
    assert torch.equal(mix, mix[:1].expand(3, -1)) and not torch.equal(mix[0], init[0, cols])
    fcols = [S.INDEX[k] for k in frozen]
    assert torch.equal(res.params01[:, fcols], tp[:, fcols])
    assert res.skipped.tolist() == [0]
    pad = torch.cat([res.params01, torch.full((1, 78), 0.5, device=dev)])
    fresh = matcher.loss.per_item(v.render(pad), target_audio=torch.cat([target, target.new_zeros((1, 16000))]))[:3]
    assert torch.equal(fresh, res.loss) and res.group_loss.item() == _mean_in_row_order(res.loss.cpu())


# ------------------------------------------------------------------------------------------------ entry point
RATE = 16000


def _write_pcm16(path, x, sr):
    pcm = np.clip(np.round(np.asarray(x, dtype=np.float64) * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(pcm.tobytes())


def _match_audio(tmp_path, name, *flags):
    from conftest import ROOT
    wav = tmp_path / "phrase.wav"
    if not wav.exists():
        _write_pcm16(wav, om.note_sequence(RATE), RATE)
    out = tmp_path / name
    cmd = [sys.executable, os.path.join(ROOT, "match_audio.py"), str(wav), "torchsynth.rate=16000",
           "torchsynth.buffer_size_seconds=1.0", "--steps", "2", "--out", str(out), *flags]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:]
    return out


def test_match_audio_shared_entry_point(lib, dev, tmp_path):
    out = _match_audio(tmp_path, "shared", "--split", "--pitch", "--shared")
    doc = json.load(open(out / "phrase.notes.json"))
    preset = json.load(open(out / "phrase.preset.json"))
    notes = doc["notes"]
    assert len(notes) == 4
    shared = doc["shared"]
    assert shared == preset["shared"] and preset["input"] == "phrase.wav"
    assert shared["own"] == ["keyboard.midi_f0", "keyboard.duration"] and len(shared["tied"]) == 76
    assert shared["group_loss"] <= shared["initial_group_loss"]
    tied = set(shared["tied"])
    by_note = [{f"{p['module']}.{p['name']}": (p["value01"], p["value"]) for p in note["params"]} for note in notes]
    assert all(len(d) == 78 for d in by_note) and tied == set(by_note[0]) - set(shared["own"])
    for d in by_note[1:]:
        assert all(d[k] == by_note[0][k] for k in tied)
    assert len({d["keyboard.midi_f0"] for d in by_note}) == 4
    assert len(preset["params"]) == 76
    assert {f"{p['module']}.{p['name']}": (p["value01"], p["value"]) for p in preset["params"]} == \
        {k: by_note[0][k] for k in tied}
    with wave.open(str(out / "phrase.match.wav"), "rb") as w:
        assert w.getnframes() == 48000 and w.getframerate() == RATE
    plain = _match_audio(tmp_path, "plain", "--split", "--pitch")
    assert sorted(os.listdir(plain)) == ["phrase.match.wav", "phrase.notes.json"]
    assert "shared" not in json.load(open(plain / "phrase.notes.json"))

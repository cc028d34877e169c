"""ias_envelope_frames and ias_envelope_score on the GPU against the fp64 model of their contracts (tests/envelope_model.py),
their bit guarantees across batch layouts, ``fit_envelope`` end to end on six voices of known envelope, and
``match_audio.py --envelope``."""
import functools
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import envelope_model as vm
import onset_model as om

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32).astype(np.int64)


def _offset_copy(t, off):
    """A contiguous copy of ``t`` whose first element sits ``off`` floats past a 16-byte boundary."""
    flat = torch.zeros(t.numel() + 8, dtype=t.dtype, device=t.device)
    flat[off:off + t.numel()] = t.reshape(-1)
    view = flat[off:off + t.numel()].view(t.shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * off
    return view


# ------------------------------------------------------------------------------------------------ frames
# (B, T, W, hop).  W and hop coprime (blocks of one sample: the direct kernel), W = T (one frame), hop > W (the tile kernel
# with unused blocks between frames), the defaults on one second at 16 kHz (three tiles of 29 frames), blocks of 48 (no
# power of two, two tiles), and a window past the tile's LDS span (the direct kernel with long blocks).
FRAME_CASES = [(3, 4099, 200, 37), (2, 4099, 4099, 64), (3, 4099, 100, 300), (3, 16000, 1024, 256), (2, 16000, 192, 48),
               (1, 20000, 9000, 4500)]


@functools.lru_cache(maxsize=None)
def _frame_inputs(case):
    B, T, _W, _hop = FRAME_CASES[case]
    rng = np.random.default_rng(40 + case)
    x = (rng.standard_normal((B, T)) * np.exp(-np.arange(T) / (0.3 * T))).astype(np.float32)
    if B > 1:
        x[1] = 0.0                                                     # an all-zero row
    x[0, 0], x[0, 1], x[0, T - 1] = np.float32(1e-42), np.float32(1e18), np.float32(-3.0)
    return x


@functools.lru_cache(maxsize=None)
def _frame_kernel(case):
    from inverse_audio_synthesis_amd.envelope import envelope_frames
    _B, _T, W, hop = FRAME_CASES[case]
    rms = envelope_frames(torch.from_numpy(_frame_inputs(case)).cuda(), W, hop)
    torch.cuda.synchronize()
    return rms.cpu().numpy()


@pytest.mark.parametrize("case", range(len(FRAME_CASES)))
def test_frames_match_the_model(lib, dev, case):
    """rms within 1 fp32 ulp of the model: the fp64 sums are the same chains, so only the device's fp64 root can move the
    one rounding to fp32.  A row of zeros gives +0."""
    B, T, W, hop = FRAME_CASES[case]
    got, want = _frame_kernel(case), vm.frames(_frame_inputs(case), W, hop)
    assert got.shape == want.shape == (B, (T - W) // hop + 1)
    ulps = np.abs(_bits(got) - _bits(want))
    print(f"frames {FRAME_CASES[case]}: {int((ulps > 0).sum())} of {ulps.size} values differ, at most {int(ulps.max())} ulp")
    assert np.isfinite(got).all() and ulps.max() <= 1
    if B > 1:
        assert (_bits(got[1]) == 0).all()


@pytest.mark.parametrize("case", range(len(FRAME_CASES)))
def test_frames_bits_do_not_depend_on_the_batch_layout(lib, dev, case):
    from inverse_audio_synthesis_amd.envelope import envelope_frames
    B, T, W, hop = FRAME_CASES[case]
    x = torch.from_numpy(_frame_inputs(case)).cuda()
    ref = _bits(_frame_kernel(case))
    perm = list(range(B))[::-1]
    assert (_bits(envelope_frames(x[perm].contiguous(), W, hop).cpu().numpy()) == ref[perm]).all()
    padded = torch.cat([torch.ones((2, T), device=x.device), x, torch.full((1, T), 0.5, device=x.device)])
    assert (_bits(envelope_frames(padded, W, hop).cpu().numpy())[2:2 + B] == ref).all()
    for off in (1, 2, 3):
        assert (_bits(envelope_frames(_offset_copy(x, off), W, hop).cpu().numpy()) == ref).all(), off
    for b in range(B):                                                 # a row alone, at whatever phase it has in the batch
        assert (_bits(envelope_frames(x[b:b + 1], W, hop).cpu().numpy())[0] == ref[b]).all(), b


# ------------------------------------------------------------------------------------------------ score
N_SOUNDS = 3
SCORE_F = (1, 45, 1000)
# u = 0 in attack, decay and release; sustain 0 and 1; duration below attack; duration beyond the last frame (4 s);
# alpha at both ends; everything 0 (a note over before the first frame: the model is 0 everywhere) and everything 1
CRAFTED = [(0.5, 0.0, 0.0, 0.5, 0.0, 0.5), (0.5, 0.2, 0.3, 0.0, 0.3, 0.5), (0.5, 0.2, 0.3, 1.0, 0.3, 0.5),
           (0.1, 0.8, 0.3, 0.5, 0.3, 0.5), (1.0, 0.3, 0.3, 0.5, 0.3, 0.5), (0.5, 0.3, 0.3, 0.5, 0.3, 0.0),
           (0.5, 0.3, 0.3, 0.5, 0.3, 1.0), (0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0, 1.0, 1.0),
           (0.3, 0.0, 0.4, 0.2, 0.5, 0.2), (0.3, 0.4, 0.0, 0.2, 0.0, 0.7), (0.2, 0.2, 0.0, 0.6, 0.2, 0.1)]
M_LARGE = 70
SINGLE = 9                                                             # the candidate of the M = 1 runs


def _times(F):
    """(t0, dt): 1000 frames cover 4 s, 45 frames 0.74 s, one frame sits at 0.1 s."""
    return {1: (0.1, 0.01), 45: (0.032, 0.016), 1000: (0.008, 0.004)}[F]


@functools.lru_cache(maxsize=None)
def _score_inputs(F):
    """-> (env [3, F], cand [3, 70, 6]): row 0 the law of a candidate at a gain (as fp32), row 1 silence, row 2 noise with
    one NaN; per sound the crafted candidates first, then uniform ones of its own."""
    rng = np.random.default_rng(60 + F)
    cand = rng.random((N_SOUNDS, M_LARGE, 6)).astype(np.float32)
    cand[:, :len(CRAFTED)] = np.asarray(CRAFTED, dtype=np.float32)
    t0, dt = _times(F)
    src = np.array([0.45, 0.25, 0.35, 0.4, 0.3, 0.3], dtype=np.float32)
    env = np.empty((N_SOUNDS, F), dtype=np.float32)
    env[0] = (0.37 * np.array([vm.law(src, t0 + f * dt) for f in range(F)])).astype(np.float32)
    env[1] = 0.0
    env[2] = rng.random(F).astype(np.float32)
    env[2, F // 2] = np.nan
    return env, cand


@functools.lru_cache(maxsize=None)
def _score_kernel(F, M):
    from inverse_audio_synthesis_amd.envelope import envelope_score
    env, cand = _score_inputs(F)
    cand = cand if M == M_LARGE else cand[:, SINGLE:SINGLE + 1]
    t0, dt = _times(F)
    d = envelope_score(torch.from_numpy(env).cuda(), torch.from_numpy(np.ascontiguousarray(cand)).cuda(), t0, dt)
    torch.cuda.synchronize()
    return d.cpu().numpy()


@pytest.mark.parametrize("F", SCORE_F)
@pytest.mark.parametrize("M", (1, M_LARGE))
def test_score_matches_the_model(lib, dev, F, M):
    """dist within 1 fp32 ulp of fp32(model), or within 1e-12 absolute where 1 - ratio cancels near 0; silence scores
    exactly 1 and the row with a NaN is NaN."""
    env, cand = _score_inputs(F)
    cand = cand if M == M_LARGE else cand[:, SINGLE:SINGLE + 1]
    got, want = _score_kernel(F, M), vm.score(env, cand, *_times(F))
    assert got.shape == want.shape == (N_SOUNDS, M)
    assert (got[1] == 1.0).all() and (want[1] == 1.0).all()
    assert np.isnan(got[2]).all() and np.isnan(want[2]).all()
    ulps = np.abs(_bits(got[0]) - _bits(want[0]))
    diff = np.abs(got[0].astype(np.float64) - want[0].astype(np.float64))
    ok = (ulps <= 1) | (diff <= 1e-12)
    print(f"score F = {F}, M = {M}: {int((ulps > 0).sum())} of {M} differ, at most {int(ulps.max())} ulp, "
          f"{float(diff.max()):.3e} absolute; distances {float(got[0].min()):.3e} .. {float(got[0].max()):.3e}")
    assert (got[0] >= 0.0).all() and (got[0] <= 1.0).all()
    assert ok.all(), (np.flatnonzero(~ok), got[0][~ok], want[0][~ok])
    if M == M_LARGE and F > 1:
        assert got[0, 7] == 1.0                                        # the note that is over before the first frame


@pytest.mark.parametrize("F", SCORE_F)
def test_topk_merge_ranks_the_scores_as_the_model_does(lib, dev, F):
    from inverse_audio_synthesis_amd.retrieval import EMPTY_INDEX, rank_distances, topk_merge
    d = torch.from_numpy(_score_kernel(F, M_LARGE)).cuda()
    k = 16
    best = torch.full((N_SOUNDS, k), float("inf"), dtype=torch.float32, device=d.device)
    idx = torch.full((N_SOUNDS, k), EMPTY_INDEX, dtype=torch.int64, device=d.device)
    topk_merge(d, 0, best, idx)
    want = rank_distances(d)[:, :k]
    assert torch.equal(idx, want)
    assert (_bits(best.cpu().numpy()) == _bits(torch.gather(d, 1, want).cpu().numpy())).all()
    assert idx[2].tolist() == list(range(k))                           # the NaN row: by index


@pytest.mark.parametrize("F", SCORE_F)
def test_score_bits_do_not_depend_on_the_layout(lib, dev, F):
    from inverse_audio_synthesis_amd.envelope import envelope_score
    env_h, cand_h = _score_inputs(F)
    env, cand = torch.from_numpy(env_h).cuda(), torch.from_numpy(cand_h).cuda()
    t0, dt = _times(F)
    ref = _bits(_score_kernel(F, M_LARGE))
    assert (_bits(_score_kernel(F, 1))[:, 0] == ref[:, SINGLE]).all()   # across both M
    perm = np.random.default_rng(5).permutation(M_LARGE)               # wherever it sits in M (across the 64-lane tile)
    got = envelope_score(env, cand[:, torch.from_numpy(perm).cuda()].contiguous(), t0, dt)
    assert (_bits(got.cpu().numpy()) == ref[:, perm]).all()
    rows = [2, 0, 1]
    got = envelope_score(env[rows].contiguous(), cand[rows].contiguous(), t0, dt)
    assert (_bits(got.cpu().numpy()) == ref[rows]).all()
    pad_e = torch.cat([torch.ones((2, F), device=env.device), env])    # batch padding
    pad_c = torch.cat([torch.full((2, M_LARGE, 6), 0.25, device=env.device), cand])
    assert (_bits(envelope_score(pad_e, pad_c, t0, dt).cpu().numpy())[2:] == ref).all()
    for off in (1, 2, 3):
        assert (_bits(envelope_score(_offset_copy(env, off), cand, t0, dt).cpu().numpy()) == ref).all(), off


def test_refusals_leave_the_outputs_alone(lib, dev):
    """Every refusal returns its code and launches nothing: the outputs keep their sentinel."""
    import ctypes
    from inverse_audio_synthesis_amd import _lib
    x = torch.zeros((2, 1000), device=dev)
    rms = torch.full((2, 16), -7.0, device=dev)
    env = torch.zeros((2, 16), device=dev)
    cand = torch.full((2, 4, 6), 0.5, device=dev)
    dist = torch.full((2, 4), -7.0, device=dev)
    P, st = _lib.ptr, _lib.stream()

    def frames(audio=P(x), B=2, T=1000, W=100, hop=60, out=P(rms)):
        return lib.ias_envelope_frames(audio, B, T, W, hop, out, st)

    def score(e=P(env), c=P(cand), N=2, M=4, F=16, t0=0.01, dt=0.01, out=P(dist)):
        return lib.ias_envelope_score(e, c, N, M, F, t0, dt, out, st)
    for kw in (dict(audio=None), dict(out=None), dict(B=0), dict(T=0), dict(W=0), dict(hop=0), dict(hop=-1), dict(W=1001),
               dict(B=-2)):
        assert frames(**kw) == -1, kw
    assert frames(B=65536) == -2
    nan, inf = float("nan"), float("inf")
    for kw in (dict(e=None), dict(c=None), dict(out=None), dict(N=0), dict(M=0), dict(F=0), dict(dt=0.0), dict(dt=-0.01),
               dict(dt=nan), dict(dt=inf), dict(t0=nan), dict(t0=inf)):
        assert score(**kw) == -1, kw
    assert score(F=16385) == -2 and score(N=65536) == -2 and score(N=65536, dt=0.0) == -1
    torch.cuda.synchronize()
    assert (rms == -7.0).all() and (dist == -7.0).all()
    assert frames() == 0 and score() == 0
    torch.cuda.synchronize()
    assert (rms == 0.0).all() and (dist == 1.0).all()                  # F = (1000 - 100) // 60 + 1 = 16 frames of silence


def test_wrappers_refuse_what_the_kernels_refuse(lib, dev):
    from inverse_audio_synthesis_amd.envelope import envelope_frames, envelope_score
    x = torch.zeros((2, 1000), device=dev)
    for bad in (lambda: envelope_frames(x, 1001, 10), lambda: envelope_frames(x, 0, 10), lambda: envelope_frames(x, 10, 0),
                lambda: envelope_frames(x.double(), 10, 10), lambda: envelope_frames(x[:, ::2], 10, 10),
                lambda: envelope_frames(x[0], 10, 10)):
        with pytest.raises(ValueError):
            bad()
    env, cand = torch.ones((2, 16), device=dev), torch.full((2, 4, 6), 0.5, device=dev)
    for bad in (lambda: envelope_score(env, cand[:1], 0.0, 0.01), lambda: envelope_score(env, cand[..., :5], 0.0, 0.01),
                lambda: envelope_score(env, cand, 0.0, 0.0), lambda: envelope_score(env, cand, float("nan"), 0.01),
                lambda: envelope_score(torch.ones((2, 16385), device=dev), cand, 0.0, 0.01),
                lambda: envelope_score(env, cand, 0.0, 0.01, out=torch.empty((2, 5), device=dev))):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------ the whole stage
@functools.lru_cache(maxsize=None)
def _voice_fit():
    """The six voices of tests/envelope_model.py (routes zeroed) rendered by the HIP Voice and fitted twice."""
    from inverse_audio_synthesis_amd.envelope import fit_envelope
    from inverse_audio_synthesis_amd.voice import SynthConfig, Voice
    voice = Voice(SynthConfig(batch_size=len(vm.VOICES), sample_rate=vm.RATE, buffer_size_seconds=vm.SECONDS,
                              reproducible=False)).cuda()
    target = voice.render(vm.voice_params01(True).cuda()).detach().clone()
    fits = [fit_envelope(target, vm.RATE, W=vm.W, hop=vm.HOP, seed=0) for _ in range(2)]
    return voice, target, fits


def test_fit_envelope_on_the_six_voices(lib, dev):
    """The bounds of tests/test_envelope_cpu.py hold for the kernels on the HIP Voice's renders, and a seed fixes the bits."""
    _voice, _target, (fit, again) = _voice_fit()
    dist, start = fit.dist.cpu().numpy(), fit.start_dist.cpu().numpy()
    for n in range(len(vm.VOICES)):
        print(f"voice {n + 1}: distance {start[n]:.4g} -> {dist[n]:.4g} ({start[n] / dist[n]:.1f}x), units "
              + ", ".join(f"{v:.4g}" for v in fit.units[n].tolist()))
    for a, b in ((fit.params01, again.params01), (fit.dist, again.dist), (fit.start_dist, again.start_dist),
                 (fit.rms, again.rms)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert fit.sounding.all() and fit.params01.shape == (6, 6) and fit.units.dtype == torch.float64
    assert (dist <= start / 5.0).all(), (dist, start)
    assert (dist <= vm.DIST_BOUND).all(), dist
    err = np.abs(fit.units[:2, 0].cpu().numpy() - np.array([vm.VOICES[0][0], vm.VOICES[1][0]]))
    print(f"duration errors of voices 1 and 2: {err[0]:.4f} s, {err[1]:.4f} s")
    assert (err <= min(vm.DURATION_BOUND, 0.05)).all(), err


def test_the_reshaped_centre_renders_the_fitted_envelope(lib, dev):
    """With the LFO routes and the noise at zero the render is the model: the centre voice ``reshape``d by the fit and
    rendered has an RMS envelope (the fit's own frames) within the same bound of the target's."""
    from inverse_audio_synthesis_amd import voice_spec as S
    from inverse_audio_synthesis_amd.envelope import envelope_frames, reshape
    voice, _target, (fit, _again) = _voice_fit()
    centre = torch.full((len(vm.VOICES), S.NPARAMS), 0.5, device=dev)
    centre[:, S.INDEX[("mixer", "noise")]] = 0.0
    for lfo in ("lfo_1", "lfo_2"):
        for o in S.MOD_OUTPUTS:
            centre[:, S.INDEX[("mod_matrix", f"{lfo}->{o}")]] = 0.0
    shaped = reshape(centre, fit)
    assert int((shaped != centre).sum()) == 11 * len(vm.VOICES)
    a = envelope_frames(voice.render(shaped).detach().contiguous(), vm.W, vm.HOP).double().cpu().numpy()
    b = fit.rms.double().cpu().numpy()
    d = 1.0 - (a * b).sum(1) ** 2 / ((a * a).sum(1) * (b * b).sum(1))
    print("distance of the reshaped centre's envelope to the target's: " + ", ".join(f"{v:.4g}" for v in d))
    assert (d <= vm.DIST_BOUND).all(), d


# ------------------------------------------------------------------------------------------------ match_audio.py
RATE = 16000


def _write_pcm16(path, x, rate):
    pcm = np.clip(np.round(np.asarray(x, dtype=np.float64) * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.tobytes())


def _match_audio(tmp_path, name, *flags):
    from conftest import ROOT
    wav = tmp_path / "phrase.wav"
    if not wav.exists():
        _write_pcm16(wav, om.detector_rows(RATE)[0], RATE)             # the four notes of tests/test_onset_gpu.py
    out = tmp_path / name
    cmd = [sys.executable, os.path.join(ROOT, "match_audio.py"), str(wav), "torchsynth.rate=16000",
           "torchsynth.buffer_size_seconds=1.0", "--steps", "2", "--out", str(out), *flags]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:]
    return out


def test_match_audio_envelope_entry_point(lib, dev, tmp_path):
    doc = json.load(open(_match_audio(tmp_path, "with", "--envelope", "--split", "--pitch") / "phrase.notes.json"))
    assert len(doc["notes"]) == 4
    for note in doc["notes"]:
        e = note["envelope"]
        assert sorted(e) == sorted(["sounding", "distance", "start_distance"] + list(vm.COLUMNS))
        print(f"note at {note['onset_sample']}: distance {e['start_distance']:.4g} -> {e['distance']:.4g}, duration "
              f"{e['duration']:.3f} s")
        assert e["sounding"] is True and 0.0 <= e["distance"] < e["start_distance"] <= 1.0
        assert 0.01 <= e["duration"] <= 4.0 and 0.1 <= e["alpha"] <= 6.0 and note["voiced"] is True
        by_name = {(p["module"], p["name"]): p for p in note["params"]}
        assert len(by_name) == 78
    plain = json.load(open(_match_audio(tmp_path, "without", "--split", "--pitch") / "phrase.notes.json"))
    assert len(plain["notes"]) == 4 and all("envelope" not in note for note in plain["notes"])

"""The envelope stage without a GPU: ``envelope.fit_envelope`` run with the fp64 model of its kernels (tests/envelope_model.py)
on six oracle voices of known envelope, ``reshape``, the 0..1 -> units maps and the new ``match_audio.py`` flags."""
import functools

import numpy as np
import pytest
import torch

import envelope_model as vm

from envelope_model import DIST_BOUND, DURATION_BOUND, HOP, RATE, SECONDS, VOICES, W, voice_params01


@functools.lru_cache(maxsize=None)
def oracle_fit(routes_zeroed):
    """The six voices rendered by the oracle and fitted by the model search at the defaults -> ``EnvelopeFit``."""
    from oracle import synth_oracle as so
    from inverse_audio_synthesis_amd.envelope import fit_envelope
    cfg = so.VoiceConfig(batch_size=len(VOICES), sample_rate=RATE, buffer_size_seconds=SECONDS)
    audio = so.render_from_params01(cfg, voice_params01(routes_zeroed), so.make_noise(cfg))
    return fit_envelope(audio, RATE, W=W, hop=HOP, ops=vm.MODEL_OPS)


def test_six_voices_with_the_routes_zeroed():
    fit = oracle_fit(True)
    dist, start = fit.dist.numpy(), fit.start_dist.numpy()
    for n in range(len(VOICES)):
        print(f"voice {n + 1}: distance {start[n]:.4g} -> {dist[n]:.4g} ({start[n] / dist[n]:.1f}x), units "
              + ", ".join(f"{v:.4g}" for v in fit.units[n].tolist()))
    assert fit.sounding.all()
    assert (dist <= start / 5.0).all(), (dist, start)
    assert (dist <= DIST_BOUND).all(), dist
    err = np.abs(fit.units[:2, 0].numpy() - np.array([VOICES[0][0], VOICES[1][0]]))
    print(f"duration errors of voices 1 and 2: {err[0]:.4f} s, {err[1]:.4f} s")
    assert (err <= min(DURATION_BOUND, 0.05)).all(), err
    # the start is candidate 0: the model scores the centre the same outside the search
    centre = np.full((len(VOICES), 1, 6), 0.5, dtype=np.float32)
    again = vm.score(fit.rms.numpy(), centre, (W / 2.0) / RATE, HOP / RATE)[:, 0]
    assert (again.view(np.uint32) == start.view(np.uint32)).all()


def test_six_voices_with_the_routes_at_the_centre():
    """The LFOs then shape the amplitude too, which the law cannot follow: the distance still falls for every sound.
    Measured ratios start / final: 17.0, 8.1, 15.9, 2.5, 13.3, 27.1 (final distances 7.8e-3 .. 5.8e-2)."""
    fit = oracle_fit(False)
    dist, start = fit.dist.numpy(), fit.start_dist.numpy()
    for n in range(len(VOICES)):
        print(f"voice {n + 1}: distance {start[n]:.4g} -> {dist[n]:.4g} ({start[n] / dist[n]:.1f}x)")
    assert fit.sounding.all() and (dist < start).all(), (dist, start)


def test_the_same_seed_gives_the_same_bits_and_another_seed_does_not():
    from inverse_audio_synthesis_amd.envelope import fit_envelope
    t = np.arange(4000) / 8000.0
    audio = torch.from_numpy((np.sin(2 * np.pi * 220.0 * t) * np.exp(-t / 0.1)).astype(np.float32)).reshape(1, -1)
    kw = dict(W=256, hop=64, generations=3, population=32, elites=4, ops=vm.MODEL_OPS)
    a, b, c = fit_envelope(audio, 8000, seed=5, **kw), fit_envelope(audio, 8000, seed=5, **kw), \
        fit_envelope(audio, 8000, seed=6, **kw)
    assert torch.equal(a.params01, b.params01) and torch.equal(a.dist, b.dist)
    assert not torch.equal(a.params01, c.params01)
    assert (a.dist <= a.start_dist).all()


def test_a_silent_sound_is_not_sounding_and_scores_one():
    from inverse_audio_synthesis_amd.envelope import fit_envelope
    audio = torch.zeros((2, 2000), dtype=torch.float32)
    audio[1, 100:900] = 0.25
    fit = fit_envelope(audio, 8000, W=256, hop=64, generations=2, population=16, elites=4, ops=vm.MODEL_OPS)
    assert fit.sounding.tolist() == [False, True]
    assert float(fit.dist[0]) == 1.0 and float(fit.start_dist[0]) == 1.0 and float(fit.dist[1]) < 1.0


def test_fit_envelope_refusals():
    from inverse_audio_synthesis_amd.envelope import fit_envelope
    audio = torch.zeros((2, 2000), dtype=torch.float32)
    for kw in (dict(generations=0), dict(population=0), dict(elites=0), dict(elites=65, population=128),
               dict(elites=17, population=16), dict(sigma0=float("inf")), dict(sigma_min=0.6), dict(alpha=1.5),
               dict(init01=torch.zeros((3, 6))), dict(init01=torch.zeros((2, 5)))):
        with pytest.raises(ValueError):
            fit_envelope(audio, 8000, W=256, hop=64, ops=vm.MODEL_OPS, **kw)
    with pytest.raises(ValueError):
        fit_envelope(audio[0], 8000, ops=vm.MODEL_OPS)


# ------------------------------------------------------------------------------------------------ reshape and the maps
def _fit_of(params01, sounding):
    from inverse_audio_synthesis_amd.envelope import EnvelopeFit, to_units
    n = params01.shape[0]
    return EnvelopeFit(params01=params01, dist=torch.zeros(n), start_dist=torch.ones(n), sounding=sounding,
                       units=to_units(params01), rms=torch.ones((n, 3)))


def test_reshape_moves_eleven_columns_and_keeps_silent_rows():
    from inverse_audio_synthesis_amd import voice_spec as S
    from inverse_audio_synthesis_amd.envelope import reshape
    g = torch.Generator().manual_seed(3)
    p = torch.rand((3, S.NPARAMS), generator=g)
    p[0, 5] = float("nan")                                # bits, not values, are kept
    fit = _fit_of(torch.rand((3, 6), generator=g), torch.tensor([True, False, True]))
    out = reshape(p, fit)
    want = vm.reshape(p.numpy(), fit.params01.numpy(), fit.sounding.numpy())
    assert (out.numpy().view(np.uint32) == want.view(np.uint32)).all()
    moved = (out.view(torch.int32) != p.view(torch.int32))
    cols = sorted([S.INDEX[("keyboard", "duration")]] + [S.INDEX[(m, n)] for m in ("adsr_1", "adsr_2")
                                                          for n in vm.COLUMNS[1:]])
    assert len(cols) == 11
    assert moved[0].nonzero().flatten().tolist() == cols and moved[2].nonzero().flatten().tolist() == cols
    assert not moved[1].any() and not moved[:, [c for c in range(S.NPARAMS) if c not in cols]].any()
    assert out is not p and out.data_ptr() != p.data_ptr()

    p3 = torch.rand((3, 4, S.NPARAMS), generator=g)
    out3 = reshape(p3, fit)
    want3 = vm.reshape(p3.numpy(), fit.params01.numpy(), fit.sounding.numpy())
    assert (out3.numpy().view(np.uint32) == want3.view(np.uint32)).all()
    assert torch.equal(out3[1], p3[1]) and not torch.equal(out3[0], p3[0])


def test_reshape_refuses_mismatched_shapes():
    from inverse_audio_synthesis_amd import voice_spec as S
    from inverse_audio_synthesis_amd.envelope import reshape
    fit = _fit_of(torch.rand((3, 6)), torch.ones(3, dtype=torch.bool))
    for bad in (torch.zeros((2, S.NPARAMS)), torch.zeros((3, S.NPARAMS - 1)), torch.zeros(S.NPARAMS),
                torch.zeros((4, 2, S.NPARAMS))):
        with pytest.raises(ValueError):
            reshape(bad, fit)


def test_units_equal_the_voice_table():
    """The squares and lines of ias_envelope_score are ``voice_grad._from_0to1`` (exp2(log2(u) / curve)) on those columns:
    fp64 against fp64, so only the rounding of exp2 and log2 separates them."""
    from inverse_audio_synthesis_amd import voice_spec as S
    from inverse_audio_synthesis_amd.envelope import to_units
    from inverse_audio_synthesis_amd.voice_grad import _from_0to1
    u = torch.rand((64, 6), generator=torch.Generator().manual_seed(1))
    u[0], u[1] = 0.0, 1.0
    for mod in ("adsr_1", "adsr_2"):
        p = torch.full((64, S.NPARAMS), 0.5, dtype=torch.float64)
        p[:, S.INDEX[("keyboard", "duration")]] = u[:, 0].double()
        for j, name in enumerate(vm.COLUMNS[1:], start=1):
            p[:, S.INDEX[(mod, name)]] = u[:, j].double()
        table = _from_0to1(p)
        cols = [S.INDEX[("keyboard", "duration")]] + [S.INDEX[(mod, name)] for name in vm.COLUMNS[1:]]
        assert torch.allclose(to_units(u), table[:, cols], rtol=1e-13, atol=1e-15)
    model = np.stack(vm.to_units(u.numpy()), axis=-1)
    assert (model == to_units(u).numpy()).all()
    for (name, lo, hi, curve, sym) in S._ADSR:
        assert curve in (0.5, 1.0) and not sym
    assert S.PARAMS[S.INDEX[("keyboard", "duration")]][2:] == (0.01, 4.0, 0.5, False)


# ------------------------------------------------------------------------------------------------ the model itself
def test_model_frames_and_score_basics():
    """The model the GPU tests lean on: a constant row has its own level as rms whatever the blocks, the law reproduces
    itself with distance 0 at any gain, and the order of the frame sum is the contract's (gcd blocks)."""
    x = np.full((1, 1000), 0.5, dtype=np.float32)
    for w, hop in ((200, 37), (256, 64), (1000, 7), (100, 300)):
        r = vm.frames(x, w, hop)
        assert r.shape == (1, vm.num_frames(1000, w, hop)) and (r == np.float32(0.5)).all()
    cand = np.random.default_rng(0).random((1, 5, 6)).astype(np.float32)
    t0, dt = 0.016, 0.008
    env = np.stack([vm.law(cand[0, 2], t0 + f * dt) for f in range(200)]).astype(np.float32)[None] * np.float32(3.0)
    d = vm.score(env, cand, t0, dt)
    assert d[0, 2] < 1e-12 and (d >= 0.0).all() and (d <= 1.0).all()


def test_kernels_refuse_before_touching_the_device(lib):
    """Every refusal is decided on the host from the arguments alone: the pointers are never followed, nothing is launched,
    no GPU is needed."""
    import ctypes
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.ias_envelope_num_frames(1024, 1024, 256) == 1 and lib.ias_envelope_num_frames(1279, 1024, 256) == 1
    assert lib.ias_envelope_num_frames(1280, 1024, 256) == 2 and lib.ias_envelope_num_frames(176400, 1024, 256) == 686
    assert lib.ias_envelope_num_frames(4099, 100, 300) == 14 and lib.ias_envelope_num_frames(2 ** 31 - 1, 1, 1) == 2 ** 31 - 1
    for a in ((1023, 1024, 256), (0, 1, 1), (100, 0, 10), (100, 10, 0), (-5, 1, 1), (100, 10, -1)):
        assert lib.ias_envelope_num_frames(*a) == -1, a

    def frames(audio=p, B=2, T=1000, W=100, hop=60, out=p):
        return lib.ias_envelope_frames(audio, B, T, W, hop, out, None)

    def score(e=p, c=p, N=2, M=4, F=16, t0=0.01, dt=0.01, out=p):
        return lib.ias_envelope_score(e, c, N, M, F, t0, dt, out, None)
    for kw in (dict(audio=None), dict(out=None), dict(B=0), dict(B=-2), dict(T=0), dict(W=0), dict(hop=0), dict(hop=-1),
               dict(W=1001), dict(B=65536, W=0)):
        assert frames(**kw) == -1, kw
    assert frames(B=65536) == -2
    nan, inf = float("nan"), float("inf")
    for kw in (dict(e=None), dict(c=None), dict(out=None), dict(N=0), dict(M=0), dict(F=0), dict(F=-1), dict(dt=0.0),
               dict(dt=-0.01), dict(dt=nan), dict(dt=inf), dict(t0=nan), dict(t0=-inf), dict(N=65536, dt=0.0)):
        assert score(**kw) == -1, kw
    # the LDS budget: a row of env, 4 F <= 65536 bytes
    from inverse_audio_synthesis_amd.envelope import LDS_BUDGET_BYTES
    assert LDS_BUDGET_BYTES == 65536
    assert score(F=16385) == -2 and score(F=2 ** 31 - 1) == -2 and score(N=65536) == -2


# ------------------------------------------------------------------------------------------------ match_audio.py flags
def test_match_audio_envelope_flags():
    import match_audio
    args, _f, _o = match_audio.parse_args(["a.wav", "--out", "o"])
    assert args.envelope is False and args.envelope_generations == 16 and args.envelope_population == 512
    args, _f, _o = match_audio.parse_args(["a.wav", "--out", "o", "--envelope", "--envelope-generations", "4",
                                          "--envelope-population", "100", "--split", "--pitch"])
    assert args.envelope is True and args.envelope_generations == 4 and args.envelope_population == 100


@pytest.mark.parametrize("argv", [["--envelope-generations", "0"], ["--envelope-population", "15"],
                                  ["--envelope-population", "0"], ["--envelope-generations", "x"],
                                  ["--envelope-population", str(1 << 30), "--envelope-generations", "4"]])
def test_match_audio_refuses_bad_envelope_flags(argv):
    import match_audio
    with pytest.raises(SystemExit):
        match_audio.parse_args(["a.wav", "--out", "o", "--envelope"] + argv)

"""Evolutionary search stage without a GPU: the restated Philox4x32-10 against the Random123 known-answer vectors, the
declared entry points, their host-side refusals, match_audio.py's --evolve flags, evolve_search's own refusals, and the
search loop itself (``evolve.cross_entropy_search``) run on the numpy primitives of tests/evolve_model.py."""
import ctypes
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT

import evolve_model as em

# Random123's kat_vectors for philox4x32 with 10 rounds: counter, key -> output
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("counter,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_model_philox_reproduces_random123(counter, key, want):
    got = em.philox4x32_10(counter, key)
    assert tuple(int(x) for x in got) == want
    # vectorised over a counter array: the same words at every position
    arr = em.philox4x32_10([np.full((2, 3), c, dtype=np.uint64) for c in counter], key)
    for a, w in zip(arr, want):
        assert a.shape == (2, 3) and (a == w).all()


def test_model_unit_and_normals():
    assert em.unit(0) == 2.0 ** -24 and em.unit(0xffffffff) == 1.0 - 2.0 ** -24
    u = em.unit(np.array([0x12345678, 0x80000000], dtype=np.uint64))
    assert (u.astype(np.float32).astype(np.float64) == u).all()          # exact in fp32
    z = em.normals(4, 5000, 7, 0, 0, 3, 1)
    assert abs(z.mean()) < 0.02 and abs(z.var() - 1.0) < 0.02 and np.abs(z).max() <= 5.77
    # the cut: rows and candidates are named by their global position
    assert np.array_equal(em.normals(1, 3, 7, 2, 11, 3, 1), z[2:3, 11:14])
    assert not np.array_equal(em.normals(4, 5000, 7, 0, 0, 4, 1), z)


SAMPLE_ARGS = ["const float* mean", "const float* sigma", "const unsigned char* free_cols", "int N", "int M", "int P",
               "int n_base", "long long m_base", "unsigned long long seed", "long long generation", "float* out",
               "void* stream"]
UPDATE_ARGS = ["const float* pop", "long long base", "int M", "const float* elite_dist", "const long long* elite_idx",
               "const long long* prev_idx", "const float* prev_params", "float* elite_params", "float* mean", "float* sigma",
               "const unsigned char* free_cols", "int N", "int k", "int P", "double alpha", "double sigma_min",
               "double sigma_max", "void* stream"]


@pytest.mark.parametrize("name,want", [("ias_evolve_sample", SAMPLE_ARGS), ("ias_evolve_update", UPDATE_ARGS)])
def test_header_declares_the_entry_points(name, want):
    text = open(os.path.join(ROOT, "include", "ias_hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"include/ias_hip.h does not declare {name}"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == want


def _host_pointer():
    buf = (ctypes.c_char * 64)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_sample_refuses_before_touching_the_device(lib):
    """Every refusal is decided on the host from the arguments alone (the pointers are never followed)."""
    _buf, p = _host_pointer()

    def call(mean=p, sigma=p, free=p, N=2, M=3, P=5, n_base=0, m_base=0, seed=1, generation=0, out=p):
        return lib.ias_evolve_sample(mean, sigma, free, N, M, P, n_base, m_base, seed, generation, out, None)
    for kw in (dict(mean=None), dict(sigma=None), dict(free=None), dict(out=None), dict(N=0), dict(M=0), dict(P=0),
               dict(P=129), dict(n_base=-1), dict(m_base=-1), dict(generation=-1), dict(N=-3), dict(M=-1)):
        assert call(**kw) == -1, kw
    for kw in (dict(m_base=(1 << 32) - 2), dict(m_base=1 << 40), dict(generation=1 << 32), dict(generation=1 << 40)):
        assert call(**kw) == -2, kw


def test_update_refuses_before_touching_the_device(lib):
    _buf, p = _host_pointer()
    _buf2, p2 = _host_pointer()

    def call(pop=p, base=0, M=3, ed=p, ei=p, pi=p, pp=p, ep=p2, mean=p, sigma=p, free=p, N=2, k=2, P=5, alpha=0.5,
             smin=0.01, smax=0.5):
        return lib.ias_evolve_update(pop, base, M, ed, ei, pi, pp, ep, mean, sigma, free, N, k, P, alpha, smin, smax, None)
    bad = [dict(pop=None), dict(ed=None), dict(ei=None), dict(pi=None), dict(pp=None), dict(ep=None), dict(mean=None),
           dict(sigma=None), dict(free=None), dict(N=0), dict(M=0), dict(k=0), dict(P=0), dict(k=65), dict(P=129),
           dict(base=-1), dict(alpha=-0.01), dict(alpha=1.01), dict(alpha=math.nan), dict(smin=math.nan),
           dict(smax=math.inf), dict(smin=-math.inf), dict(smin=-0.1), dict(smin=0.3, smax=0.2), dict(ep=p)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call(N=65536) == -2


def test_match_audio_accepts_evolve_flags():
    import match_audio
    args, files, _o = match_audio.parse_args(["a.wav", "--out", "o"])
    assert (args.evolve, args.evolve_population, args.evolve_elites, args.evolve_sigma) == (0, 512, 8, 0.2)
    args, files, _o = match_audio.parse_args(["a.wav", "--out", "o", "--init", "bank", "--evolve", "3", "--starts", "4",
                                              "--evolve-population", "256", "--evolve-elites", "4", "--evolve-sigma", "0.1",
                                              "--seed", "7"])
    assert (args.evolve, args.evolve_population, args.evolve_elites, args.evolve_sigma) == (3, 256, 4, 0.1)
    assert args.starts == 4 and args.seed == 7 and files == ["a.wav"]
    # the elites are the starts, so the centre may have several
    args, _f, _o = match_audio.parse_args(["a.wav", "--out", "o", "--evolve", "2", "--starts", "3"])
    assert args.init == "center" and args.starts == 3


@pytest.mark.parametrize("argv", [["--evolve", "-1"], ["--evolve", "2", "--evolve-population", "0"],
                                  ["--evolve", "2", "--evolve-population", "200"],
                                  ["--evolve", "2", "--evolve-population", "-128"],
                                  ["--evolve", "2", "--evolve-elites", "0"], ["--evolve", "2", "--evolve-elites", "65"],
                                  ["--evolve", "2", "--evolve-elites", "4", "--init", "random", "--starts", "5"],
                                  ["--evolve", "2", "--starts", "9"], ["--starts", "3"]])
def test_match_audio_refuses_bad_evolve(argv):
    import match_audio
    with pytest.raises(SystemExit) as e:
        match_audio.parse_args(["a.wav", "--out", "o"] + argv)
    assert e.value.code == 2


def _cpu_voice(B=2):
    from inverse_audio_synthesis_amd.voice import SynthConfig, Voice
    return Voice(SynthConfig(batch_size=B, sample_rate=16000, buffer_size_seconds=1.0))


def test_search_refuses_multi_resolution_loss():
    from inverse_audio_synthesis_amd.match import evolve_search
    from inverse_audio_synthesis_amd.spectral import MultiResolutionSTFTLoss
    with pytest.raises(ValueError, match="mel bank"):
        evolve_search(_cpu_voice(), MultiResolutionSTFTLoss(), target_audio=torch.zeros(1, 16000))


def test_search_refuses_bad_sizes():
    from inverse_audio_synthesis_amd.evolve import evolve_search
    from inverse_audio_synthesis_amd.spectral import STFTL1
    v, loss = _cpu_voice(B=2), STFTL1(n_fft=512, hop_length=128, power=1.0)
    tv = torch.zeros(3, loss.plan.num_frames(16000), loss.plan.n_out)
    for kw in (dict(population=3), dict(population=0), dict(population=-2), dict(generations=0),
               dict(population=1 << 30, generations=4), dict(elites=0), dict(elites=65), dict(population=4, elites=5),
               dict(alpha=1.5), dict(sigma_min=0.3, sigma_max=0.2), dict(sigma0=-1.0),
               dict(init_params01=torch.zeros(2, 78)), dict(init_params01=torch.zeros(3, 5, 78), population=4),
               dict(init_params01=torch.zeros(3, 77))):
        with pytest.raises(ValueError):
            evolve_search(v, loss, target_values=tv, **kw)
    with pytest.raises(ValueError):
        evolve_search(v, loss, target_values=tv[:, :-1])
    with pytest.raises(ValueError):
        evolve_search(v, loss)
    with pytest.raises(ValueError):
        evolve_search(v, loss, target_audio=torch.zeros(1, 16000), target_values=tv)
    with pytest.raises(KeyError):
        evolve_search(v, loss, target_values=tv, frozen=[("mixer", "nothing")])


# ------------------------------------------------------------------------------------------------ the search loop
N, P, M, K, G = 3, 6, 16, 4, 5
HIDDEN = torch.rand((N, P), generator=torch.Generator().manual_seed(40))
SETTINGS = dict(generations=G, population=M, elites=K, sigma0=0.2, alpha=0.7, sigma_min=0.005, sigma_max=0.5)
FIELDS = ("params01", "dist", "idx", "mean", "sigma")


def _score(g, pop, out):
    """Mean |candidate - hidden vector| per sound, in fp64 numpy."""
    d = np.abs(pop.numpy().astype(np.float64) - HIDDEN.numpy().astype(np.float64)[:, None]).mean(-1)
    out.copy_(torch.from_numpy(d.astype(np.float32)))


def _starts(S=1, seed=41):
    return torch.rand((N, S, P), generator=torch.Generator().manual_seed(seed))


def _search(starts=None, free=None, score=_score, seed=3, **kw):
    from inverse_audio_synthesis_amd.evolve import cross_entropy_search
    starts = _starts() if starts is None else starts
    free = torch.ones(starts.shape[2], dtype=torch.uint8) if free is None else free
    return cross_entropy_search(starts, free, score, seed=seed, **{"ops": em.MODEL_OPS, "what": "a_search", **SETTINGS, **kw})


def test_loop_is_a_function_of_its_seed():
    a, b, c = _search(), _search(), _search(seed=4)
    for f in FIELDS + ("history",):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert not torch.equal(a.params01, c.params01) and not torch.equal(a.idx, c.idx)
    assert a.params01.shape == (N, K, P) and a.dist.shape == a.idx.shape == (N, K) and a.idx.dtype == torch.int64
    assert a.mean.shape == a.sigma.shape == (N, P) and ((a.idx >= 0) & (a.idx < G * M)).all()


def test_loop_history_falls_and_ends_at_the_best_elite():
    a = _search()
    assert a.history.shape == (G, N)
    assert (a.history[1:] <= a.history[:-1]).all() and (a.history[-1] < a.history[0]).any()
    assert torch.equal(a.history[-1], a.dist[:, 0])
    assert (a.dist[:, 1:] >= a.dist[:, :-1]).all()
    # every elite's distance is the scorer's value of its parameters
    again = torch.empty((N, K))
    _score(0, a.params01, again)
    assert torch.equal(again, a.dist)


def test_loop_without_history_differs_in_nothing_else():
    a, b = _search(), _search(keep_history=False)
    assert b.history is None
    for f in FIELDS:
        assert torch.equal(getattr(a, f), getattr(b, f)), f


def test_loop_keeps_a_planted_start():
    starts = _starts(S=2)
    starts[:, 1] = HIDDEN
    r = _search(starts=starts)
    assert r.dist[:, 0].tolist() == [0.0] * N and r.idx[:, 0].tolist() == [1] * N
    assert torch.equal(r.params01[:, 0], HIDDEN)
    assert (r.history == 0.0).all()


def test_loop_leaves_frozen_columns_at_start_0():
    starts, free = _starts(), torch.ones(P, dtype=torch.uint8)
    free[1] = free[4] = 0
    r = _search(starts=starts, free=free)
    assert torch.equal(r.params01[:, :, [1, 4]], starts[:, :1, [1, 4]].expand(N, K, 2))
    assert torch.equal(r.mean[:, [1, 4]], starts[:, 0, [1, 4]])
    assert not torch.equal(r.mean[:, [0, 2, 3, 5]], starts[:, 0, [0, 2, 3, 5]])


def _counting(ops):
    """``ops`` with every primitive counted -> (the counting ops, the counts by name)."""
    calls = {name: 0 for name in vars(ops)}

    def counted(name, fn):
        def call(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return call
    return SimpleNamespace(**{name: counted(name, fn) for name, fn in vars(ops).items()}), calls


def test_loop_calls_every_primitive_once_per_generation():
    ops, calls = _counting(em.MODEL_OPS)
    seen = []

    def score(g, pop, out):
        seen.append(g)
        assert tuple(pop.shape) == (N, M, P) and tuple(out.shape) == (N, M)
        _score(g, pop, out)
    _search(score=score, ops=ops)
    assert seen == list(range(G))
    assert calls == {"sample": G, "merge": G, "update": G}


def test_fit_envelope_calls_the_loop_once():
    import envelope_model as vm
    from inverse_audio_synthesis_amd.envelope import fit_envelope
    ops, calls = _counting(vm.MODEL_OPS)
    audio = torch.zeros((2, 2000), dtype=torch.float32)
    audio[:, 100:900] = 0.25
    fit_envelope(audio, 8000, W=256, hop=64, generations=3, population=16, elites=4, ops=ops)
    assert calls == {"frames": 1, "score": 3, "sample": 3, "merge": 3, "update": 3}


@pytest.mark.parametrize("kw", [dict(generations=0), dict(population=0), dict(elites=0), dict(elites=65, population=128),
                                dict(elites=M + 1), dict(sigma0=float("inf")), dict(sigma0=float("nan")),
                                dict(sigma_min=0.6, sigma_max=0.5), dict(alpha=1.5), dict(starts=torch.zeros((0, 1, P)))],
                         ids=lambda kw: "-".join(kw))
def test_loop_refusals_name_the_caller(kw):
    def never(g, pop, out):
        raise AssertionError("scored after a refusal")
    with pytest.raises(ValueError, match="^a_search: "):
        _search(score=never, **kw)

"""Tied sound matching without a GPU: the symbol table of include/ias_hip_tied.h, the fp64 model (tests/tied_model.py)
against the untied rule on singleton groups, ``tie_starts``, ``group_starts`` and the flags of ``match_audio.py --shared``."""
import ctypes
import os

import numpy as np
import pytest
import torch

import tied_model as tm
from conftest import ROOT

_P, _I, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float


# ------------------------------------------------------------------------------------------------ symbols
def test_tied_symbols_and_prototype():
    from inverse_audio_synthesis_amd import _lib
    assert sorted(_lib.TIED_SYMBOLS) == ["ias_match_tied_step"]
    assert not set(_lib.TIED_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.DIAG_SYMBOLS) | set(_lib.REPORT_SYMBOLS))
    assert len(_lib.SYMBOLS) == 120
    # int ias_match_tied_step(params, grad, m, v, best_params, loss, group_start, step, skipped, best_loss, group_loss,
    #                         free_cols, tied_cols, active, N, G, P, update, lr, beta1, beta2, eps, stream)
    assert _lib.TIED_SYMBOLS == {"ias_match_tied_step": (_I, [_P] * 14 + [_I] * 4 + [_F] * 4 + [_P])}


def test_tied_kernel_file_is_compiled_against_its_declaration():
    from test_capi_symbols import _code, _reaches
    path = os.path.join(ROOT, "inverse-audio-synthesis_amd", "csrc", "match_step_kernels.hip")
    assert _reaches(path, os.path.join(ROOT, "include", "ias_hip_tied.h"), set())
    code = _code(path)
    assert 'extern "C" int ias_match_tied_step(' in code and "getenv" not in code and "ias_diag_env" not in code
    assert 'extern "C" int ias_match_adam_step(' in code          # the untied step shares the file and its Adam update
    assert _reaches(path, os.path.join(ROOT, "include", "ias_hip.h"), set())
    makefile = open(os.path.join(ROOT, "inverse-audio-synthesis_amd", "csrc", "Makefile")).read()
    assert "ias_hip_tied.h" in makefile


# ------------------------------------------------------------------------------------------------ the model
def _rule_rows(st, grad, loss, free, active, lr=0.01, betas=(0.9, 0.999), eps=1e-8):
    """``_rule_fp64`` of tests/test_match_gpu.py restated row by row (dict of fp64 CPU tensors, in place)."""
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))     # noqa: E731
    b1, b2, lr, eps = f32(betas[0]), f32(betas[1]), f32(lr), f32(eps)
    cols = free.bool()
    for b in range(grad.shape[0]):
        if not active[b]:
            continue
        if loss[b] < st["best_loss"][b]:
            st["best_params"][b] = st["params01"][b]
            st["best_loss"][b] = loss[b]
        if not torch.isfinite(loss[b]) or not torch.isfinite(grad[b, cols]).all():
            st["skipped"][b] += 1
            continue
        st["step"][b] += 1
        t = int(st["step"][b])
        g = grad[b, cols]
        st["m"][b, cols] = b1 * st["m"][b, cols] + (1 - b1) * g
        st["v"][b, cols] = b2 * st["v"][b, cols] + (1 - b2) * g * g
        denom = st["v"][b, cols].sqrt() / (1 - b2 ** t) ** 0.5 + eps
        st["params01"][b, cols] = (st["params01"][b, cols] - lr / (1 - b1 ** t) * st["m"][b, cols] / denom).clamp(0, 1)


def test_model_with_singleton_groups_is_the_untied_rule():
    N, P = 6, 78
    st = tm.as_fp64(tm.state(N, P, N, seed=1))
    ref = {k: torch.from_numpy(a.copy()) for k, a in st.items()}
    free = np.ones(P, np.uint8)
    free[[0, 5, 40, 77]] = 0
    tied = np.ones(P, np.uint8)
    tied[[1, 30]] = 0                                 # with one row per group tied and own columns are the same thing
    active = np.array([1, 1, 0, 1, 1, 1], np.uint8)
    rng = np.random.default_rng(2)
    for it in range(5):
        grad = rng.standard_normal((N, P)).astype(np.float32)
        loss = (rng.random(N) + (0.0 if it % 2 == 0 else 1.0)).astype(np.float32)
        if it == 2:
            grad[1, 10], grad[3, 5], loss[4] = np.nan, np.inf, np.nan     # free: skip; frozen: ignored; loss: skip
        tm.tied_step(st, grad, loss, np.arange(N + 1), free, tied, active)
        _rule_rows(ref, torch.from_numpy(grad).double(), torch.from_numpy(loss).double(), torch.from_numpy(free),
                   torch.from_numpy(active))
    for k in ("params01", "m", "v", "best_params", "best_loss", "step", "skipped"):
        assert np.array_equal(st[k], ref[k].numpy()), k
    assert st["skipped"].tolist() == [0, 1, 0, 0, 1, 0] and st["step"].tolist() == [5, 4, 0, 5, 4, 5]


def test_model_ties_and_owns():
    """By hand on one group of three rows and three columns (tied, own, frozen), one step from zero moments: Adam's first
    step moves a column by lr sign(g) (eps aside), the tied column by the sign of the MEAN gradient."""
    st = tm.as_fp64(tm.state(3, 3, 1, seed=3))
    st["params01"][:, 0] = [0.5, 0.6, 0.7]            # rows that disagree in a tied column: the first row's value rules
    before = {k: a.copy() for k, a in st.items()}
    grad = np.array([[1.0, -1.0, 9.0], [1.0, 2.0, 9.0], [-5.0, 3.0, np.inf]])
    tm.tied_step(st, grad, [0.3, 0.2, 0.4], [0, 3], free=[1, 1, 0], tied=[1, 0, 1], active=[1], lr=0.01)
    assert np.allclose(st["params01"][:, 0], 0.5 + 0.01, atol=1e-8)            # mean gradient -1: up
    assert np.allclose(st["params01"][:, 1], before["params01"][:, 1] - 0.01 * np.sign(grad[:, 1]), atol=1e-8)
    assert np.array_equal(st["params01"][:, 2], before["params01"][:, 2]) and not st["m"][:, 2].any()
    assert np.allclose(st["m"][:, 0], (1 - tm.f32(0.9)) * -1.0) and st["group_loss"][0] == (0.3 + 0.2 + 0.4) / 3
    assert np.array_equal(st["best_params"], before["params01"]) and st["best_loss"][0] == st["group_loss"][0]
    assert st["step"].tolist() == [1] and st["skipped"].tolist() == [0]


# ------------------------------------------------------------------------------------------------ tie_starts
def test_tie_starts():
    from inverse_audio_synthesis_amd.match import tie_starts
    p = torch.arange(7 * 4, dtype=torch.float32).reshape(7, 4)
    groups = torch.tensor([0, 0, 0, 1, 1, 1, 2])
    tied = torch.tensor([0, 1, 1, 0], dtype=torch.uint8)

    def ref_rows(out):
        rows = out[:, 1].div(4, rounding_mode="floor").long().tolist()     # column 1 of row r holds 4 r + 1
        assert torch.equal(out[:, [0, 3]], p[:, [0, 3]])                   # own columns: left alone
        assert torch.equal(out[:, 1:3], p[rows][:, 1:3])
        return rows

    assert ref_rows(tie_starts(p, groups, tied)) == [0, 0, 0, 3, 3, 3, 6]                 # score=None: the first row
    nan, inf = float("nan"), float("inf")
    score = torch.tensor([3.0, 1.0, 1.0, nan, inf, nan, nan])
    # a tie goes to the lowest row; NaN ranks after +inf; a group of NaN alone keeps its first row
    assert ref_rows(tie_starts(p, groups, tied, score)) == [1, 1, 1, 4, 4, 4, 6]
    assert ref_rows(tie_starts(p, groups, tied, torch.tensor([nan, nan, -1.0, nan, nan, nan, 0.0]))) == [2, 2, 2, 3, 3, 3, 6]
    assert ref_rows(tie_starts(p, groups.int(), tied.bool(), torch.zeros(7))) == [0, 0, 0, 3, 3, 3, 6]
    with pytest.raises(ValueError):
        tie_starts(p, groups[:6], tied)
    with pytest.raises(ValueError):
        tie_starts(p, groups, tied, torch.zeros(6))


# ------------------------------------------------------------------------------------------------ groups
def test_group_starts_and_its_refusals():
    """``fit_tied`` calls ``group_starts(groups, N)`` before it touches the device: its check is tested through it."""
    from inverse_audio_synthesis_amd.match import group_starts
    gs = group_starts(torch.tensor([0, 0, 0, 1, 2, 2], dtype=torch.int32), 6)
    assert gs.dtype == torch.int32 and gs.tolist() == [0, 3, 4, 6]
    assert group_starts(torch.zeros(5, dtype=torch.int64), 5).tolist() == [0, 5]
    assert group_starts([0, 1, 2], 3).tolist() == [0, 1, 2, 3]
    for bad, n in (([0, 1, 0], 3),                   # decreasing
                   ([1, 1, 2], 3),                   # not starting at 0
                   ([0, 0, 1], 4), ([0, 0, 1, 1], 3),    # a wrong length
                   ([0, 2, 2], 3),                   # an id left out: an empty group
                   ([[0, 1]], 2), ([], 0)):
        with pytest.raises(ValueError):
            group_starts(torch.tensor(bad, dtype=torch.int64), n)
    with pytest.raises(ValueError):
        group_starts(torch.tensor([0.0, 1.0]), 2)


def test_tied_mask_and_default_own():
    from inverse_audio_synthesis_amd import match
    from inverse_audio_synthesis_amd import voice_spec as S
    assert match.DEFAULT_OWN == (("keyboard", "midi_f0"), ("keyboard", "duration"))

    class _M:                                        # tied_mask needs the matcher's free mask alone
        free = torch.ones(S.NPARAMS, dtype=torch.uint8)
    _M.free[S.INDEX[("mixer", "noise")]] = 0
    mask = match.SoundMatcher.tied_mask(_M, match.DEFAULT_OWN)
    assert mask.dtype == torch.uint8 and int(mask.sum()) == 75
    assert [i for i in range(S.NPARAMS) if not mask[i]] == [0, 1, S.INDEX[("mixer", "noise")]]
    assert int(match.SoundMatcher.tied_mask(_M, ()).sum()) == 77
    with pytest.raises(KeyError):
        match.SoundMatcher.tied_mask(_M, (("keyboard", "velocity"),))


# ------------------------------------------------------------------------------------------------ match_audio.py flags
def test_match_audio_shared_flags():
    import match_audio
    args, _f, _o = match_audio.parse_args(["a.wav", "--out", "o"])
    assert args.shared is False and args.own == (("keyboard", "midi_f0"), ("keyboard", "duration"))
    args, _f, _o = match_audio.parse_args(["a.wav", "--out", "o", "--split", "--shared"])
    assert args.shared is True and args.own == (("keyboard", "midi_f0"), ("keyboard", "duration"))
    args, _f, _o = match_audio.parse_args(["a.wav", "--out", "o", "--split", "--shared", "--own",
                                          "keyboard.midi_f0, mixer.noise", "--evolve", "2"])
    assert args.own == (("keyboard", "midi_f0"), ("mixer", "noise"))


@pytest.mark.parametrize("argv", [["--shared"], ["--split", "--shared", "--starts", "2", "--init", "random"],
                                  ["--split", "--shared", "--evolve", "2", "--starts", "2"],
                                  ["--split", "--shared", "--own", "keyboard.velocity"],
                                  ["--split", "--shared", "--own", "midi_f0"]],
                         ids=["no-split", "starts", "evolve-starts", "unknown-own", "own-without-module"])
def test_match_audio_refuses_bad_shared_flags(argv):
    import match_audio
    with pytest.raises(SystemExit) as e:
        match_audio.parse_args(["a.wav", "--out", "o"] + argv)
    assert e.value.code == 2

"""Streamed spectral bank search without a GPU: match_audio.py's --bank-stream flag, the declared entry point, its host-side
refusals, and the merge order restated in numpy (tests/evolve_model.py; the reference tests/test_bank_stream_gpu.py leans
on)."""
import math
import os
import re

import pytest
import torch

from conftest import ROOT

import evolve_model as em

INT64_MAX = torch.iinfo(torch.int64).max


def test_match_audio_accepts_bank_stream():
    import match_audio
    args, files, _o = match_audio.parse_args(["a.wav", "--out", "o", "--init", "bank", "--bank-stream", "4"])
    assert args.init == "bank" and args.bank_stream == 4 and files == ["a.wav"]
    args, _f, _o = match_audio.parse_args(["a.wav", "--out", "o", "--init", "bank"])
    assert args.bank_stream is None


@pytest.mark.parametrize("argv", [["--init", "bank", "--bank-stream", "0"], ["--bank-stream", "4", "--init", "random"],
                                  ["--bank-stream", "4"], ["--init", "bank", "--bank-stream", "4", "--starts", "65"]])
def test_match_audio_refuses_bad_bank_stream(argv):
    import match_audio
    with pytest.raises(SystemExit) as e:
        match_audio.parse_args(["a.wav", "--out", "o"] + argv)
    assert e.value.code == 2


def test_header_declares_topk_merge():
    text = open(os.path.join(ROOT, "include", "ias_hip.h")).read()
    m = re.search(r"\bint\s+ias_topk_merge\s*\(([^)]*)\)\s*;", text)
    assert m, "include/ias_hip.h does not declare ias_topk_merge"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const float* dist", "int N", "int M", "long long ld", "long long base", "int k", "float* best_dist",
                    "long long* best_idx", "void* stream"]


def test_topk_merge_refuses_before_touching_the_device(lib):
    """Every refusal is decided on the host from the arguments alone (the pointers are never followed)."""
    import ctypes
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(N=2, M=3, ld=3, base=0, k=2, dist=p, bd=p, bi=p):
        return lib.ias_topk_merge(dist, N, M, ld, base, k, bd, bi, None)
    for kw in (dict(k=0), dict(k=65), dict(N=0), dict(M=0), dict(ld=2), dict(base=-1), dict(dist=None), dict(bd=None),
               dict(bi=None), dict(base=INT64_MAX - 2)):
        assert call(**kw) == -1, kw
    assert call(N=65536) == -2


def _merge(state, block, base):
    """ias_topk_merge as tests/evolve_model.py restates it (the model the search loop's CPU tests run on), on torch tensors:
    the running entries and the block's, ranked by ``rank_distances``' key with ties by GLOBAL index, cut to k."""
    d, i = em.merge(block.numpy(), base, state[0].numpy(), state[1].numpy())
    return torch.from_numpy(d), torch.from_numpy(i)


def _fresh(N, k):
    return torch.full((N, k), math.inf), torch.full((N, k), INT64_MAX, dtype=torch.int64)


@pytest.mark.parametrize("k", [1, 4, 64])
def test_restated_merge_is_associative_and_equals_the_full_sort(k):
    from inverse_audio_synthesis_amd.retrieval import rank_distances
    g = torch.Generator().manual_seed(k)
    N, M = 5, 300
    d = torch.randint(0, 4, (N, M), generator=g).float()
    u = torch.rand((N, M), generator=g)
    d[u < 0.05] = math.nan
    d[u < 0.0333] = math.inf
    d[u < 0.0167] = -math.inf
    want_idx = rank_distances(d)[:, :k]
    want = torch.gather(d, 1, want_idx)
    cuts = [(0, 1), (1, 8), (8, 264), (264, 300)]
    results = []
    for order in ([0, 1, 2, 3], [3, 1, 0, 2], [2, 3, 1, 0]):
        state = _fresh(N, k)
        for j in order:
            a, b = cuts[j]
            state = _merge(state, d[:, a:b], a)
        results.append(state)
    results.append(_merge(_fresh(N, k), d, 0))
    # (A + B) + C == A + (B + C): merging a merged state of two blocks (as a block list would be) changes nothing
    left = _merge(_merge(_merge(_fresh(N, k), d[:, :100], 0), d[:, 100:200], 100), d[:, 200:], 200)
    right = _merge(_merge(_merge(_fresh(N, k), d[:, 200:], 200), d[:, 100:200], 100), d[:, :100], 0)
    results += [left, right]
    for sd, si in results:
        assert torch.equal(si, want_idx)
        assert torch.equal(sd.view(torch.int32), want.view(torch.int32))


def test_restated_merge_keeps_empty_slots_when_candidates_run_out():
    d = torch.tensor([[1.0, math.nan, 1.0]])
    sd, si = _merge(_merge(_fresh(1, 5), d[:, 2:], 2), d[:, :2], 0)
    assert si.tolist() == [[0, 2, 1, INT64_MAX, INT64_MAX]]
    assert sd[0, :2].tolist() == [1.0, 1.0] and math.isnan(sd[0, 2]) and sd[0, 3:].tolist() == [math.inf, math.inf]

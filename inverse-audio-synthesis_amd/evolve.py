"""Evolutionary search stage of sound matching: an elitist cross-entropy search per sound, all state on the device.

The bank search (``retrieval.SpectralBank``) samples the parameter cube without looking at the losses it finds, and the Adam
fit (``match.SoundMatcher``) is purely local; DESIGN.md section 4.6 measured that a larger bank brings the start nearer but
not the final loss lower.  This stage concentrates samples where the loss is already low: per sound it keeps a Gaussian
(mean, sigma per parameter), draws a population from it (ias_evolve_sample), scores it with the matcher's own spectral L1
(``voice.render`` -> ``loss.target`` -> ias_l1_cdist), keeps the k best candidates seen so far (ias_topk_merge: elitist
selection) and refits the Gaussian to them (ias_evolve_update), generation after generation with no host read in between.
Its elites are starts for ``SoundMatcher.fit``.
"""
from dataclasses import dataclass

import torch

from . import _lib
from . import voice_spec as S
from .retrieval import EMPTY_INDEX, Scorer, l1_cdist, topk_merge


@dataclass
class EvolveResult:
    params01: torch.Tensor          # [N, k, 78] the elites in rank order
    dist: torch.Tensor              # [N, k] fp32: their distances (retrieval.rank_distances order)
    idx: torch.Tensor               # [N, k] int64: their global candidate indices g M + m
    mean: torch.Tensor              # [N, 78] the sampling distribution after the last generation
    sigma: torch.Tensor             # [N, 78]
    history: torch.Tensor           # [G, N] fp32: dist[:, 0] after each generation


def _check(t, dtype, shape, what):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous {dtype} tensor of shape {tuple(shape)}, got {t.dtype} "
                         f"{tuple(t.shape)}")


def evolve_sample(mean, sigma, free, seed, generation, out, n_base=0, m_base=0):
    """One launch of ias_evolve_sample (include/ias_hip.h): out [N, M, P] fp32 = clamp(mean + sigma z, 0, 1) on the free
    columns, mean on the frozen ones; z names (seed, generation, n_base + n, m_base + m, column) and nothing else."""
    if out.dim() != 3:
        raise ValueError(f"evolve_sample: out must be [N, M, P], got {tuple(out.shape)}")
    N, M, P = out.shape
    _check(out, torch.float32, (N, M, P), "evolve_sample out")
    _check(mean, torch.float32, (N, P), "evolve_sample mean")
    _check(sigma, torch.float32, (N, P), "evolve_sample sigma")
    _check(free, torch.uint8, (P,), "evolve_sample free")
    st = _lib.load().ias_evolve_sample(_lib.ptr(mean), _lib.ptr(sigma), _lib.ptr(free), N, M, P, int(n_base), int(m_base),
                                       int(seed) & 0xFFFFFFFFFFFFFFFF, int(generation), _lib.ptr(out), _lib.stream())
    _lib.check(st, "ias_evolve_sample")
    return out


def evolve_update(pop, base, elite_dist, elite_idx, prev_idx, prev_params, elite_params, mean, sigma, free, alpha,
                  sigma_min, sigma_max):
    """One launch of ias_evolve_update (include/ias_hip.h) after ``topk_merge(dist, base, elite_dist, elite_idx)``: gathers
    the elites' parameters into ``elite_params`` (from ``pop`` or ``prev_params``) and refits ``mean`` / ``sigma`` in
    place."""
    if pop.dim() != 3 or elite_dist.dim() != 2:
        raise ValueError(f"evolve_update: pop [N, M, P] and elite_dist [N, k], got {tuple(pop.shape)} and "
                         f"{tuple(elite_dist.shape)}")
    N, M, P = pop.shape
    k = elite_dist.shape[1]
    _check(pop, torch.float32, (N, M, P), "evolve_update pop")
    _check(elite_dist, torch.float32, (N, k), "evolve_update elite_dist")
    _check(elite_idx, torch.int64, (N, k), "evolve_update elite_idx")
    _check(prev_idx, torch.int64, (N, k), "evolve_update prev_idx")
    _check(prev_params, torch.float32, (N, k, P), "evolve_update prev_params")
    _check(elite_params, torch.float32, (N, k, P), "evolve_update elite_params")
    _check(mean, torch.float32, (N, P), "evolve_update mean")
    _check(sigma, torch.float32, (N, P), "evolve_update sigma")
    _check(free, torch.uint8, (P,), "evolve_update free")
    st = _lib.load().ias_evolve_update(_lib.ptr(pop), int(base), M, _lib.ptr(elite_dist), _lib.ptr(elite_idx),
                                       _lib.ptr(prev_idx), _lib.ptr(prev_params), _lib.ptr(elite_params), _lib.ptr(mean),
                                       _lib.ptr(sigma), _lib.ptr(free), N, k, P, float(alpha), float(sigma_min),
                                       float(sigma_max), _lib.stream())
    _lib.check(st, "ias_evolve_update")


def free_columns(frozen, device):
    """(module, name) keys as ``SoundMatcher(frozen=...)`` -> [78] uint8, 0 at the frozen parameters."""
    frozen = [tuple(k) for k in frozen]
    for k in frozen:
        if k not in S.INDEX:
            raise KeyError(f"unknown Voice parameter {k}")
    return torch.tensor([(m, n) not in frozen for (m, n, *_r) in S.PARAMS], dtype=torch.uint8, device=device)


@torch.no_grad()
def evolve_search(voice, loss, target_audio=None, target_values=None, generations=20, population=None, elites=8,
                  init_params01=None, sigma0=0.2, alpha=0.7, sigma_min=0.005, sigma_max=0.5, seed=0, frozen=()):
    """Elitist cross-entropy search of the Voice parameters nearest to each target under ``loss`` -> ``EvolveResult``.

    ``loss``: a ``MelSpectrogramL1`` or an ``STFTL1`` (``SoundMatcher.loss``; the multi-resolution loss is refused as by
    ``SpectralBank``).  Give the targets as audio [N, T] or as their ``loss.target`` values.  Per sound the search keeps a
    Gaussian per parameter, ``mean`` (initially start 0) and ``sigma`` (initially ``sigma0``), and the ``elites`` best
    candidates seen so far.  Every generation draws ``population`` (M, a positive multiple of B = ``voice.batch_size``;
    default 4 B) candidates clamp(mean + sigma z, 0, 1), scores them, merges them into the elites and moves the Gaussian
    towards the elites' mean and standard deviation by ``alpha``, sigma kept within [sigma_min, sigma_max].  ``frozen``
    ((module, name) keys as ``SoundMatcher``): those parameters stay at start 0's value in every sampled candidate.

    ``init_params01``: None (0.5 everywhere), [N, 78] or [N, S, 78] with S <= M.  The starts are candidates m < S of
    generation 0, written over the sampled ones, so a start (a bank voice, say) competes as it is and can never be lost;
    the starts keep their own values in the frozen columns.

    Index convention: candidate m of generation g has the global index g M + m (``EvolveResult.idx``) and is rendered at
    row m % B of the Voice, as a bank item is.  The Voice keeps one noise row per batch row, so a parameter vector renders
    the same audio only at the same row (unless its noise mixer level is 0): ``dist`` is the loss of the elite rendered at
    row idx % M % B, which is not the row ``SoundMatcher.fit`` will give it (``SpectralBank`` has the same caveat).

    Per generation and sound: M / B renders and value passes into one reused buffer and one ias_l1_cdist; then, for all
    sounds at once, a copy of the elite indices, one ias_topk_merge, one ias_evolve_update, one copy into ``history`` and
    one ias_evolve_sample for the next generation.  The host reads nothing from the device inside the loop, every buffer
    is reused, no gradient is taken and ``voice.params01`` is left alone.  A run is a function of its arguments: the same
    seed gives the same bits."""
    sc = Scorer(voice, loss)
    B, T, K, P = sc.B, sc.T, sc.K, voice.params01.shape[1]
    dev = voice.params01.device
    G = int(generations)
    if G < 1:
        raise ValueError(f"evolve_search: generations must be >= 1, got {generations}")
    M = 4 * B if population is None else int(population)
    if M < 1 or M % B != 0:
        raise ValueError(f"evolve_search: population must be a positive multiple of the voice's batch size {B}, got {M}")
    if M > (1 << 31) // G:
        raise ValueError(f"evolve_search: population x generations must not exceed 2^31, got {M} x {G}")
    k = int(elites)
    if not 1 <= k <= 64 or k > M:
        raise ValueError(f"evolve_search: elites must be in 1..64 (ias_topk_merge) and at most the population {M}, got {k}")
    for name, v in (("sigma0", sigma0), ("sigma_min", sigma_min), ("sigma_max", sigma_max)):
        if not (0.0 <= float(v) < float("inf")):
            raise ValueError(f"evolve_search: {name} must be finite and >= 0, got {v}")
    if float(sigma_max) < float(sigma_min) or not 0.0 <= float(alpha) <= 1.0:
        raise ValueError("evolve_search: need sigma_min <= sigma_max and alpha in [0, 1]")
    if target_audio is not None:
        if target_audio.dim() != 2 or target_audio.shape[1] != T:
            raise ValueError(f"target_audio must be [N, {T}] (the voice's buffer), got {tuple(target_audio.shape)}")
        target_audio = target_audio.detach().to(device=dev, dtype=torch.float32)
    q = sc.targets(target_audio, target_values, "evolve_search")
    N = q.shape[0]
    if N > 65535:
        raise ValueError(f"evolve_search: at most 65535 sounds per call (ias_topk_merge), got {N}")
    if init_params01 is None:
        starts = torch.full((N, 1, P), 0.5, dtype=torch.float32, device=dev)
    else:
        starts = init_params01.detach().to(device=dev, dtype=torch.float32)
        starts = starts.unsqueeze(1) if starts.dim() == 2 else starts
        if starts.dim() != 3 or starts.shape[0] != N or starts.shape[2] != P or not 1 <= starts.shape[1] <= M:
            raise ValueError(f"init_params01 must be [{N}, {P}] or [{N}, starts <= {M}, {P}], got "
                             f"{tuple(init_params01.shape)}")
        starts = starts.clamp(0.0, 1.0)
    nS = starts.shape[1]
    free = free_columns(frozen, dev)

    ws = sc.workspace(1, M)
    values = torch.empty((M, sc.F, sc.n_out), dtype=torch.float32, device=dev)
    block = torch.empty((N, M), dtype=torch.float32, device=dev)
    pop = torch.empty((N, M, P), dtype=torch.float32, device=dev)
    mean = starts[:, 0].contiguous().clone()
    sigma = torch.full((N, P), float(sigma0), dtype=torch.float32, device=dev)
    elite_dist = torch.full((N, k), float("inf"), dtype=torch.float32, device=dev)
    elite_idx = torch.full((N, k), EMPTY_INDEX, dtype=torch.int64, device=dev)
    prev_idx = torch.empty_like(elite_idx)
    elite_params = torch.zeros((N, k, P), dtype=torch.float32, device=dev)
    prev_params = torch.zeros_like(elite_params)
    history = torch.empty((G, N), dtype=torch.float32, device=dev)

    evolve_sample(mean, sigma, free, seed, 0, pop)
    pop[:, :nS] = starts
    sounds = pop.unbind(0)                               # views, made once: pop is rewritten in place
    for g in range(G):
        for n in range(N):
            sc.fill(values, sounds[n])
            l1_cdist(q[n:n + 1], values.view(M, K), out=block[n:n + 1], workspace=ws)
        prev_idx.copy_(elite_idx)
        elite_params, prev_params = prev_params, elite_params
        topk_merge(block, g * M, elite_dist, elite_idx)
        evolve_update(pop, g * M, elite_dist, elite_idx, prev_idx, prev_params, elite_params, mean, sigma, free, alpha,
                      sigma_min, sigma_max)
        history[g].copy_(elite_dist[:, 0])
        if g + 1 < G:
            evolve_sample(mean, sigma, free, seed, g + 1, pop)
    return EvolveResult(params01=elite_params, dist=elite_dist, idx=elite_idx, mean=mean, sigma=sigma, history=history)

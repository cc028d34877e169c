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
from types import SimpleNamespace

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
    history: torch.Tensor           # [G, N] fp32: dist[:, 0] after each generation (None when not kept)


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


# The three primitives of ``cross_entropy_search`` on the device.  The tests pass the same three restated in numpy on CPU
# tensors (tests/evolve_model.py), so the loop below is one code path for both.
DEVICE_OPS = SimpleNamespace(sample=evolve_sample, merge=topk_merge, update=evolve_update)


@torch.no_grad()
def cross_entropy_search(starts, free, score, generations, population, elites, sigma0, alpha, sigma_min, sigma_max, seed,
                         keep_history=True, ops=DEVICE_OPS, what="cross_entropy_search"):
    """The elitist cross-entropy search itself, whatever is searched -> ``EvolveResult`` (P columns in place of 78).

    ``starts`` [N, S, P] fp32 in 0..1 and ``free`` [P] uint8 on the device of the search; ``score(g, pop, out)`` fills
    out [N, M] fp32 with the distances of generation g's candidates pop [N, M, P] (the same two buffers every generation).
    Per sound a Gaussian per column, ``mean`` (initially start 0) and ``sigma`` (initially ``sigma0``).  The first
    population is drawn and candidates m < S of it overwritten with the starts, so a start competes as it is and can never
    be lost.  Then per generation g: ``score``; a copy of the elite indices (``prev_idx``, taken BEFORE the merge) and a
    swap of ``elite_params`` and ``prev_params`` (two buffers: the update gathers from one into the other);
    ``ops.merge`` of the block at base g M into the ``elites`` best seen so far; ``ops.update``, which gathers their
    parameters and moves the Gaussian towards them by ``alpha``, sigma kept within [sigma_min, sigma_max]; with
    ``keep_history`` one copy of dist[:, 0] into ``history[g]``; and ``ops.sample`` for generation g + 1.  The host reads
    nothing back and every buffer is reused.  Limits: M G <= 2^31 (the index g M + m), 1 <= k <= 64 and k <= M and
    1 <= N <= 65535 (ias_topk_merge).  ``what`` begins every refusal."""
    G, M, k = int(generations), int(population), int(elites)
    if G < 1:
        raise ValueError(f"{what}: generations must be >= 1, got {generations}")
    if M < 1 or M > (1 << 31) // G:
        raise ValueError(f"{what}: population must be >= 1 and population x generations at most 2^31, got {M} x {G}")
    if not 1 <= k <= 64 or k > M:
        raise ValueError(f"{what}: elites must be in 1..64 (ias_topk_merge) and at most the population {M}, got {k}")
    for name, v in (("sigma0", sigma0), ("sigma_min", sigma_min), ("sigma_max", sigma_max)):
        if not (0.0 <= float(v) < float("inf")):
            raise ValueError(f"{what}: {name} must be finite and >= 0, got {v}")
    if float(sigma_max) < float(sigma_min) or not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"{what}: need sigma_min <= sigma_max and alpha in [0, 1]")
    if starts.dim() != 3 or starts.dtype != torch.float32 or not 1 <= starts.shape[1] <= M:
        raise ValueError(f"{what}: the starts must be float32 [N, 1..{M}, P], got {starts.dtype} {tuple(starts.shape)}")
    N, nS, P = starts.shape
    if not 1 <= N <= 65535:
        raise ValueError(f"{what}: 1..65535 sounds per call (ias_topk_merge), got {N}")
    dev = starts.device

    block = torch.empty((N, M), dtype=torch.float32, device=dev)
    pop = torch.empty((N, M, P), dtype=torch.float32, device=dev)
    mean = starts[:, 0].contiguous().clone()
    sigma = torch.full((N, P), float(sigma0), dtype=torch.float32, device=dev)
    elite_dist = torch.full((N, k), float("inf"), dtype=torch.float32, device=dev)
    elite_idx = torch.full((N, k), EMPTY_INDEX, dtype=torch.int64, device=dev)
    prev_idx = torch.empty_like(elite_idx)
    elite_params = torch.zeros((N, k, P), dtype=torch.float32, device=dev)
    prev_params = torch.zeros_like(elite_params)
    history = torch.empty((G, N), dtype=torch.float32, device=dev) if keep_history else None

    ops.sample(mean, sigma, free, seed, 0, pop)
    pop[:, :nS] = starts
    for g in range(G):
        score(g, pop, block)
        prev_idx.copy_(elite_idx)
        elite_params, prev_params = prev_params, elite_params
        ops.merge(block, g * M, elite_dist, elite_idx)
        ops.update(pop, g * M, elite_dist, elite_idx, prev_idx, prev_params, elite_params, mean, sigma, free, alpha,
                   sigma_min, sigma_max)
        if keep_history:
            history[g].copy_(elite_dist[:, 0])
        if g + 1 < G:
            ops.sample(mean, sigma, free, seed, g + 1, pop)
    return EvolveResult(params01=elite_params, dist=elite_dist, idx=elite_idx, mean=mean, sigma=sigma, history=history)


@torch.no_grad()
def evolve_search(voice, loss, target_audio=None, target_values=None, generations=20, population=None, elites=8,
                  init_params01=None, sigma0=0.2, alpha=0.7, sigma_min=0.005, sigma_max=0.5, seed=0, frozen=()):
    """Elitist cross-entropy search of the Voice parameters nearest to each target under ``loss`` -> ``EvolveResult``.

    ``loss``: a ``MelSpectrogramL1`` or an ``STFTL1`` (``SoundMatcher.loss``; the multi-resolution loss is refused as by
    ``SpectralBank``).  Give the targets as audio [N, T] or as their ``loss.target`` values.  The search and the meaning
    of its settings are ``cross_entropy_search``'s, over the 78 parameters with ``population`` (M, a positive multiple of
    B = ``voice.batch_size``; default 4 B) candidates per generation.  ``frozen`` ((module, name) keys as
    ``SoundMatcher``): those parameters stay at start 0's value in every sampled candidate.

    ``init_params01``: None (0.5 everywhere), [N, 78] or [N, S, 78] with S <= M.  The starts are candidates m < S of
    generation 0, written over the sampled ones, so a start (a bank voice, say) competes as it is and can never be lost;
    the starts keep their own values in the frozen columns.

    Index convention: candidate m of generation g has the global index g M + m (``EvolveResult.idx``) and is rendered at
    row m % B of the Voice, as a bank item is.  The Voice keeps one noise row per batch row, so a parameter vector renders
    the same audio only at the same row (unless its noise mixer level is 0): ``dist`` is the loss of the elite rendered at
    row idx % M % B, which is not the row ``SoundMatcher.fit`` will give it (``SpectralBank`` has the same caveat).

    This function is the loop's scorer: per generation and sound, M / B renders and value passes into one reused buffer
    and one ias_l1_cdist; the loop adds, for all sounds at once, a copy of the elite indices, one ias_topk_merge, one
    ias_evolve_update, one copy into ``history`` and one ias_evolve_sample.  No gradient is taken and ``voice.params01`` is
    left alone.  A run is a function of its arguments: the same seed gives the same bits."""
    sc = Scorer(voice, loss)
    B, T, K, P = sc.B, sc.T, sc.K, voice.params01.shape[1]
    dev = voice.params01.device
    M = 4 * B if population is None else int(population)
    if M < 1 or M % B != 0:
        raise ValueError(f"evolve_search: population must be a positive multiple of the voice's batch size {B}, got {M}")
    if target_audio is not None:
        if target_audio.dim() != 2 or target_audio.shape[1] != T:
            raise ValueError(f"target_audio must be [N, {T}] (the voice's buffer), got {tuple(target_audio.shape)}")
        target_audio = target_audio.detach().to(device=dev, dtype=torch.float32)
    q = sc.targets(target_audio, target_values, "evolve_search")
    N = q.shape[0]
    if init_params01 is None:
        starts = torch.full((N, 1, P), 0.5, dtype=torch.float32, device=dev)
    else:
        starts = init_params01.detach().to(device=dev, dtype=torch.float32)
        starts = starts.unsqueeze(1) if starts.dim() == 2 else starts
        if starts.dim() != 3 or starts.shape[0] != N or starts.shape[2] != P or not 1 <= starts.shape[1] <= M:
            raise ValueError(f"init_params01 must be [{N}, {P}] or [{N}, starts <= {M}, {P}], got "
                             f"{tuple(init_params01.shape)}")
        starts = starts.clamp(0.0, 1.0)
    free = free_columns(frozen, dev)

    own = SimpleNamespace()                              # the scorer's buffers, made once the loop has accepted the sizes

    def score(g, pop, out):
        if g == 0:
            own.ws = sc.workspace(1, M)
            own.values = torch.empty((M, sc.F, sc.n_out), dtype=torch.float32, device=dev)
            own.sounds = pop.unbind(0)                   # views, made once: pop is rewritten in place
        ws, values, sounds = own.ws, own.values, own.sounds
        for n in range(N):
            sc.fill(values, sounds[n])
            l1_cdist(q[n:n + 1], values.view(M, K), out=out[n:n + 1], workspace=ws)
    return cross_entropy_search(starts, free, score, generations, M, elites, sigma0, alpha, sigma_min, sigma_max, seed,
                                what="evolve_search")

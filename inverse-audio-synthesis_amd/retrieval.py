"""Nearest-neighbour retrieval in embedding space.

The reference's notebook export searches the closest audio representations with ``torch.cdist``
(/root/reference/evaluate_audio_representations.py:202-231; the file itself is stale and does not import).
Here: embed a bank of rendered voices with a (frozen) ``VicregAudioParams``, then for query audio return the
indices / distances of the k closest bank items.  ``torch.cdist`` is a plain library GEMM on ROCm.

``SpectralBank`` needs no trained model: it ranks the bank voices by the sound matcher's own spectral L1 (all pairs in
one ias_l1_cdist launch, csrc/bank_kernels.hip), the start ``match_audio.py --init bank`` uses.
"""
import ctypes

import torch

from . import _lib


@torch.no_grad()
def embed_audio(model, audio):
    """audio [B, T] -> representation [B, dim] with the audio backbone (no projector), eval mode."""
    was_training = model.training
    model.eval()
    try:
        return model.vicreg.backbone_audio(audio.unsqueeze(1))
    finally:
        model.train(was_training)


@torch.no_grad()
def build_bank(model, batch_indices):
    """Render the given voice batches and embed them -> (embeddings [N, dim], params [N, 78])."""
    embs, params = [], []
    for idx in batch_indices:
        audio, p, _ = model.voice(int(idx))
        embs.append(embed_audio(model, audio))
        params.append(p)
    return torch.cat(embs), torch.cat(params)


@torch.no_grad()
def nearest(queries, bank, k=1):
    """-> (distances [Q, k], indices [Q, k]) of the k nearest bank rows (Euclidean, as torch.cdist)."""
    d = torch.cdist(queries, bank)
    dist, idx = torch.topk(d, k, dim=1, largest=False)
    return dist, idx


@torch.no_grad()
def init_from_bank(model, audio, bank_embs, bank_params):
    """Starting point for sound matching (match.SoundMatcher.fit's ``init_params01``): the parameters [N, 78] of the
    bank item nearest to each query sound audio [N, T] in embedding space."""
    _dist, idx = nearest(embed_audio(model, audio), bank_embs, k=1)
    return bank_params[idx[:, 0]].clone()


# ------------------------------------------------------------------------------------------------ spectral bank
def rank_distances(dist):
    """[N, M] distances -> [N, M] int64 bank indices per row in ascending order: a stable sort, so equal distances keep
    the lowest index first; NaN and +-Inf rank after every finite distance (among themselves by index)."""
    key = torch.where(torch.isfinite(dist), dist, torch.full_like(dist, float("inf")))
    return torch.sort(key, dim=1, stable=True).indices


def l1_cdist(queries, bank, out=None, workspace=None):
    """queries [N, K], bank [M, K] fp32 on the device (any row-major views with row stride K) -> [N, M] fp32
    sum_k |queries[n, k] - bank[m, k]| / K (ias_l1_cdist: a pair's value is the same bits whatever N, M, n, m or where the
    rows sit in memory).  ``out`` ([N, M] fp32, contiguous) and ``workspace`` (uint8, at least
    ias_l1_cdist_workspace_bytes(N, M, K)) are allocated unless given (a caller in a loop reuses its own)."""
    lib = _lib.load()
    _lib.require_f32(queries, bank)
    if queries.dim() != 2 or bank.dim() != 2 or queries.shape[1] != bank.shape[1]:
        raise ValueError(f"l1_cdist: queries [N, K] and bank [M, K], got {tuple(queries.shape)} and {tuple(bank.shape)}")
    N, K = queries.shape
    M = bank.shape[0]
    nbytes = lib.ias_l1_cdist_workspace_bytes(N, M, K)
    _lib.check(min(nbytes, 0), "ias_l1_cdist_workspace_bytes")
    if workspace is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=queries.device)
    else:
        ws = workspace
        if ws.dtype != torch.uint8 or ws.numel() < nbytes:
            raise ValueError(f"l1_cdist: workspace must be uint8 with at least {nbytes} bytes")
    if out is None:
        dist = torch.empty((N, M), dtype=torch.float32, device=queries.device)
    else:
        dist = out
        _lib.require_f32(dist)
        if tuple(dist.shape) != (N, M):
            raise ValueError(f"l1_cdist: out must be [{N}, {M}], got {tuple(dist.shape)}")
    _lib.check(lib.ias_l1_cdist(_lib.ptr(queries), _lib.ptr(bank), N, M, K, _lib.ptr(ws), _lib.ptr(dist), _lib.stream()),
               "ias_l1_cdist")
    return dist


EMPTY_INDEX = torch.iinfo(torch.int64).max              # an empty slot of a running top-k is (+inf, EMPTY_INDEX)


def topk_merge(dist, base, best_dist, best_idx):
    """Merge a block of candidate distances into the running k nearest per row, in place (ias_topk_merge).

    dist [N, M] fp32 on the device (unit column stride, any row stride >= M): the candidates of global bank indices
    ``base + m``, disjoint from the indices already in ``best_idx``.  best_dist [N, k] fp32, best_idx [N, k] int64
    (contiguous, k <= 64): the running result in ``rank_distances`` order (finite distances ascending, equal ones by
    ascending index, non-finite ones last by index), each entry with its original distance.  A fresh state is
    ``best_dist`` filled with +inf and ``best_idx`` with ``EMPTY_INDEX``.  The result depends only on the set of
    candidates merged so far, not on how they were cut into blocks or in which order the blocks came."""
    lib = _lib.load()
    _lib.require_f32(dist, best_dist)
    if dist.dim() != 2 or best_dist.dim() != 2 or best_idx.dtype != torch.int64 or best_idx.shape != best_dist.shape \
            or best_dist.shape[0] != dist.shape[0]:
        raise ValueError(f"topk_merge: dist [N, M] fp32, best_dist [N, k] fp32 and best_idx [N, k] int64, got "
                         f"{tuple(dist.shape)}, {tuple(best_dist.shape)} and {tuple(best_idx.shape)} {best_idx.dtype}")
    N, M = dist.shape
    if not dist.is_cuda or N < 1 or M < 1 or (M > 1 and dist.stride(1) != 1):
        raise ValueError("topk_merge: dist must be a non-empty device tensor with unit column stride")
    ld = dist.stride(0) if N > 1 else M
    _lib.check(lib.ias_topk_merge(ctypes.c_void_p(dist.data_ptr()), N, M, ld, int(base), best_dist.shape[1],
                                  _lib.ptr(best_dist), _lib.ptr(best_idx), _lib.stream()), "ias_topk_merge")


def _bank_plan(loss):
    from .spectral import MelSpectrogramL1, MultiResolutionSTFTLoss, STFTL1
    if isinstance(loss, MelSpectrogramL1):
        return loss.mel.plan
    if isinstance(loss, STFTL1):
        return loss.plan
    if isinstance(loss, MultiResolutionSTFTLoss):
        raise ValueError("SpectralBank: the multi-resolution STFT loss is not the L1 of one array; build the bank with a "
                         "MelSpectrogramL1 (a mel bank) and fit with any loss")
    raise ValueError(f"SpectralBank: the loss must be a MelSpectrogramL1 or an STFTL1, got {type(loss).__name__}")


class Scorer:
    """Render candidates and score them against targets under a per-sound L1 loss, for the resident bank, the streamed
    search and ``evolve_search``: B rows of T samples per render, ``loss.target`` values [F, n_out] per row, K = F n_out."""

    def __init__(self, voice, loss):
        self.voice, self.loss, self.plan = voice, loss, _bank_plan(loss)
        self.B, self.T = voice.batch_size, voice.synthconfig.buffer_size
        self.F, self.n_out = self.plan.num_frames(self.T), self.plan.n_out
        self.K = self.F * self.n_out

    def targets(self, target_audio, target_values, what):
        """The targets as audio [N, T] or as their ``loss.target`` values [N, F, n_out] -> q [N, K] fp32 contiguous."""
        if (target_audio is None) == (target_values is None):
            raise ValueError(f"{what}: give the target audio or its values")
        if target_values is None:
            target_values = self.loss.target(target_audio)
        if tuple(target_values.shape[1:]) != (self.F, self.n_out):
            raise ValueError(f"{what}: target values must be [N, {self.F}, {self.n_out}], got {tuple(target_values.shape)}")
        return target_values.detach().to(torch.float32).contiguous().reshape(-1, self.K)

    def workspace(self, N, M):
        """The uint8 workspace of ``l1_cdist`` on [N, K] queries and [M, K] candidates."""
        nbytes = _lib.load().ias_l1_cdist_workspace_bytes(N, M, self.K)
        _lib.check(min(nbytes, 0), "ias_l1_cdist_workspace_bytes")
        return torch.empty(nbytes, dtype=torch.uint8, device=self.voice.params01.device)

    def fill(self, values, params, row=0):
        """values[row:row + len(params)] = ``loss.target`` of the renders of params [j B, 78], row m at Voice row m % B."""
        B = self.B
        for j in range(params.shape[0] // B):
            values[row + j * B:row + (j + 1) * B] = self.loss.target(      # (unnamed: the next render reuses its buffer)
                self.voice.render(params[j * B:(j + 1) * B], normalize=True))


class SpectralBank:
    """A bank of rendered voices and their spectral values under a per-sound L1 loss (``MelSpectrogramL1`` or ``STFTL1``,
    e.g. ``SoundMatcher.loss``), searched with the loss itself: ``distances(target_values)[n, m]`` is the quantity
    ``loss.per_item`` measures between target n and the render of ``params01[m]``, summed in another fixed order.

    Batch index i is rendered as ``voice.render(sample_params01(B, i), normalize=True)``, the parameters ``voice(i)``
    would draw; ``voice.params01`` is left alone.  The Voice keeps one noise row per batch row, so a parameter vector
    renders the same audio only at the same row (unless its noise mixer level is 0): a bank distance is the loss of bank
    item m = i B + r rendered at row r.  The bank holds M = len(batch_indices) B voices: ``params01`` [M, 78] and
    ``values`` [M, F, n_out] fp32 (``loss.target`` of each render)."""

    def __init__(self, voice, loss, batch_indices):
        from .voice import sample_params01
        sc = self._scorer = Scorer(voice, loss)
        self.plan, self.loss = sc.plan, loss
        B, dev = sc.B, voice.params01.device
        idx = [int(i) for i in batch_indices]
        if not idx:
            raise ValueError("SpectralBank: no batch indices")
        self.params01 = torch.empty((len(idx) * B, voice.params01.shape[1]), dtype=torch.float32, device=dev)
        self.values = torch.empty((len(idx) * B, sc.F, sc.n_out), dtype=torch.float32, device=dev)
        with torch.no_grad():
            for j, i in enumerate(idx):
                p = sample_params01(B, i).to(dev)
                self.params01[j * B:(j + 1) * B] = p
                sc.fill(self.values, p, j * B)

    @staticmethod
    def nbytes(voice, loss, n_batches):
        """Bytes of the values of a bank of ``n_batches`` voice batches (before building it)."""
        sc = Scorer(voice, loss)
        return 4 * int(n_batches) * sc.B * sc.K

    @torch.no_grad()
    def distances(self, target_values):
        """target_values [N, F, n_out] (``loss.target`` of the targets) -> [N, M] fp32 mean |target - bank| per pair."""
        return l1_cdist(self._scorer.targets(None, target_values, "SpectralBank"), self.values.flatten(1))

    @torch.no_grad()
    def nearest(self, target_audio=None, target_values=None, k=1):
        """The k nearest bank voices of each target (give the audio [N, T] or its ``loss.target`` values) -> (dist [N, k]
        fp32, idx [N, k] int64) in ``rank_distances`` order; ``params01[idx]`` are the starts for ``SoundMatcher.fit``."""
        d = l1_cdist(self._scorer.targets(target_audio, target_values, "SpectralBank"), self.values.flatten(1))
        k = min(int(k), d.shape[1])
        idx = rank_distances(d)[:, :k]
        return torch.gather(d, 1, idx), idx

    @staticmethod
    @torch.no_grad()
    def search(voice, loss, batch_indices, target_audio=None, target_values=None, k=1, chunk_batches=8):
        """``SpectralBank(voice, loss, batch_indices).nearest(...)`` without the bank in memory: the same indices and the
        same distance bits (a pair's ias_l1_cdist value does not depend on the launch; the merge does not depend on the
        cut), for a bank of any size -> (dist [N, k] fp32, idx [N, k] int64, params01 [N, k, 78] fp32).

        The bank is rendered ``chunk_batches`` voice batches at a time into one reused [chunk_batches B, F, n_out]
        buffer; each chunk costs one upload of its parameters from pinned memory, its renders and value passes, one
        ias_l1_cdist and one ias_topk_merge, and the host reads nothing from the device until the loop is over.  Index
        convention as for the resident bank: item m = j B + r is row r of ``batch_indices[j]``, rendered at row r.
        ``params01`` is drawn again on the host for the winning batches only; ``voice.params01`` is left alone."""
        from .voice import sample_params01
        sc = Scorer(voice, loss)
        idx = [int(i) for i in batch_indices]
        if not idx:
            raise ValueError("SpectralBank: no batch indices")
        C = int(chunk_batches)
        if C < 1:
            raise ValueError("SpectralBank.search: chunk_batches must be >= 1")
        C = min(C, len(idx))
        B, K, P = sc.B, sc.K, voice.params01.shape[1]
        dev = voice.params01.device
        q = sc.targets(target_audio, target_values, "SpectralBank.search")
        N = q.shape[0]
        k = min(int(k), len(idx) * B)
        if not 1 <= k <= 64:
            raise ValueError(f"SpectralBank.search: k must be in 1..64 (ias_topk_merge), got {k}")

        ws = sc.workspace(N, C * B)
        block = torch.empty(N * C * B, dtype=torch.float32, device=dev)
        values = torch.empty((C * B, sc.F, sc.n_out), dtype=torch.float32, device=dev)
        params = torch.empty((C * B, P), dtype=torch.float32, device=dev)
        # two pinned staging buffers: the host fills one while the other's upload may still be queued behind the
        # previous chunk's kernels; an event per buffer says when its upload has been consumed
        staging = [torch.empty((C * B, P), dtype=torch.float32, pin_memory=True) for _ in range(2)]
        uploaded = [torch.cuda.Event(), torch.cuda.Event()]
        best_dist = torch.full((N, k), float("inf"), dtype=torch.float32, device=dev)
        best_idx = torch.full((N, k), EMPTY_INDEX, dtype=torch.int64, device=dev)
        for c, j0 in enumerate(range(0, len(idx), C)):
            chunk = idx[j0:j0 + C]
            n = len(chunk)
            host = staging[c & 1]
            if c >= 2:
                uploaded[c & 1].synchronize()
            for j, i in enumerate(chunk):
                host[j * B:(j + 1) * B] = sample_params01(B, i)
            params[:n * B].copy_(host[:n * B], non_blocking=True)
            uploaded[c & 1].record()
            sc.fill(values, params[:n * B])
            d = l1_cdist(q, values[:n * B].reshape(n * B, K), out=block[:N * n * B].view(N, n * B), workspace=ws)
            topk_merge(d, j0 * B, best_dist, best_idx)

        win = best_idx.cpu()
        batches, which = torch.unique(win // B, return_inverse=True)
        draws = torch.stack([sample_params01(B, idx[j]) for j in batches.tolist()])
        return best_dist, best_idx, draws[which, win % B].to(dev)

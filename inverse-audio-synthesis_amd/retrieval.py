"""Nearest-neighbour retrieval in embedding space.

The reference's notebook export searches the closest audio representations with ``torch.cdist``
(/root/reference/evaluate_audio_representations.py:202-231; the file itself is stale and does not import).
Here: embed a bank of rendered voices with a (frozen) ``VicregAudioParams``, then for query audio return the
indices / distances of the k closest bank items.  ``torch.cdist`` is a plain library GEMM on ROCm.

``SpectralBank`` needs no trained model: it ranks the bank voices by the sound matcher's own spectral L1 (all pairs in
one ias_l1_cdist launch, csrc/bank_kernels.hip), the start ``match_audio.py --init bank`` uses.
"""
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


def l1_cdist(queries, bank):
    """queries [N, K], bank [M, K] fp32 on the device (any row-major views with row stride K) -> [N, M] fp32
    sum_k |queries[n, k] - bank[m, k]| / K (ias_l1_cdist: a pair's value is the same bits whatever N, M, n, m or where the
    rows sit in memory)."""
    lib = _lib.load()
    _lib.require_f32(queries, bank)
    if queries.dim() != 2 or bank.dim() != 2 or queries.shape[1] != bank.shape[1]:
        raise ValueError(f"l1_cdist: queries [N, K] and bank [M, K], got {tuple(queries.shape)} and {tuple(bank.shape)}")
    N, K = queries.shape
    M = bank.shape[0]
    nbytes = lib.ias_l1_cdist_workspace_bytes(N, M, K)
    _lib.check(min(nbytes, 0), "ias_l1_cdist_workspace_bytes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=queries.device)
    dist = torch.empty((N, M), dtype=torch.float32, device=queries.device)
    _lib.check(lib.ias_l1_cdist(_lib.ptr(queries), _lib.ptr(bank), N, M, K, _lib.ptr(ws), _lib.ptr(dist), _lib.stream()),
               "ias_l1_cdist")
    return dist


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
        self.plan = _bank_plan(loss)
        self.loss = loss
        B, T = voice.batch_size, voice.synthconfig.buffer_size
        dev = voice.params01.device
        idx = [int(i) for i in batch_indices]
        if not idx:
            raise ValueError("SpectralBank: no batch indices")
        F, n_out = self.plan.num_frames(T), self.plan.n_out
        self.params01 = torch.empty((len(idx) * B, voice.params01.shape[1]), dtype=torch.float32, device=dev)
        self.values = torch.empty((len(idx) * B, F, n_out), dtype=torch.float32, device=dev)
        with torch.no_grad():
            for j, i in enumerate(idx):
                p = sample_params01(B, i).to(dev)
                self.params01[j * B:(j + 1) * B] = p
                self.values[j * B:(j + 1) * B] = loss.target(voice.render(p, normalize=True))

    @staticmethod
    def nbytes(voice, loss, n_batches):
        """Bytes of the values of a bank of ``n_batches`` voice batches (before building it)."""
        plan = _bank_plan(loss)
        return 4 * int(n_batches) * voice.batch_size * plan.num_frames(voice.synthconfig.buffer_size) * plan.n_out

    @torch.no_grad()
    def distances(self, target_values):
        """target_values [N, F, n_out] (``loss.target`` of the targets) -> [N, M] fp32 mean |target - bank| per pair."""
        if tuple(target_values.shape[1:]) != tuple(self.values.shape[1:]):
            raise ValueError(f"target values must be [N, {self.values.shape[1]}, {self.values.shape[2]}], got "
                             f"{tuple(target_values.shape)}")
        K = self.values[0].numel()
        q = target_values.detach().to(torch.float32).contiguous().reshape(-1, K)
        return l1_cdist(q, self.values.reshape(-1, K))

    @torch.no_grad()
    def nearest(self, target_audio=None, target_values=None, k=1):
        """The k nearest bank voices of each target (give the audio [N, T] or its ``loss.target`` values) -> (dist [N, k]
        fp32, idx [N, k] int64) in ``rank_distances`` order; ``params01[idx]`` are the starts for ``SoundMatcher.fit``."""
        if (target_audio is None) == (target_values is None):
            raise ValueError("give the target audio or its values")
        if target_values is None:
            target_values = self.loss.target(target_audio)
        d = self.distances(target_values)
        k = min(int(k), d.shape[1])
        idx = rank_distances(d)[:, :k]
        return torch.gather(d, 1, idx), idx

"""Sound matching: fit the 78 Voice parameters to given audio, each sound on its own.

This closes the loop the reference left commented out (/root/reference/audio_to_params.py:56-172: params -> synth ->
mel-L1 against the true audio) as a product feature, and returns what its notebook wanted in the end
(/root/reference/evaluate_audio_representations.py:202-231): a candidate and a distance per target sound.

Per chunk of ``voice.batch_size`` targets, every iteration is

    audio = voice.render(p)                      HIP render with its adjoint (voice_grad.py), normalize=True
    L     = loss.per_item(audio, target)         [B] per-sound spectral L1 or MR-STFT (spectral.py, csrc/match_kernels.hip)
    L.backward(active)                           per-row cotangent (the ``rows`` form of spectral._L1Fn / _MRSTFTFn:
                                                 ias_stft_loss_backward_rows, ias_mrstft_coef_rows + the *_mrstft_rows
                                                 span / frame kernels): a sound's gradient does not depend on the
                                                 batch, padded rows get exactly 0
    ias_match_adam_step                          best-so-far, non-finite skip, Adam per row, clamp to [0, 1]

with all state on the device and no host read inside the loop.

``fit_tied`` fits the notes of a phrase to ONE instrument: the rows of a group share every free column that is not one of
the group's ``own`` columns (by default the note and its length).  Render, loss and backward are the per-row ones above;
each iteration walks all chunks, collects the rows' gradients and losses in [N, 78] and [N] buffers and ends in one
``ias_match_tied_step`` (include/ias_hip_tied.h) over all N rows: the mean gradient of a tied column over the group, one
Adam update, the result written to every row.
"""
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from . import voice_spec as S
from .evolve import EvolveResult, evolve_search  # noqa: F401  (the search stage, exported beside the fit)
from .spectral import MelSpectrogramL1, MultiResolutionSTFTLoss, STFTL1

LOSSES = ("mel_l1", "stft_l1", "multi_resolution_stft")
DEFAULT_OWN = (("keyboard", "midi_f0"), ("keyboard", "duration"))   # fit_tied: what differs from note to note


@dataclass
class MatchResult:
    params01: torch.Tensor          # [N, 78] best parameters per sound
    loss: torch.Tensor              # [N] fp32: the loss of params01, exactly
    initial_loss: torch.Tensor      # [N] fp32: the loss of the initial parameters
    skipped: torch.Tensor           # [N] int32: iterations skipped for a non-finite loss or gradient
    audio: Optional[torch.Tensor] = None   # [N, T] render of params01 (fit(return_audio=True))
    start: Optional[torch.Tensor] = None   # [N] int64: the chosen start (init_params01 [N, S, 78] only)
    start_loss: Optional[torch.Tensor] = None            # [N, S] fp32: each start's final loss
    start_initial_loss: Optional[torch.Tensor] = None    # [N, S] fp32: each start's initial loss


@dataclass
class TiedMatchResult:
    params01: torch.Tensor          # [N, 78] best parameters: the rows of a group agree in every tied column
    loss: torch.Tensor              # [N] fp32: the per-note loss of params01, from a fresh forward
    group_loss: torch.Tensor        # [G] fp64: the best mean loss of every group (the mean of ``loss`` over its rows)
    initial_loss: torch.Tensor      # [N] fp32: the per-note loss of the (tied) start
    initial_group_loss: torch.Tensor    # [G] fp64
    skipped: torch.Tensor           # [G] int32: iterations a group skipped for a non-finite loss or gradient
    audio: Optional[torch.Tensor] = None   # [N, T] render of params01 (fit_tied(return_audio=True))


def match_adam_step(params01, grad, m, v, step, loss, best_loss, best_params, free, active, skipped, lr, betas, eps):
    """One launch of ias_match_adam_step over [B, P] (see include/ias_hip.h).  Updates params01, m, v, step, best_loss,
    best_params and skipped in place."""
    B, P = params01.shape
    for t, dt, shape in ((params01, torch.float32, (B, P)), (grad, torch.float32, (B, P)), (m, torch.float32, (B, P)),
                         (v, torch.float32, (B, P)), (best_params, torch.float32, (B, P)), (step, torch.int32, (B,)),
                         (loss, torch.float32, (B,)), (best_loss, torch.float64, (B,)), (free, torch.uint8, (P,)),
                         (active, torch.uint8, (B,)), (skipped, torch.int32, (B,))):
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"match_adam_step: expected a contiguous {dt} tensor of shape {shape}, got {t.dtype} "
                             f"{tuple(t.shape)}")
    st = _lib.load().ias_match_adam_step(
        _lib.ptr(params01), _lib.ptr(grad), _lib.ptr(m), _lib.ptr(v), _lib.ptr(step), _lib.ptr(loss), _lib.ptr(best_loss),
        _lib.ptr(best_params), _lib.ptr(free), _lib.ptr(active), _lib.ptr(skipped), B, P, float(lr), float(betas[0]),
        float(betas[1]), float(eps), _lib.stream())
    _lib.check(st, "ias_match_adam_step")


def tied_adam_step(params01, grad, m, v, best_params, loss, group_start, step, skipped, best_loss, group_loss, free, tied,
                   active, update, lr, betas, eps):
    """One launch of ias_match_tied_step over [N, P] rows in G groups (see include/ias_hip_tied.h).  Updates params01, m,
    v, step, best_loss, best_params, group_loss and skipped in place; ``update`` False: the best-so-far pass alone."""
    N, P = params01.shape
    G = step.shape[0]
    for t, dt, shape in ((params01, torch.float32, (N, P)), (grad, torch.float32, (N, P)), (m, torch.float32, (N, P)),
                         (v, torch.float32, (N, P)), (best_params, torch.float32, (N, P)), (loss, torch.float32, (N,)),
                         (group_start, torch.int32, (G + 1,)), (step, torch.int32, (G,)), (skipped, torch.int32, (G,)),
                         (best_loss, torch.float64, (G,)), (group_loss, torch.float64, (G,)), (free, torch.uint8, (P,)),
                         (tied, torch.uint8, (P,)), (active, torch.uint8, (G,))):
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"tied_adam_step: expected a contiguous {dt} tensor of shape {shape}, got {t.dtype} "
                             f"{tuple(t.shape)}")
    if update not in (0, 1, False, True):
        raise ValueError(f"tied_adam_step: update must be 0 or 1, got {update!r}")
    st = _lib.load().ias_match_tied_step(
        _lib.ptr(params01), _lib.ptr(grad), _lib.ptr(m), _lib.ptr(v), _lib.ptr(best_params), _lib.ptr(loss),
        _lib.ptr(group_start), _lib.ptr(step), _lib.ptr(skipped), _lib.ptr(best_loss), _lib.ptr(group_loss), _lib.ptr(free),
        _lib.ptr(tied), _lib.ptr(active), N, G, P, int(update), float(lr), float(betas[0]), float(betas[1]), float(eps),
        _lib.stream())
    _lib.check(st, "ias_match_tied_step")


def group_starts(groups, N):
    """groups [N]: non-decreasing integer group ids that start at 0 and leave none out -> group_start [G + 1] int32 on
    ``groups``' device (rows group_start[g] .. group_start[g + 1] - 1 are group g).  The one host read of ``fit_tied``:
    anything else raises ValueError."""
    if not isinstance(groups, torch.Tensor):
        groups = torch.as_tensor(groups)
    if groups.dim() != 1 or groups.shape[0] != N or N < 1:
        raise ValueError(f"groups must be [{N}] group ids, one per target, got {tuple(groups.shape)}")
    if groups.is_floating_point() or groups.is_complex() or groups.dtype == torch.bool:
        raise ValueError(f"groups must be integers, got {groups.dtype}")
    ids = groups.to(torch.int64)
    steps = ids[1:] - ids[:-1]
    ok = (ids[0] == 0) & (steps >= 0).all() & (steps <= 1).all()
    if not bool(ok):                                 # the host read
        raise ValueError("groups must be non-decreasing group ids that start at 0 and leave none out (0, 0, 1, 2, 2, ...)")
    first = torch.cat([torch.ones(1, dtype=torch.bool, device=ids.device), steps > 0])
    start = torch.nonzero(first).reshape(-1)
    return torch.cat([start, torch.full((1,), N, dtype=torch.int64, device=ids.device)]).to(torch.int32)


def tie_starts(params01, groups, tied, score=None):
    """params01 [N, P], groups [N] integer group ids (in any order), tied [P] (bool or uint8 mask), score [N] or None
    -> [N, P]: per group, the tied columns of every row take the values of the group's reference row; the other columns
    are left alone.  The reference row is the row with the lowest ``score``: ties go to the lowest row, NaN ranks last,
    ``score=None`` means the group's first row.  Plain torch without a host read, on the tensors' device (CPU too)."""
    N = params01.shape[0]
    dev = params01.device
    groups = torch.as_tensor(groups).to(device=dev, dtype=torch.int64)
    tied = torch.as_tensor(tied).to(device=dev) != 0
    if params01.dim() != 2 or tuple(groups.shape) != (N,) or tuple(tied.shape) != (params01.shape[1],):
        raise ValueError(f"tie_starts: params01 [N, P], groups [N] and tied [P] expected, got {tuple(params01.shape)}, "
                         f"{tuple(groups.shape)}, {tuple(tied.shape)}")
    order = torch.arange(N, device=dev)
    if score is not None:
        score = torch.as_tensor(score).to(device=dev, dtype=torch.float64)
        if tuple(score.shape) != (N,):
            raise ValueError(f"tie_starts: score must be [{N}], got {tuple(score.shape)}")
        nan = torch.isnan(score)
        # stable sorts from the least significant key up: row (as given), score, NaN last
        order = order[torch.sort(torch.where(nan, torch.zeros_like(score), score)[order], stable=True)[1]]
        order = order[torch.sort(nan[order].to(torch.int8), stable=True)[1]]
    order = order[torch.sort(groups[order], stable=True)[1]]          # ... and the group: its first row is its reference
    g = groups[order]
    first = torch.cat([torch.ones(1, dtype=torch.bool, device=dev), g[1:] != g[:-1]])
    at = torch.cummax(torch.where(first, torch.arange(N, device=dev), torch.zeros(N, dtype=torch.int64, device=dev)), 0)[0]
    ref = torch.empty(N, dtype=torch.int64, device=dev)
    ref[order] = order[at]
    return torch.where(tied.unsqueeze(0), params01[ref], params01)


class SoundMatcher:
    """Fit Voice parameters to target sounds by descent through the HIP render and a per-sound spectral loss.

    ``loss``: "mel_l1" (``MelSpectrogramL1(sample_rate=voice rate, **mel_kwargs)``), "stft_l1" (``STFTL1(**stft_kwargs)``)
    or "multi_resolution_stft" (``MultiResolutionSTFTLoss(**mrstft_kwargs)``: auraloss' defaults, FFT sizes 1024 / 2048 /
    512, hops 120 / 240 / 50, windows 600 / 1200 / 240, when none are given).
    ``frozen``: keys as ``Voice.get_parameters()`` ((module, name) pairs) that keep their initial value.  The matcher
    renders with explicit parameters: it leaves ``voice.params01`` and the voice's own frozen set alone."""

    def __init__(self, voice, loss="mel_l1", mel_kwargs=None, stft_kwargs=None, lr=0.01, betas=(0.9, 0.999), eps=1e-8,
                 frozen=(), mrstft_kwargs=None):
        self.voice = voice
        if loss == "mel_l1":
            kw = dict(mel_kwargs or {})
            kw.setdefault("sample_rate", voice.synthconfig.sample_rate)
            self.loss = MelSpectrogramL1(**kw)
        elif loss == "stft_l1":
            self.loss = STFTL1(**dict(stft_kwargs or {}))
        elif loss == "multi_resolution_stft":
            self.loss = MultiResolutionSTFTLoss(**dict(mrstft_kwargs or {}))
        else:
            raise ValueError(f"unknown matching loss {loss!r}: " + ", ".join(repr(n) for n in LOSSES))
        self.loss_kind = loss
        self.loss.to(voice.params01.device)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        keys = [(m, n) for (m, n, *_r) in S.PARAMS]
        frozen = [tuple(k) for k in frozen]
        for k in frozen:
            if k not in S.INDEX:
                raise KeyError(f"unknown Voice parameter {k}")
        self.frozen = tuple(frozen)
        self.free = torch.tensor([k not in frozen for k in keys], dtype=torch.uint8, device=voice.params01.device)

    def _per_item(self, audio, target):
        if self.loss_kind == "mel_l1":
            return self.loss.per_item(audio, target_mel=target)
        if self.loss_kind == "multi_resolution_stft":
            return self.loss.per_item(audio, targets=target)
        return self.loss.per_item(audio, target_values=target)

    def search(self, target_audio, **kw):
        """``evolve.evolve_search`` on this matcher's voice with its loss and frozen set (``kw``: generations, population,
        elites, init_params01, sigma0, alpha, sigma_min, sigma_max, seed) -> ``EvolveResult``; its ``params01[:, :S]`` are
        starts for ``fit(init_params01=...)``.  The multi-resolution loss is refused as by ``SpectralBank``: search with a
        mel matcher's loss through ``evolve_search`` instead."""
        return evolve_search(self.voice, self.loss, target_audio=target_audio, frozen=self.frozen, **kw)

    def fit(self, target_audio, init_params01=None, steps=200, return_audio=False):
        """target_audio [N, T] (device, T == voice.synthconfig.buffer_size); init_params01 [N, 78] in 0..1 (None: 0.5)
        -> ``MatchResult``.  Targets go through in chunks of ``voice.batch_size``; the last chunk is padded with inactive
        rows (zero cotangent, never updated, not returned).

        Several starts per sound: init_params01 [N, S, 78].  The N S rows are fitted as one flattened [N S, 78] fit
        (row n S + s fits target n from start s) and, per sound, the start with the lowest final loss is kept (ties: the
        lowest s; ``retrieval.rank_distances``).  ``loss``, ``initial_loss``, ``skipped`` and ``audio`` are the chosen
        start's; ``start``, ``start_loss`` and ``start_initial_loss`` say which and how every start ended."""
        voice = self.voice
        T = voice.synthconfig.buffer_size
        dev = voice.params01.device
        if target_audio.dim() != 2 or target_audio.shape[1] != T:
            raise ValueError(f"target_audio must be [N, {T}] (the voice's buffer), got {tuple(target_audio.shape)}")
        N = target_audio.shape[0]
        if init_params01 is not None and init_params01.dim() == 3:
            if init_params01.shape[0] != N or init_params01.shape[2] != S.NPARAMS or init_params01.shape[1] < 1:
                raise ValueError(f"init_params01 must be [{N}, {S.NPARAMS}] or [{N}, starts, {S.NPARAMS}], got "
                                 f"{tuple(init_params01.shape)}")
            return self._fit_starts(target_audio, init_params01, steps, return_audio)
        if init_params01 is None:
            init_params01 = torch.full((N, S.NPARAMS), 0.5, dtype=torch.float32, device=dev)
        if tuple(init_params01.shape) != (N, S.NPARAMS):
            raise ValueError(f"init_params01 must be [{N}, {S.NPARAMS}], got {tuple(init_params01.shape)}")
        return self._fit_rows(target_audio, init_params01, steps, return_audio)

    def _fit_rows(self, target_audio, init_params01, steps, return_audio):
        voice = self.voice
        B, dev = voice.batch_size, voice.params01.device
        N = target_audio.shape[0]
        target_audio = target_audio.detach().to(device=dev, dtype=torch.float32)
        init_params01 = init_params01.detach().to(device=dev, dtype=torch.float32).clamp(0.0, 1.0)
        outs = [self._fit_chunk(target_audio[s:s + B], init_params01[s:s + B], int(steps), return_audio)
                for s in range(0, N, B)]
        cat = lambda i: torch.cat([o[i] for o in outs])     # noqa: E731
        return MatchResult(params01=cat(0), loss=cat(1), initial_loss=cat(2), skipped=cat(3),
                           audio=cat(4) if return_audio else None)

    def _fit_starts(self, target_audio, init_params01, steps, return_audio):
        from .retrieval import rank_distances
        N, nS = init_params01.shape[0], init_params01.shape[1]
        flat = self._fit_rows(target_audio.repeat_interleave(nS, dim=0), init_params01.reshape(N * nS, S.NPARAMS),
                              steps, return_audio)
        start_loss = flat.loss.reshape(N, nS)
        start = rank_distances(start_loss)[:, 0]
        rows = torch.arange(N, device=start.device) * nS + start
        pick = lambda t: None if t is None else t[rows]      # noqa: E731
        return MatchResult(params01=pick(flat.params01), loss=pick(flat.loss), initial_loss=pick(flat.initial_loss),
                           skipped=pick(flat.skipped), audio=pick(flat.audio), start=start, start_loss=start_loss,
                           start_initial_loss=flat.initial_loss.reshape(N, nS))

    def _fit_chunk(self, target, init, steps, return_audio):
        voice = self.voice
        B, n = voice.batch_size, target.shape[0]
        dev = target.device
        active = torch.zeros(B, dtype=torch.uint8, device=dev)
        active[:n] = 1
        if n < B:                                    # padded rows: silence against centre parameters
            target = torch.cat([target, target.new_zeros((B - n, target.shape[1]))])
            init = torch.cat([init, init.new_full((B - n, S.NPARAMS), 0.5)])
        cot = active.to(torch.float32)
        with torch.no_grad():
            tgt = self.loss.target(target)
        p = init.clone().contiguous()
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        step = torch.zeros(B, dtype=torch.int32, device=dev)
        skipped = torch.zeros(B, dtype=torch.int32, device=dev)
        best_loss = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)
        best_params = p.clone()
        initial = None
        for _ in range(steps):
            q = p.clone().requires_grad_(True)
            loss = self._per_item(voice.render(q, normalize=True), tgt)
            if initial is None:
                initial = loss.detach().clone()
            loss.backward(cot)
            match_adam_step(p, q.grad, m, v, step, loss.detach(), best_loss, best_params, self.free, active, skipped,
                            self.lr, self.betas, self.eps)
        with torch.no_grad():                        # the last parameters compete for "best" too
            last = self._per_item(voice.render(p, normalize=True), tgt)
            if initial is None:
                initial = last.clone()
            better = (active != 0) & (last.double() < best_loss)
            best_params = torch.where(better.unsqueeze(1), p, best_params)
            best_loss = torch.where(better, last.double(), best_loss)
            audio = voice.render(best_params, normalize=True)[:n].clone() if return_audio else None
        return best_params[:n], best_loss[:n].float(), initial[:n], skipped[:n], audio

    def tied_mask(self, own=DEFAULT_OWN):
        """-> [78] uint8 on the voice's device: 1 for the columns ``fit_tied`` ties, every non-frozen column that is not
        in ``own`` ((module, name) pairs; an unknown one raises KeyError, as in ``frozen``)."""
        own = [tuple(k) for k in own]
        for k in own:
            if k not in S.INDEX:
                raise KeyError(f"unknown Voice parameter {k}")
        mask = self.free.clone()
        if own:
            mask[[S.INDEX[k] for k in own]] = 0
        return mask

    def _chunks(self, target_audio):
        """The chunks of ``voice.batch_size`` rows of [N, T] targets -> [(first row, rows, the loss's target of the chunk
        padded with silence, its cotangent [B]: 1 for a row, 0 for padding)]."""
        B, N = self.voice.batch_size, target_audio.shape[0]
        chunks = []
        for s in range(0, N, B):
            target = target_audio[s:s + B]
            n = target.shape[0]
            if n < B:                                # padded rows: silence against centre parameters, as in _fit_chunk
                target = torch.cat([target, target.new_zeros((B - n, target.shape[1]))])
            cot = torch.zeros(B, dtype=torch.float32, device=target.device)
            cot[:n] = 1.0
            with torch.no_grad():
                chunks.append((s, n, self.loss.target(target), cot))
        return chunks

    def _padded(self, p, s, n):
        B = self.voice.batch_size
        rows = p[s:s + n]
        return rows if n == B else torch.cat([rows, rows.new_full((B - n, S.NPARAMS), 0.5)])

    def _forward_all(self, chunks, p, loss_out, audio_out=None):
        with torch.no_grad():
            for s, n, tgt, _cot in chunks:
                audio = self.voice.render(self._padded(p, s, n).contiguous(), normalize=True)
                loss_out[s:s + n] = self._per_item(audio, tgt)[:n]
                if audio_out is not None:
                    audio_out[s:s + n] = audio[:n]

    def fit_tied(self, target_audio, groups, init_params01=None, own=DEFAULT_OWN, steps=200, return_audio=False):
        """target_audio [N, T] as for ``fit``; groups [N]: non-decreasing integer group ids starting at 0 (``group_starts``:
        the one host check, before the loop; ValueError otherwise); init_params01 [N, 78] (None: 0.5) ->
        ``TiedMatchResult``.  The rows of a group are fitted as one instrument: every free column outside ``own`` is
        TIED, one value per group, which moves along the mean of the rows' gradients; the ``own`` columns stay per row.
        A start whose rows disagree in a tied column takes the group's first row there (``tie_starts``).

        Each iteration walks all chunks of ``voice.batch_size`` rows (render, ``per_item``, ``backward`` with the active
        cotangent; the last chunk padded as in ``fit``), writes the chunk's gradient and loss into [N, 78] and [N]
        buffers and ends in one ``ias_match_tied_step`` over all N rows, so a group may cross chunks.  After the last
        iteration one forward pass lets the last parameters compete for best (``update=0``).  With one row per group
        this is ``fit``, bit for bit."""
        voice = self.voice
        T = voice.synthconfig.buffer_size
        dev = voice.params01.device
        if target_audio.dim() != 2 or target_audio.shape[1] != T:
            raise ValueError(f"target_audio must be [N, {T}] (the voice's buffer), got {tuple(target_audio.shape)}")
        N = target_audio.shape[0]
        group_start = group_starts(groups, N).to(dev)
        G = group_start.shape[0] - 1
        if init_params01 is None:
            init_params01 = torch.full((N, S.NPARAMS), 0.5, dtype=torch.float32, device=dev)
        if tuple(init_params01.shape) != (N, S.NPARAMS):
            raise ValueError(f"init_params01 must be [{N}, {S.NPARAMS}], got {tuple(init_params01.shape)}")
        tied = self.tied_mask(own)
        ids = torch.as_tensor(groups).to(device=dev, dtype=torch.int64)
        target_audio = target_audio.detach().to(device=dev, dtype=torch.float32)
        init = init_params01.detach().to(device=dev, dtype=torch.float32).clamp(0.0, 1.0)
        p = tie_starts(init, ids, tied).contiguous()
        chunks = self._chunks(target_audio)
        m, v, grad = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
        loss = torch.zeros(N, dtype=torch.float32, device=dev)
        step = torch.zeros(G, dtype=torch.int32, device=dev)
        skipped = torch.zeros(G, dtype=torch.int32, device=dev)
        active = torch.ones(G, dtype=torch.uint8, device=dev)
        best_loss = torch.full((G,), float("inf"), dtype=torch.float64, device=dev)
        group_loss = torch.zeros(G, dtype=torch.float64, device=dev)
        best_params = p.clone()
        initial = initial_group = None

        def tied_step(update):
            tied_adam_step(p, grad, m, v, best_params, loss, group_start, step, skipped, best_loss, group_loss, self.free,
                           tied, active, update, self.lr, self.betas, self.eps)

        for _ in range(int(steps)):
            for s, n, tgt, cot in chunks:
                q = self._padded(p, s, n).clone().requires_grad_(True)
                rows = self._per_item(voice.render(q, normalize=True), tgt)
                rows.backward(cot)
                grad[s:s + n] = q.grad[:n]
                loss[s:s + n] = rows.detach()[:n]
            tied_step(1)
            if initial is None:
                initial, initial_group = loss.clone(), group_loss.clone()
        self._forward_all(chunks, p, loss)           # the last parameters compete for "best" too
        tied_step(0)
        if initial is None:
            initial, initial_group = loss.clone(), group_loss.clone()
        audio = target_audio.new_zeros((N, T)) if return_audio else None
        final = torch.zeros_like(loss)
        self._forward_all(chunks, best_params, final, audio)
        return TiedMatchResult(params01=best_params, loss=final, group_loss=best_loss, initial_loss=initial,
                               initial_group_loss=initial_group, skipped=skipped, audio=audio)

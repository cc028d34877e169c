"""Sound matching: fit the 78 Voice parameters to given audio, each sound on its own.

This closes the loop the reference left commented out (/root/reference/audio_to_params.py:56-172: params -> synth ->
mel-L1 against the true audio) as a product feature, and returns what its notebook wanted in the end
(/root/reference/evaluate_audio_representations.py:202-231): a candidate and a distance per target sound.

``fit`` and ``fit_tied`` are one descent routine (``SoundMatcher._descend``) with two optimiser steps.  It owns the padding
of its rows to whole chunks of ``voice.batch_size``, the state, the iterations, the final pass in which the last
parameters compete for best, and the gain column.  Per chunk, every iteration is

    audio = voice.render(p)                      HIP render with its adjoint (voice_grad.py), normalize=True
    L     = loss.per_item(audio, target)         [B] per-sound spectral L1 or MR-STFT (spectral.py, csrc/match_kernels.hip)
    L.backward(active)                           per-row cotangent (the ``rows`` form of spectral._L1Fn / _MRSTFTFn:
                                                 ias_stft_loss_backward_rows, ias_mrstft_coef_rows + the *_mrstft_rows
                                                 span / frame kernels): a sound's gradient does not depend on the
                                                 batch, padded rows get exactly 0

and then one step over all its rows: ``ias_match_adam_step`` (best-so-far, non-finite skip, Adam per row, clamp to
[0, 1]) or ``ias_match_tied_step`` (csrc/match_step_kernels.hip), with all state on the device and no host read inside
the loop.  ``fit`` hands the routine one chunk at a time, all its steps, so that one chunk's loss target is alive at once;
the step then reads the chunk's gradient and loss where backward left them.

``fit_tied`` fits the notes of a phrase to ONE instrument: the rows of a group share every free column that is not one of
the group's ``own`` columns (by default the note and its length).  It hands the routine all N rows: each iteration walks
all chunks, collects the rows' gradients and losses in [rows, 78] and [rows] buffers and ends in one
``ias_match_tied_step`` (include/ias_hip_tied.h) over the N rows: the mean gradient of a tied column over the group, one
Adam update, the result written to every row.

``gain="solved"`` / ``gain="fitted"`` (``fit`` and ``fit_tied``) add an output gain per sound, in dB, beside the 78
parameters: the loss is taken on ``apply_gain(render, g)``, where g starts at the closed-form ``solve_gain`` of the target
against the start's render and, when fitted, is the optimiser's 79th column (include/ias_hip_gain.h has the gain law and
the three entry points).  The Voice and ``voice_spec.PARAMS`` know nothing of it.
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
GAINS = (None, "solved", "fitted")
GAIN_DB_LO, GAIN_DB_HI = -60.0, 20.0                 # the gain law of include/ias_hip_gain.h: g01 0 .. 1 is LO .. HI dB
GAIN_UNITY01 = 0.75                                  # 0 dB, exact in fp32


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
    gain_db: Optional[torch.Tensor] = None               # [N] fp32: the output gain of ``audio`` and ``loss`` (fit(gain=...))
    initial_gain_db: Optional[torch.Tensor] = None       # [N] fp32: the gain the fit started from


@dataclass
class TiedMatchResult:
    params01: torch.Tensor          # [N, 78] best parameters: the rows of a group agree in every tied column
    loss: torch.Tensor              # [N] fp32: the per-note loss of params01, from a fresh forward
    group_loss: torch.Tensor        # [G] fp64: the best mean loss of every group (the mean of ``loss`` over its rows)
    initial_loss: torch.Tensor      # [N] fp32: the per-note loss of the (tied) start
    initial_group_loss: torch.Tensor    # [G] fp64
    skipped: torch.Tensor           # [G] int32: iterations a group skipped for a non-finite loss or gradient
    audio: Optional[torch.Tensor] = None   # [N, T] render of params01 (fit_tied(return_audio=True))
    gain_db: Optional[torch.Tensor] = None               # [N] fp32: every note's output gain (fit_tied(gain=...))
    initial_gain_db: Optional[torch.Tensor] = None       # [N] fp32


@dataclass
class _Descent:
    """What ``SoundMatcher._descend`` leaves, over its rows padded to whole chunks."""
    best_params: torch.Tensor       # [rows, 78 or 79 (gain="fitted": the gain column)]
    best_loss: torch.Tensor         # [rows] or [G] fp64
    skipped: torch.Tensor           # [rows] or [G] int32
    chunks: list                    # per chunk (its rows as a slice, the loss's target, cotangent [B], views of p and g)
    gain: Optional[str]
    gain01: Optional[torch.Tensor]  # [rows]: the gain the descent started from (and, "solved", kept)
    initial_loss: Optional[torch.Tensor] = None          # [rows] fp32
    group_loss: Optional[torch.Tensor] = None            # [G] fp64 (tied): the last step's
    initial_group_loss: Optional[torch.Tensor] = None    # [G] fp64 (tied)


def _check_arrays(what, table):
    """The argument check of the step wrappers: ``table`` of (tensor, dtype, shape), each to be contiguous."""
    for t, dt, shape in table:
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{what}: expected a contiguous {dt} tensor of shape {shape}, got {t.dtype} {tuple(t.shape)}")


def match_adam_step(params01, grad, m, v, step, loss, best_loss, best_params, free, active, skipped, lr, betas, eps):
    """One launch of ias_match_adam_step over [B, P] (see include/ias_hip.h).  Updates params01, m, v, step, best_loss,
    best_params and skipped in place."""
    B, P = params01.shape
    f32, i32, u8 = torch.float32, torch.int32, torch.uint8
    _check_arrays("match_adam_step", ((params01, f32, (B, P)), (grad, f32, (B, P)), (m, f32, (B, P)), (v, f32, (B, P)),
                                      (best_params, f32, (B, P)), (step, i32, (B,)), (loss, f32, (B,)),
                                      (best_loss, torch.float64, (B,)), (free, u8, (P,)), (active, u8, (B,)),
                                      (skipped, i32, (B,))))
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
    f32, i32, f64, u8 = torch.float32, torch.int32, torch.float64, torch.uint8
    _check_arrays("tied_adam_step", ((params01, f32, (N, P)), (grad, f32, (N, P)), (m, f32, (N, P)), (v, f32, (N, P)),
                                     (best_params, f32, (N, P)), (loss, f32, (N,)), (group_start, i32, (G + 1,)),
                                     (step, i32, (G,)), (skipped, i32, (G,)), (best_loss, f64, (G,)),
                                     (group_loss, f64, (G,)), (free, u8, (P,)), (tied, u8, (P,)), (active, u8, (G,))))
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


# ------------------------------------------------------------------------------------------------ output gain
def gain01_from_db(db):
    """dB (tensor) -> the gain column's value g01, fp32, clamped to GAIN_DB_LO .. GAIN_DB_HI (0 dB -> 0.75)."""
    return ((db.double() - GAIN_DB_LO) / (GAIN_DB_HI - GAIN_DB_LO)).clamp(0.0, 1.0).float()


def gain_db_from01(gain01):
    """g01 (fp32 tensor) -> dB, fp32 (formed in fp64 as the kernels form it)."""
    return (GAIN_DB_LO + (GAIN_DB_HI - GAIN_DB_LO) * gain01.double()).float()


def _gain_rows(what, rows, vectors):
    """The checks of the gain entry points: ``rows`` contiguous fp32 [B, T] of one shape, ``vectors`` contiguous fp32 [B]."""
    shape = tuple(rows[0].shape)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"{what}: expected [B, T] rows, got {shape}")
    for t in rows:
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{what}: expected a contiguous float32 tensor of shape {shape}, got {t.dtype} {tuple(t.shape)}")
    for t in vectors:
        if t.dtype != torch.float32 or tuple(t.shape) != shape[:1] or not t.is_contiguous():
            raise ValueError(f"{what}: expected a contiguous float32 tensor of shape {shape[:1]}, got {t.dtype} "
                             f"{tuple(t.shape)}")
    return shape


def _gain_partials(B, T, width, dev):
    n = _lib.load().ias_gain_partials_count(T)
    _lib.check(min(n, 0), "ias_gain_partials_count")
    return torch.empty((B, n, width), dtype=torch.float64, device=dev)


def gain_forward(audio, gain01):
    """ias_gain_apply: audio [B, T], gain01 [B] -> a new [B, T] tensor a_b audio[b] (include/ias_hip_gain.h)."""
    B, T = _gain_rows("gain_forward", (audio,), (gain01,))
    out = torch.empty_like(audio)
    st = _lib.load().ias_gain_apply(_lib.ptr(audio), _lib.ptr(gain01), _lib.ptr(out), B, T, _lib.stream())
    _lib.check(st, "ias_gain_apply")
    return out


def gain_backward(g_out, audio, gain01):
    """ias_gain_backward: the cotangent g_out [B, T] of ``gain_forward(audio, gain01)`` -> (g_audio [B, T], g_gain01 [B])."""
    B, T = _gain_rows("gain_backward", (g_out, audio), (gain01,))
    g_audio, g_gain01 = torch.empty_like(audio), torch.empty_like(gain01)
    partials = _gain_partials(B, T, 1, audio.device)
    st = _lib.load().ias_gain_backward(_lib.ptr(g_out), _lib.ptr(audio), _lib.ptr(gain01), _lib.ptr(g_audio),
                                       _lib.ptr(g_gain01), _lib.ptr(partials), B, T, _lib.stream())
    _lib.check(st, "ias_gain_backward")
    return g_audio, g_gain01


class _ApplyGain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, audio, gain01):
        ctx.save_for_backward(audio, gain01)
        return gain_forward(audio, gain01)

    @staticmethod
    def backward(ctx, g_out):
        audio, gain01 = ctx.saved_tensors
        return gain_backward(g_out.contiguous(), audio, gain01)


def apply_gain(audio, gain01):
    """audio [B, T] fp32, gain01 [B] fp32 (g01 of the gain law: 0 .. 1 is -60 .. +20 dB, 0.75 is 0 dB) -> a_b audio[b] as a
    new tensor, differentiable in both (ias_gain_apply / ias_gain_backward)."""
    return _ApplyGain.apply(audio.contiguous(), gain01.contiguous())


def solve_gain(target, render):
    """target, render [B, T] fp32 -> g01 [B] fp32: the gain that gives ``render`` the energy of ``target``, clamped to the
    range; 0.75 (0 dB) where either is silent or not finite (ias_gain_solve).  Not differentiable."""
    target, render = target.detach().contiguous(), render.detach().contiguous()
    B, T = _gain_rows("solve_gain", (target, render), ())
    g01 = torch.empty(B, dtype=torch.float32, device=target.device)
    partials = _gain_partials(B, T, 2, target.device)
    st = _lib.load().ias_gain_solve(_lib.ptr(target), _lib.ptr(render), _lib.ptr(g01), _lib.ptr(partials), B, T,
                                    _lib.stream())
    _lib.check(st, "ias_gain_solve")
    return g01


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

    def _gain_args(self, gain, init_gain_db, N):
        """The ``gain`` and ``init_gain_db`` of ``fit`` / ``fit_tied``, checked -> the start's g01 [N] on the voice's
        device (clamped to the range), or None: solve it."""
        if gain not in GAINS:
            raise ValueError(f"gain must be one of {GAINS}, got {gain!r}")
        if init_gain_db is None:
            return None
        if gain is None:
            raise ValueError("init_gain_db needs gain='solved' or gain='fitted'")
        db = torch.as_tensor(init_gain_db).detach().to(device=self.voice.params01.device)
        if tuple(db.shape) != (N,):
            raise ValueError(f"init_gain_db must be [{N}] (dB, one per target), got {tuple(db.shape)}")
        return gain01_from_db(db).contiguous()

    def _render(self, q, gain=None, g=None):
        """The audio the loss sees: q [B, 78] rendered and, with a gain, scaled by the fixed g [B] ("solved"); q [B, 79]:
        the render of its first 78 columns scaled by its last ("fitted")."""
        if gain is None:
            return self.voice.render(q, normalize=True)
        if gain == "fitted":
            return apply_gain(self.voice.render(q[:, :S.NPARAMS].contiguous(), normalize=True), q[:, S.NPARAMS])
        return apply_gain(self.voice.render(q, normalize=True), g)

    def _fit_inputs(self, target_audio, init_params01, starts=False, groups=None):
        """The checks ``fit`` and ``fit_tied`` share -> (N, init_params01 or the centre, ``group_starts(groups, N)`` on the
        voice's device or None).  ``starts``: init_params01 may be [N, starts, 78]."""
        T, dev = self.voice.synthconfig.buffer_size, self.voice.params01.device
        if target_audio.dim() != 2 or target_audio.shape[1] != T:
            raise ValueError(f"target_audio must be [N, {T}] (the voice's buffer), got {tuple(target_audio.shape)}")
        N = target_audio.shape[0]
        group_start = None if groups is None else group_starts(groups, N).to(dev)
        if starts and init_params01 is not None and init_params01.dim() == 3:
            if init_params01.shape[0] != N or init_params01.shape[2] != S.NPARAMS or init_params01.shape[1] < 1:
                raise ValueError(f"init_params01 must be [{N}, {S.NPARAMS}] or [{N}, starts, {S.NPARAMS}], got "
                                 f"{tuple(init_params01.shape)}")
            return N, init_params01, group_start
        if init_params01 is None:
            init_params01 = torch.full((N, S.NPARAMS), 0.5, dtype=torch.float32, device=dev)
        if tuple(init_params01.shape) != (N, S.NPARAMS):
            raise ValueError(f"init_params01 must be [{N}, {S.NPARAMS}], got {tuple(init_params01.shape)}")
        return N, init_params01, group_start

    def fit(self, target_audio, init_params01=None, steps=200, return_audio=False, gain=None, init_gain_db=None):
        """target_audio [N, T] (device, T == voice.synthconfig.buffer_size); init_params01 [N, 78] in 0..1 (None: 0.5)
        -> ``MatchResult``.  Targets go through in chunks of ``voice.batch_size``; the last chunk is padded with inactive
        rows (zero cotangent, never updated, not returned).

        Several starts per sound: init_params01 [N, S, 78].  The N S rows are fitted as one flattened [N S, 78] fit
        (row n S + s fits target n from start s) and, per sound, the start with the lowest final loss is kept (ties: the
        lowest s; ``retrieval.rank_distances``).  ``loss``, ``initial_loss``, ``skipped`` and ``audio`` are the chosen
        start's; ``start``, ``start_loss`` and ``start_initial_loss`` say which and how every start ended.

        ``gain``: None (no gain: the [B, 78] path as it was), "solved" or "fitted".  With either, every sound has an
        output gain g in dB (``GAIN_DB_LO`` .. ``GAIN_DB_HI``) and the loss is taken on ``apply_gain(render, g)``, in every
        iteration, in the final pass and for ``steps=0``.  g starts at ``solve_gain(target, render of the start)``, or at
        ``init_gain_db`` [N] (clamped to the range) where given.  "solved": g stays there.  "fitted": g is the 79th
        column of the optimiser's state (free, whatever ``frozen`` says; clamped to the range by the step's clamp to
        0 .. 1), and best-so-far covers all 79 columns.  Padded rows carry 0 dB.  ``params01`` stays [N, 78]; ``gain_db``
        and ``initial_gain_db`` [N] are the returned and the starting gain, ``audio`` is the gained render and ``loss`` its
        loss.  With several starts, ``init_gain_db`` [N] goes to every start of a sound."""
        N, init_params01, _ = self._fit_inputs(target_audio, init_params01, starts=True)
        g0 = self._gain_args(gain, init_gain_db, N)
        run = self._fit_starts if init_params01.dim() == 3 else self._fit_rows
        return run(target_audio, init_params01, steps, return_audio, gain, g0)

    def _fit_rows(self, target_audio, init_params01, steps, return_audio, gain=None, g0=None):
        voice = self.voice
        B, dev = voice.batch_size, voice.params01.device
        N = target_audio.shape[0]
        target_audio = target_audio.detach().to(device=dev, dtype=torch.float32)
        init_params01 = init_params01.detach().to(device=dev, dtype=torch.float32).clamp(0.0, 1.0)
        outs = [self._fit_chunk(target_audio[s:s + B], init_params01[s:s + B], int(steps), return_audio, gain,
                                None if g0 is None else g0[s:s + B])
                for s in range(0, N, B)]
        cat = lambda i: torch.cat([o[i] for o in outs])     # noqa: E731
        return MatchResult(params01=cat(0), loss=cat(1), initial_loss=cat(2), skipped=cat(3),
                           audio=cat(4) if return_audio else None, gain_db=None if gain is None else cat(5),
                           initial_gain_db=None if gain is None else cat(6))

    def _fit_starts(self, target_audio, init_params01, steps, return_audio, gain=None, g0=None):
        from .retrieval import rank_distances
        N, nS = init_params01.shape[0], init_params01.shape[1]
        flat = self._fit_rows(target_audio.repeat_interleave(nS, dim=0), init_params01.reshape(N * nS, S.NPARAMS),
                              steps, return_audio, gain, None if g0 is None else g0.repeat_interleave(nS))
        start_loss = flat.loss.reshape(N, nS)
        start = rank_distances(start_loss)[:, 0]
        rows = torch.arange(N, device=start.device) * nS + start
        pick = lambda t: None if t is None else t[rows]      # noqa: E731
        return MatchResult(params01=pick(flat.params01), loss=pick(flat.loss), initial_loss=pick(flat.initial_loss),
                           skipped=pick(flat.skipped), audio=pick(flat.audio), start=start, start_loss=start_loss,
                           start_initial_loss=flat.initial_loss.reshape(N, nS), gain_db=pick(flat.gain_db),
                           initial_gain_db=pick(flat.initial_gain_db))

    def _fit_chunk(self, target, init, steps, return_audio, gain=None, g0=None):
        """One chunk of ``fit``, all its steps: what leaves this frame holds no loss target, so one chunk's is alive at a
        time (an MR-STFT target of the flagship shapes is over a gigabyte)."""
        n = target.shape[0]
        d = self._descend(target, init, steps, gain, g0)
        audio = None
        if return_audio:
            audio = target.new_zeros(target.shape)
            self._forward(d, d.best_params, audio_out=audio)
        return (d.best_params[:n, :S.NPARAMS], d.best_loss[:n].float(), d.initial_loss[:n], d.skipped[:n], audio,
                *self._gain_db(d, n))

    def _descend(self, target, init, steps, gain=None, g0=None, tied=None):
        """The descent under ``fit`` and ``fit_tied``: target [n, T] and init [n, 78] on the device (n >= 1 rows: a chunk
        of ``fit``, all rows of ``fit_tied``), g0 [n] or None -> ``_Descent``.  All state is padded to whole chunks of
        ``voice.batch_size`` rows once: centre parameters, 0 dB, silence targets, rows that are inactive (untied) or in no
        group (tied: the step sees the first n rows alone).  A row keeps its place in its chunk, which fixes its noise.
        ``tied``: None, the per-row ``match_adam_step``, or (group_start [G + 1], tied mask [78]), ``tied_adam_step``;
        nothing else differs.  An iteration is, per chunk, the clone of its parameters, render, loss and backward, then
        one step; with one chunk the step reads q.grad and the loss themselves, with several they are collected in
        [rows, P] and [rows] buffers.  The last parameters compete for best in a final forward (the step's best-so-far
        pass alone).  No host read."""
        B, n, dev = self.voice.batch_size, target.shape[0], target.device
        M = -(-n // B) * B
        real = torch.arange(M, device=dev) < n
        if n < M:
            target = torch.cat([target, target.new_zeros((M - n, target.shape[1]))])
            init = torch.cat([init, init.new_full((M - n, S.NPARAMS), 0.5)])
        spans = [slice(s, s + B) for s in range(0, M, B)]
        free, mask, g = self.free, None if tied is None else tied[1], None
        if gain is not None:
            if g0 is not None:
                g = torch.cat([g0, g0.new_full((M - n,), GAIN_UNITY01)]).contiguous()
            else:                                    # per chunk: the padded target against the padded start (silence: 0 dB)
                with torch.no_grad():
                    g = torch.cat([solve_gain(target[rows], self.voice.render(init[rows].contiguous(), normalize=True))
                                   for rows in spans])
            if gain == "fitted":                     # the 79th column: free, and under ``fit_tied`` every note's own
                init = torch.cat([init, g.unsqueeze(1)], dim=1)
                free = torch.cat([free, free.new_ones(1)])
                mask = None if mask is None else torch.cat([mask, mask.new_zeros(1)])
        p = init.clone().contiguous()
        cot = real.to(torch.float32)
        with torch.no_grad():                        # per chunk: its rows, loss target, cotangent and views of its p and g
            chunks = [(rows, self.loss.target(target[rows]), cot[rows], p[rows], None if g is None else g[rows])
                      for rows in spans]
        m, v, best_params = torch.zeros_like(p), torch.zeros_like(p), p.clone()
        K = M if tied is None else tied[0].shape[0] - 1          # counters: per row, or per group
        step = torch.zeros(K, dtype=torch.int32, device=dev)
        skipped = torch.zeros(K, dtype=torch.int32, device=dev)
        best_loss = torch.full((K,), float("inf"), dtype=torch.float64, device=dev)
        d = _Descent(best_params, best_loss, skipped, chunks, gain, g)
        if tied is None:
            active = real.to(torch.uint8)

            def take_step(grad, loss, update):
                if update:
                    return match_adam_step(p, grad, m, v, step, loss, best_loss, best_params, free, active, skipped,
                                           self.lr, self.betas, self.eps)
                better = real & (loss.double() < best_loss)
                best_params.copy_(torch.where(better.unsqueeze(1), p, best_params))
                best_loss.copy_(torch.where(better, loss.double(), best_loss))
        else:
            active = torch.ones(K, dtype=torch.uint8, device=dev)
            d.group_loss = torch.zeros(K, dtype=torch.float64, device=dev)

            def take_step(grad, loss, update):
                tied_adam_step(p[:n], grad[:n], m[:n], v[:n], best_params[:n], loss[:n], tied[0], step, skipped, best_loss,
                               d.group_loss, free, mask, active, update, self.lr, self.betas, self.eps)

        def started(loss):
            if d.initial_loss is None:
                d.initial_loss = loss.clone()
                d.initial_group_loss = None if tied is None else d.group_loss.clone()

        grad, loss = torch.zeros_like(p), torch.zeros(M, dtype=torch.float32, device=dev)
        for _ in range(steps):
            for rows, tgt, c, p_rows, g_rows in chunks:
                q = p_rows.clone().requires_grad_(True)
                rows_loss = self._per_item(self._render(q, gain, g_rows), tgt)
                rows_loss.backward(c)
                if len(chunks) == 1:
                    grad, loss = q.grad, rows_loss.detach()
                else:
                    grad[rows], loss[rows] = q.grad, rows_loss.detach()
            take_step(grad, loss, 1)
            started(loss)
        last = torch.zeros(M, dtype=torch.float32, device=dev)
        self._forward(d, p, last)                    # the last parameters compete for "best" too
        take_step(grad, last, 0)
        started(last)
        return d

    def _forward(self, d, p, loss_out=None, audio_out=None):
        """Render p [rows of ``d``, 78 or 79] chunk by chunk with ``d``'s gain -> the rows' losses into loss_out and their
        audio into audio_out (either None: not wanted), as many rows as each holds."""
        with torch.no_grad():
            for rows, tgt, _cot, _p, g_rows in d.chunks:
                audio = self._render(p[rows].contiguous(), d.gain, g_rows)
                if loss_out is not None:             # an output shorter than the padded rows ends inside the last chunk
                    loss_out[rows] = self._per_item(audio, tgt)[:loss_out[rows].shape[0]]
                if audio_out is not None:
                    audio_out[rows] = audio[:audio_out[rows].shape[0]]

    @staticmethod
    def _gain_db(d, n):
        """-> (gain_db, initial_gain_db) [n] of a descent's best parameters and of its start; (None, None) without a gain."""
        if d.gain is None:
            return None, None
        best = d.best_params[:n, S.NPARAMS] if d.gain == "fitted" else d.gain01[:n]
        return gain_db_from01(best), gain_db_from01(d.gain01[:n])

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

    def fit_tied(self, target_audio, groups, init_params01=None, own=DEFAULT_OWN, steps=200, return_audio=False,
                 gain=None, init_gain_db=None):
        """target_audio [N, T] as for ``fit``; groups [N]: non-decreasing integer group ids starting at 0 (``group_starts``:
        the one host check, before the loop; ValueError otherwise); init_params01 [N, 78] (None: 0.5) ->
        ``TiedMatchResult``.  The rows of a group are fitted as one instrument: every free column outside ``own`` is
        TIED, one value per group, which moves along the mean of the rows' gradients; the ``own`` columns stay per row.
        A start whose rows disagree in a tied column takes the group's first row there (``tie_starts``).

        The descent is ``fit``'s (``_descend``) over all N rows at once: each iteration walks all chunks of
        ``voice.batch_size`` rows (the last one padded as in ``fit``) and ends in one ``ias_match_tied_step`` over the N
        rows, so a group may cross chunks.  With one row per group this is ``fit``, bit for bit.  ``loss`` and ``audio``
        are a fresh forward of the best parameters.

        ``gain`` and ``init_gain_db`` as for ``fit``: one output gain per NOTE, which is the note's velocity under tied
        mixer levels.  "fitted": the arrays of the step are [N, 79] and the gain column is always an own column,
        whatever ``own`` says."""
        dev = self.voice.params01.device
        N, init_params01, group_start = self._fit_inputs(target_audio, init_params01, groups=groups)
        tied = self.tied_mask(own)
        g0 = self._gain_args(gain, init_gain_db, N)
        ids = torch.as_tensor(groups).to(device=dev, dtype=torch.int64)
        target_audio = target_audio.detach().to(device=dev, dtype=torch.float32)
        init = init_params01.detach().to(device=dev, dtype=torch.float32).clamp(0.0, 1.0)
        d = self._descend(target_audio, tie_starts(init, ids, tied), int(steps), gain, g0, tied=(group_start, tied))
        final = torch.zeros(N, dtype=torch.float32, device=dev)
        audio = target_audio.new_zeros(target_audio.shape) if return_audio else None
        self._forward(d, d.best_params, final, audio)
        gain_db, initial_gain_db = self._gain_db(d, N)
        return TiedMatchResult(params01=d.best_params[:N, :S.NPARAMS].contiguous(), loss=final, group_loss=d.best_loss,
                               initial_loss=d.initial_loss[:N], initial_group_loss=d.initial_group_loss, skipped=d.skipped,
                               audio=audio, gain_db=gain_db, initial_gain_db=initial_gain_db)

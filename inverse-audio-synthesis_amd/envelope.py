"""Envelope stage of sound matching: how long a target sounds and how it rises and falls, read off its RMS envelope.

``keyboard.duration`` and the ADSR times are the columns where a spectral L1 is flat or misleading:
a render that is silent where the target sounds gives no gradient that lengthens the note.  The Voice's own envelope law is
six numbers (``COLUMNS``), and fitting it to the target's envelope needs no audio render: ``envelope_frames``
(ias_envelope_frames) takes the RMS per frame, ``envelope_score`` (ias_envelope_score) gives the distance 1 - cos^2 between
it and the law for a whole population of candidates, and ``fit_envelope`` runs the evolutionary search's loop
(``evolve.cross_entropy_search``: ias_evolve_sample, ias_topk_merge, ias_evolve_update) with that scorer.  ``reshape``
writes the result into the starts of a fit (``match_audio.py --envelope``).  One note per sound is
assumed, as by ``pitch.estimate_pitch``.

The six parameters are not identifiable one by one (a short note with a long attack has the envelope of a longer note with
a short one); what the stage finds is an envelope, and ``EnvelopeFit.dist`` says how near it is.
"""
from dataclasses import dataclass
from types import SimpleNamespace

import torch

from . import _lib
from . import voice_spec as S
from .evolve import cross_entropy_search, evolve_sample, evolve_update
from .retrieval import topk_merge

COLUMNS = ("duration", "attack", "decay", "sustain", "release", "alpha")
LDS_BUDGET_BYTES = 65536            # ias_envelope_score's LDS budget: a row of env, 4 F bytes (include/ias_hip.h)

_DURATION = S.INDEX[("keyboard", "duration")]
_ADSR = tuple(tuple(S.INDEX[(mod, name)] for name in COLUMNS[1:]) for mod in ("adsr_1", "adsr_2"))


@dataclass
class EnvelopeFit:
    params01: torch.Tensor          # [N, 6] fp32 in 0..1: the best elite, columns as ``COLUMNS``
    dist: torch.Tensor              # [N] fp32: its distance
    start_dist: torch.Tensor        # [N] fp32: the distance of the start (candidate 0 of generation 0)
    sounding: torch.Tensor          # [N] bool: the row's largest rms is > 0
    units: torch.Tensor             # [N, 6] fp64: params01 in seconds (sustain and alpha: plain numbers)
    rms: torch.Tensor               # [N, F] fp32: the target's envelope


def to_units(params01):
    """[..., 6] in 0..1 -> fp64 units by the Voice's parameter table (``voice_spec``), as ias_envelope_score maps them: the
    six columns have curve 0.5 (a square) or 1 (linear)."""
    u = params01.double()
    sq = u * u
    return torch.stack([0.01 + 3.99 * sq[..., 0], 2.0 * sq[..., 1], 2.0 * sq[..., 2], u[..., 3], 5.0 * sq[..., 4],
                        0.1 + 5.9 * u[..., 5]], dim=-1)


def num_frames(T, W, hop):
    """ias_envelope_num_frames: (T - W) // hop + 1, ValueError when not even one frame fits."""
    F = _lib.load().ias_envelope_num_frames(int(T), int(W), int(hop))
    if F < 1:
        raise ValueError(f"envelope: no frame fits: T = {T}, W = {W}, hop = {hop} (need sizes >= 1 and T >= W)")
    return F


def envelope_frames(audio, W, hop):
    """One launch of ias_envelope_frames (include/ias_hip.h) on audio [B, T] (device fp32, contiguous) -> rms [B, F] fp32,
    F = (T - W) // hop + 1; frame f is the root mean square of audio[:, f hop : f hop + W], summed in fp64."""
    if audio.dim() != 2 or audio.dtype != torch.float32 or not audio.is_contiguous():
        raise ValueError(f"envelope_frames: audio must be a contiguous float32 [B, T] tensor, got {audio.dtype} "
                         f"{tuple(audio.shape)}")
    B, T = audio.shape
    W, hop = int(W), int(hop)
    if B < 1 or W < 1 or hop < 1:
        raise ValueError(f"envelope_frames: need B, W, hop >= 1, got B = {B}, W = {W}, hop = {hop}")
    F = num_frames(T, W, hop)
    if B > 65535:
        raise ValueError(f"envelope_frames: at most 65535 rows per call, got {B}")
    rms = torch.empty((B, F), dtype=torch.float32, device=audio.device)
    st = _lib.load().ias_envelope_frames(_lib.ptr(audio), B, T, W, hop, _lib.ptr(rms), _lib.stream())
    _lib.check(st, "ias_envelope_frames")
    return rms


def envelope_score(env, cand, t0, dt, out=None):
    """One launch of ias_envelope_score (include/ias_hip.h): env [N, F] and cand [N, M, 6] in 0..1 (device fp32,
    contiguous), frame f at ``t0 + f dt`` seconds -> dist [N, M] fp32, 1 - cos^2 between the row of env and the envelope
    law of the candidate; written into ``out`` when given (a caller in a loop reuses its own)."""
    if env.dim() != 2 or env.dtype != torch.float32 or not env.is_contiguous():
        raise ValueError(f"envelope_score: env must be a contiguous float32 [N, F] tensor, got {env.dtype} "
                         f"{tuple(env.shape)}")
    N, F = env.shape
    if cand.dim() != 3 or cand.dtype != torch.float32 or not cand.is_contiguous() or cand.shape[0] != N \
            or cand.shape[2] != len(COLUMNS):
        raise ValueError(f"envelope_score: cand must be a contiguous float32 [{N}, M, 6] tensor, got {cand.dtype} "
                         f"{tuple(cand.shape)}")
    M = cand.shape[1]
    if N < 1 or M < 1 or F < 1:
        raise ValueError(f"envelope_score: need N, M, F >= 1, got N = {N}, M = {M}, F = {F}")
    t0, dt = float(t0), float(dt)
    if not (abs(t0) < float("inf") and 0.0 < dt < float("inf")):
        raise ValueError(f"envelope_score: t0 must be finite and dt finite and > 0, got t0 = {t0}, dt = {dt}")
    if 4 * F > LDS_BUDGET_BYTES:
        raise ValueError(f"envelope_score: a row of {F} frames needs {4 * F} bytes of LDS, the kernel's budget is "
                         f"{LDS_BUDGET_BYTES}")
    if N > 65535:
        raise ValueError(f"envelope_score: at most 65535 sounds per call, got {N}")
    if out is None:
        out = torch.empty((N, M), dtype=torch.float32, device=env.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (N, M) or not out.is_contiguous():
        raise ValueError(f"envelope_score: out must be a contiguous float32 [{N}, {M}] tensor, got {out.dtype} "
                         f"{tuple(out.shape)}")
    st = _lib.load().ias_envelope_score(_lib.ptr(env), _lib.ptr(cand), N, M, F, t0, dt, _lib.ptr(out), _lib.stream())
    _lib.check(st, "ias_envelope_score")
    return out


# The five primitives of ``fit_envelope`` on the device.  The tests pass the same five restated in fp64 numpy on CPU
# tensors (tests/envelope_model.py), so the search is one code path for both; its loop takes the last three from here.
DEVICE_OPS = SimpleNamespace(frames=envelope_frames, sample=evolve_sample, score=envelope_score, merge=topk_merge,
                             update=evolve_update)


@torch.no_grad()
def fit_envelope(audio, sample_rate, W=1024, hop=256, generations=16, population=512, elites=16, sigma0=0.3, alpha=0.7,
                 sigma_min=0.005, sigma_max=0.5, seed=0, init01=None, ops=DEVICE_OPS):
    """audio [N, T] -> ``EnvelopeFit``: the envelope law nearest to each sound's RMS envelope.

    The envelope is ``ops.frames(audio, W, hop)``, frame f at the centre of its window: t0 = (W / 2) / sample_rate,
    dt = hop / sample_rate.  The search is ``evolve.cross_entropy_search`` (which also checks the settings) with P = 6,
    every column free, no ``history`` and ``ops.score`` as the scorer.  The start, 0.5 everywhere or ``init01`` [N, 6], is
    candidate 0 of generation 0, so the result is never worse than the start (``dist <= start_dist``).

    Per generation: one ``ops.score``, and the loop's copy of the elite indices, ``ops.merge``, ``ops.update`` and
    ``ops.sample`` for the next generation, for all sounds at once.  The host reads nothing back, every buffer is reused,
    and the same seed gives the same bits.  A silent sound scores 1 everywhere and comes back with ``sounding`` False.
    ``ops``: the primitives; the default runs the HIP kernels on device tensors."""
    if audio.dim() != 2:
        raise ValueError(f"fit_envelope: audio must be [N, T], got {tuple(audio.shape)}")
    if not float(sample_rate) > 0.0:
        raise ValueError(f"fit_envelope: sample_rate must be > 0, got {sample_rate}")
    audio = audio.detach().to(torch.float32).contiguous()
    N, dev, P = audio.shape[0], audio.device, len(COLUMNS)
    if init01 is None:
        start = torch.full((N, P), 0.5, dtype=torch.float32, device=dev)
    else:
        if tuple(init01.shape) != (N, P):
            raise ValueError(f"fit_envelope: init01 must be [{N}, {P}], got {tuple(init01.shape)}")
        start = init01.detach().to(device=dev, dtype=torch.float32).clamp(0.0, 1.0)

    rms = ops.frames(audio, W, hop)                      # first, so that it runs while the host sets the search up
    t0, dt = (int(W) / 2.0) / float(sample_rate), int(hop) / float(sample_rate)
    start_dist = torch.empty(N, dtype=torch.float32, device=dev)

    def score(g, pop, out):
        ops.score(rms, pop, t0, dt, out=out)
        if g == 0:
            start_dist.copy_(out[:, 0])
    found = cross_entropy_search(start.unsqueeze(1), torch.ones(P, dtype=torch.uint8, device=dev), score, generations,
                                 population, elites, sigma0, alpha, sigma_min, sigma_max, seed, keep_history=False, ops=ops,
                                 what="fit_envelope")
    best = found.params01[:, 0].contiguous()
    return EnvelopeFit(params01=best, dist=found.dist[:, 0].contiguous(), start_dist=start_dist,
                       sounding=rms.max(dim=1).values > 0.0, units=to_units(best), rms=rms)


def reshape(params01, fit):
    """Give every start of every sounding sound the fitted envelope -> a new tensor.

    ``params01``: [N, 78] or [N, S, 78] in 0..1; ``fit``: the ``EnvelopeFit`` of the N sounds.  Per start of a sounding
    sound, ``keyboard.duration`` and the five columns of both ``adsr_1`` and ``adsr_2`` take the fit's 0..1 values: both,
    because both feed the amplitude routes of the mod matrix.  No other column changes, and the rows of silent sounds come
    back with the same bits.  With the routes below at zero the voice's amplitude then follows the fitted law.

    NOT compensated: the LFO -> amplitude routes (``lfo_k->vco_k_amp``, ``lfo_k->noise_amp``), which add their own shape
    to the amplitude; the weights of the mod matrix, which scale the two ADSRs per oscillator; and the mixer, whose levels
    weigh the oscillators and the noise.  The fit is left to sort those out."""
    if params01.dim() not in (2, 3) or params01.shape[-1] != S.NPARAMS:
        raise ValueError(f"reshape: params01 must be [N, {S.NPARAMS}] or [N, S, {S.NPARAMS}], got {tuple(params01.shape)}")
    N = params01.shape[0]
    if tuple(fit.params01.shape) != (N, len(COLUMNS)) or tuple(fit.sounding.shape) != (N,):
        raise ValueError(f"reshape: the fit is of {tuple(fit.params01.shape)} sounds x columns, params01 of {N} sounds")
    p = params01
    new = fit.params01.to(device=p.device, dtype=p.dtype)
    sounding = fit.sounding.to(device=p.device)
    if p.dim() == 3:
        new, sounding = new.unsqueeze(1), sounding.unsqueeze(1)
    out = p.clone()
    out[..., _DURATION] = torch.where(sounding, new[..., 0], p[..., _DURATION])
    for adsr in _ADSR:
        for j, col in enumerate(adsr, start=1):
            out[..., col] = torch.where(sounding, new[..., j], p[..., col])
    return out

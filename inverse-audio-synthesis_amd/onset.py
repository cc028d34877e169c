"""Onset detection and note segmentation of the targets of sound matching: a long recording becomes one synth buffer
per note, and the matched notes go back to their onsets.

Every other stage of sound matching takes a target to be one note that starts at sample 0 of one synth buffer.
``detect_onsets`` finds the note onsets on the device: the mel power spectrogram (one ``MelSpectrogram`` launch), its
log-compressed positive spectral flux (``onset_flux``: ias_onset_flux) and a peak picker with a moving maximum, a moving
mean plus ``delta`` and a minimum distance (``onset_pick``: ias_onset_pick), the scheme of Boeck, Krebs & Schedl,
"Evaluating the online capabilities of onset detection methods" (ISMIR 2012).  ``split_notes`` cuts the recording into
one buffer per note (ias_segment_gather), ``join_notes`` puts note buffers back at their onsets (ias_segment_scatter);
csrc/onset_kernels.hip, DESIGN.md section 4.10, ``match_audio.py --split``.

The window defaults of ``detect_onsets`` were chosen on synthetic decaying notes with the fp64 model of the tests
(tests/onset_model.py) only; no measurement on real recordings exists.
"""
from dataclasses import dataclass

import torch

from . import _lib


@dataclass
class OnsetResult:
    frames: torch.Tensor            # [N, K] int32: the accepted flux frames in ascending order, -1 in unused slots
    samples: torch.Tensor           # [N, K] int64: max(frame - lag, 0) * hop, the sample a note is cut at; -1 when unused
    strength: torch.Tensor          # [N, K] fp32: the flux at the accepted frames, 0 in unused slots
    count: torch.Tensor             # [N] int32: the number accepted, which may exceed K
    flux: torch.Tensor              # [N, F] fp32


@dataclass
class NoteSegments:
    audio: torch.Tensor             # [S, T] fp32: one synth buffer per note, from its start, faded out where it was cut
    row: torch.Tensor               # [S] int32: the recording a note comes from
    start: torch.Tensor             # [S] int32: its first sample there
    length: torch.Tensor            # [S] int32: its samples, <= T
    faded: torch.Tensor             # [S] uint8: 1 when the note was cut by the next onset or by T, 0 when the file ends
    strength: torch.Tensor          # [S] fp32: the flux at the note's onset; 0 without an ``OnsetResult`` or an onset
    fade: int                       # samples of the linear fade-out of a cut note


def _check_f32(name, t, dim):
    if t.dim() != dim or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous float32 tensor of {dim} dimensions, got {t.dtype} {tuple(t.shape)}")


def onset_flux(mel, lag=2, gamma=100.0, return_logmel=False):
    """One launch of ias_onset_flux (include/ias_hip.h) on mel [B, F, M] (device fp32, contiguous, frames-major power
    values as ``STFTPlan.values`` produces them) -> flux [B, F] fp32, with ``return_logmel`` also log1p(gamma mel)
    [B, F, M]: the mean over the mels of the positive part of the log-mel difference to the frame ``lag`` frames earlier."""
    _check_f32("onset_flux: mel", mel, 3)
    B, F, M = mel.shape
    lag, gamma = int(lag), float(gamma)
    if B < 1 or F < 1 or M < 1 or lag < 1:
        raise ValueError(f"onset_flux: need B, F, M, lag >= 1, got B = {B}, F = {F}, M = {M}, lag = {lag}")
    if not 0.0 < gamma < float("inf"):
        raise ValueError(f"onset_flux: gamma must be finite and > 0, got {gamma}")
    flux = torch.empty((B, F), dtype=torch.float32, device=mel.device)
    logmel = torch.empty_like(mel) if return_logmel else None
    st = _lib.load().ias_onset_flux(_lib.ptr(mel), B, F, M, lag, gamma, _lib.ptr(flux), _lib.ptr(logmel), _lib.stream())
    _lib.check(st, "ias_onset_flux")
    return (flux, logmel) if return_logmel else flux


def onset_pick(flux, pre_max=3, post_max=3, pre_avg=10, post_avg=10, delta=0.2, wait=4, max_onsets=256):
    """One launch of ias_onset_pick (include/ias_hip.h) on flux [B, F] (device fp32, contiguous) -> (frames [B, K] int32,
    strength [B, K] fp32, count [B] int32), K = ``max_onsets``: the frames that are the maximum of [f - pre_max,
    f + post_max], at least ``delta`` above the mean of [f - pre_avg, f + post_avg] and more than ``wait`` frames after
    the onset before them."""
    _check_f32("onset_pick: flux", flux, 2)
    B, F = flux.shape
    pre_max, post_max, pre_avg, post_avg = int(pre_max), int(post_max), int(pre_avg), int(post_avg)
    wait, K, delta = int(wait), int(max_onsets), float(delta)
    if B < 1 or F < 1 or K < 1:
        raise ValueError(f"onset_pick: need B, F, max_onsets >= 1, got B = {B}, F = {F}, max_onsets = {K}")
    if min(pre_max, post_max, pre_avg, post_avg, wait) < 0:
        raise ValueError(f"onset_pick: the window sizes and wait must be >= 0, got pre_max = {pre_max}, post_max = "
                         f"{post_max}, pre_avg = {pre_avg}, post_avg = {post_avg}, wait = {wait}")
    if not delta > 0.0:
        raise ValueError(f"onset_pick: delta must be > 0 (silence would be one long plateau of candidates), got {delta}")
    if B > 65535:
        raise ValueError(f"onset_pick: at most 65535 rows per call, got {B}")
    dev = flux.device
    frames = torch.empty((B, K), dtype=torch.int32, device=dev)
    strength = torch.empty((B, K), dtype=torch.float32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    st = _lib.load().ias_onset_pick(_lib.ptr(flux), B, F, pre_max, post_max, pre_avg, post_avg, delta, wait, K,
                                    _lib.ptr(frames), _lib.ptr(strength), _lib.ptr(count), _lib.stream())
    _lib.check(st, "ias_onset_pick")
    return frames, strength, count


_PLANS = {}


def _mel_plan(sample_rate, n_fft, hop, n_mels, device):
    """The ``MelSpectrogram`` of one (sample_rate, n_fft, hop, n_mels) combination on ``device``, built once."""
    from .spectral import MelSpectrogram
    key = (int(sample_rate), int(n_fft), int(hop), int(n_mels), str(device))
    plan = _PLANS.get(key)
    if plan is None:
        plan = _PLANS[key] = MelSpectrogram(sample_rate=int(sample_rate), n_fft=int(n_fft), hop_length=int(hop),
                                            n_mels=int(n_mels)).to(device)
    return plan


@torch.no_grad()
def detect_onsets(audio, sample_rate, n_fft=1024, hop=256, n_mels=128, lag=2, gamma=100.0, pre_max=3, post_max=3,
                  pre_avg=10, post_avg=10, delta=0.2, wait=4, max_onsets=256):
    """audio [N, L] on the device -> ``OnsetResult``: the mel power spectrogram (centred frames, frame f around sample
    f hop), ``onset_flux`` and ``onset_pick``; three launches, and the host reads nothing back.  ``samples`` is
    max(frame - lag, 0) * hop: the flux peaks while the attack enters the analysis window, so a note is cut slightly
    early and its attack is never clipped.  The file counts as preceded by silence: a note sounding at sample 0 is an
    onset at frame 0.  The defaults were chosen on synthetic notes with the tests' fp64 model only (no measurement on
    real recordings exists).  A recording the STFT entry refuses (its length against ``n_fft``, B F past its grid)
    raises the library's error; chunking a longer recording is left to the caller."""
    if audio.dim() != 2:
        raise ValueError(f"detect_onsets: audio must be [N, L], got {tuple(audio.shape)}")
    if int(hop) < 1 or int(n_mels) < 1:
        raise ValueError(f"detect_onsets: need hop, n_mels >= 1, got hop = {hop}, n_mels = {n_mels}")
    audio = audio.detach().to(torch.float32).contiguous()
    mel = _mel_plan(sample_rate, n_fft, hop, n_mels, audio.device).frames_major(audio)
    flux = onset_flux(mel, lag=lag, gamma=gamma)
    frames, strength, count = onset_pick(flux, pre_max=pre_max, post_max=post_max, pre_avg=pre_avg, post_avg=post_avg,
                                         delta=delta, wait=wait, max_onsets=max_onsets)
    return OnsetResult(frames=frames, samples=onset_samples(frames, lag, hop), strength=strength, count=count, flux=flux)


def onset_samples(frames, lag, hop):
    """frames [N, K] (-1: unused) -> int64 max(frame - lag, 0) * hop, -1 where unused."""
    f = frames.to(torch.int64)
    return torch.where(f >= 0, (f - int(lag)).clamp_min(0) * int(hop), torch.full_like(f, -1))


def segment_candidates(lengths, samples, T):
    """The descriptor logic of ``split_notes`` up to the compaction, plain torch on the inputs' device (CPU tensors too),
    no host read.  lengths [N] and samples [N, K] (ascending per row, negative: unused) -> (keep [N, K + 1] bool, start,
    length [N, K + 1] int64, faded [N, K + 1] bool).  Column 0 is the segment from sample 0 of a row without an onset,
    column 1 + k is onset k.  An onset at or beyond the row's length is dropped, and so is one at the sample of the onset
    before it.  A note ends at the earliest of the next kept onset, start + T and the row's length; ``faded`` says that it
    was cut by one of the first two."""
    if lengths.dim() != 1 or samples.dim() != 2 or samples.shape[0] != lengths.shape[0]:
        raise ValueError(f"split_notes: lengths must be [N] and the onsets [N, K], got {tuple(lengths.shape)} and "
                         f"{tuple(samples.shape)}")
    if int(T) < 1:
        raise ValueError(f"split_notes: T must be >= 1, got {T}")
    lengths = lengths.to(torch.int64)
    samples = samples.to(device=lengths.device, dtype=torch.int64)
    N, K = samples.shape
    valid = (samples >= 0) & (samples < lengths[:, None])
    if K > 1:
        valid[:, 1:] &= samples[:, 1:] != samples[:, :-1]
    zero = torch.zeros((N, 1), dtype=torch.int64, device=lengths.device)
    start = torch.cat([zero, samples], dim=1)
    keep = torch.cat([~valid.any(dim=1, keepdim=True), valid], dim=1)
    # the next kept start of the row: a reversed running minimum over the kept starts behind a column
    big = torch.iinfo(torch.int64).max
    later = torch.where(keep, start, torch.full_like(start, big))
    later = torch.cat([later[:, 1:], torch.full((N, 1), big, dtype=torch.int64, device=lengths.device)], dim=1)
    nxt = torch.flip(torch.cummin(torch.flip(later, dims=[1]), dim=1).values, dims=[1])
    end = torch.minimum(torch.minimum(nxt, start + int(T)), lengths[:, None])
    length = (end - start).clamp_min(0)
    faded = end < lengths[:, None]
    return keep, start, length, faded


def _fade_args(fade):
    fade = int(fade)
    if fade < 0:
        raise ValueError(f"split_notes: fade must be >= 0 samples, got {fade}")
    return fade, (1.0 / fade if fade > 0 else 0.0)


@torch.no_grad()
def split_notes(audio, lengths, onsets, T, fade):
    """audio [N, L] (device fp32), lengths [N] (the rows' true lengths in samples; the rest is padding), onsets (an
    ``OnsetResult`` or its ``samples`` [N, K]) -> ``NoteSegments`` with audio [S, T]: note k of row i runs from its start
    to the earliest of the next note's start, start + T and the row's length; a note that was cut by the next onset or by
    T fades out linearly over its last ``fade`` samples, one that ends with the file does not.  A row without an onset
    gives one segment from sample 0 (what cropping the file to the buffer gives); onsets at or beyond the row's length
    are dropped.  The descriptors are built by torch operations on the device (``segment_candidates``).  Reading their
    number S (``torch.nonzero``) is ONE host synchronisation, the only one of the stage: the note buffers cannot be
    allocated without it.  Then one ias_segment_gather launch."""
    _check_f32("split_notes: audio", audio, 2)
    N, L = audio.shape
    fade, inv_fade = _fade_args(fade)
    samples = onsets.samples if isinstance(onsets, OnsetResult) else onsets
    lengths = lengths.to(audio.device)
    if lengths.shape != (N,) or N < 1 or L < 1:
        raise ValueError(f"split_notes: audio is {tuple(audio.shape)}, lengths {tuple(lengths.shape)}")
    keep, start, length, faded = segment_candidates(lengths.clamp(0, L), samples, T)
    at = torch.nonzero(keep.reshape(-1)).reshape(-1)                    # the host synchronisation: S = at.numel()
    width = keep.shape[1]
    row = torch.div(at, width, rounding_mode="floor").to(torch.int32)
    start = start.reshape(-1)[at].to(torch.int32)
    length = length.reshape(-1)[at].to(torch.int32)
    faded = faded.reshape(-1)[at].to(torch.uint8)
    strength = torch.zeros(keep.shape, dtype=torch.float32, device=audio.device)
    if isinstance(onsets, OnsetResult):
        strength[:, 1:] = onsets.strength
    strength = strength.reshape(-1)[at]
    S = int(at.numel())
    out = torch.empty((S, int(T)), dtype=torch.float32, device=audio.device)
    st = _lib.load().ias_segment_gather(_lib.ptr(audio), N, L, _lib.ptr(row), _lib.ptr(start), _lib.ptr(length),
                                        _lib.ptr(faded), S, int(T), fade, inv_fade, _lib.ptr(out), _lib.stream())
    _lib.check(st, "ias_segment_gather")
    return NoteSegments(audio=out, row=row, start=start, length=length, faded=faded, strength=strength, fade=fade)


@torch.no_grad()
def join_notes(note_audio, segments, N, L, gain=None):
    """note_audio [S, T] (device fp32), the ``NoteSegments`` they were cut by -> [N, L]: zeros, then every note's first
    ``length`` samples times ``gain`` [S] (default 1) at its start, with the fade-out ``split_notes`` gave it (one
    ias_segment_scatter launch; the segments of ``split_notes`` never overlap, so no sample is written twice)."""
    _check_f32("join_notes: note_audio", note_audio, 2)
    S, T = note_audio.shape
    if tuple(segments.row.shape) != (S,) or int(N) < 1 or int(L) < 1 or S < 1:
        raise ValueError(f"join_notes: {S} note buffers, {tuple(segments.row.shape)} segments, N = {N}, L = {L}")
    fade, inv_fade = _fade_args(segments.fade)
    dev = note_audio.device
    if gain is None:
        gain = torch.ones((S,), dtype=torch.float32, device=dev)
    gain = gain.to(device=dev, dtype=torch.float32).contiguous()
    if tuple(gain.shape) != (S,):
        raise ValueError(f"join_notes: gain must be [{S}], got {tuple(gain.shape)}")
    out = torch.zeros((int(N), int(L)), dtype=torch.float32, device=dev)
    st = _lib.load().ias_segment_scatter(_lib.ptr(note_audio), int(N), int(L), _lib.ptr(segments.row),
                                         _lib.ptr(segments.start), _lib.ptr(segments.length), _lib.ptr(segments.faded), S, T,
                                         fade, inv_fade, _lib.ptr(gain), _lib.ptr(out), _lib.stream())
    _lib.check(st, "ias_segment_scatter")
    return out


def note_gains(target, render, length):
    """[S, T] note targets and renders, length [S] -> [S] fp32: RMS of the target over RMS of the render, both over the
    note's first ``length`` samples; 1 where the render is silent there.  Plain torch, no host read."""
    T = target.shape[1]
    inside = torch.arange(T, device=target.device)[None, :] < length.to(target.device)[:, None]
    zero = torch.zeros((), dtype=torch.float64, device=target.device)
    et = torch.where(inside, target.double() ** 2, zero).sum(dim=1)
    er = torch.where(inside, render.double() ** 2, zero).sum(dim=1)
    return torch.where(er > 0, torch.sqrt(et / er.clamp_min(1e-300)), torch.ones_like(er)).float()

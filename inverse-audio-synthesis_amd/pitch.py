"""Pitch estimation of the targets of sound matching: YIN on the device, aggregated to one note per sound.

An L1 spectral loss has almost no gradient along ``keyboard.midi_f0`` (partials that do not overlap give a flat loss), so a
fit has to *start* within a partial's width of the target's note.  The fundamental can be read off
the waveform: ``pitch_yin`` (ias_pitch_yin, csrc/pitch_kernels.hip) runs de Cheveigne & Kawahara's YIN per frame,
``aggregate_pitch`` turns the frames of a sound into one MIDI note, a voiced flag and a confidence, and ``retune`` moves the
keyboard of a start onto that note (``match_audio.py --pitch``).  One note per sound is assumed; a
recording of several notes is cut into one sound per note first (``onset.detect_onsets`` / ``split_notes``,
``match_audio.py --split``).
"""
import math
from dataclasses import dataclass

import torch

from . import _lib
from . import voice_spec as S

LDS_BUDGET_BYTES = 65536            # the kernel's LDS budget (include/ias_hip.h: ias_pitch_yin)


@dataclass
class PitchEstimate:
    midi: torch.Tensor              # [N] fp32: the sound's note, NaN when unvoiced
    voiced: torch.Tensor            # [N] bool
    confidence: torch.Tensor        # [N] fp32: 1 - median aperiodicity of the voiced frames, 0 when unvoiced
    frame_midi: torch.Tensor        # [N, F] fp32: every frame's note, voiced or not
    frame_voiced: torch.Tensor      # [N, F] bool


def lds_bytes(W, tau_max):
    """LDS a frame needs in ias_pitch_yin: the fp64 running sum, the frame with its zero padding, and d."""
    return 8 * (tau_max + 1) + 4 * (W + tau_max + 8) + 4 * (tau_max + 1)


def num_frames(T, W, tau_max, hop):
    """ias_pitch_frames: (T - W - tau_max) // hop + 1, ValueError when not even one frame fits."""
    F = _lib.load().ias_pitch_frames(int(T), int(W), int(tau_max), int(hop))
    if F < 1:
        raise ValueError(f"pitch: no frame fits: T = {T}, W = {W}, tau_max = {tau_max}, hop = {hop} (need sizes >= 1 and "
                         f"T >= W + tau_max)")
    return F


def pitch_yin(audio, W, tau_min, tau_max, hop, threshold=0.15, return_dprime=False):
    """One launch of ias_pitch_yin (include/ias_hip.h) on audio [B, T] (device fp32, contiguous) -> (period, aperiodicity,
    energy), each [B, F] fp32 with F = (T - W - tau_max) // hop + 1, and with ``return_dprime`` also d' [B, F, tau_max + 1].
    Frame f uses audio[:, f hop : f hop + W + tau_max]; lags tau_min .. tau_max are searched."""
    if audio.dim() != 2 or audio.dtype != torch.float32 or not audio.is_contiguous():
        raise ValueError(f"pitch_yin: audio must be a contiguous float32 [B, T] tensor, got {audio.dtype} "
                         f"{tuple(audio.shape)}")
    B, T = audio.shape
    W, tau_min, tau_max, hop = int(W), int(tau_min), int(tau_max), int(hop)
    if B < 1 or W < 1 or hop < 1 or tau_min < 2 or tau_min > tau_max:
        raise ValueError(f"pitch_yin: need B, W, hop >= 1 and 2 <= tau_min <= tau_max, got B = {B}, W = {W}, hop = {hop}, "
                         f"tau_min = {tau_min}, tau_max = {tau_max}")
    if not 0.0 < float(threshold) <= 1.0:
        raise ValueError(f"pitch_yin: threshold must be in (0, 1], got {threshold}")
    F = num_frames(T, W, tau_max, hop)
    if lds_bytes(W, tau_max) > LDS_BUDGET_BYTES:
        raise ValueError(f"pitch_yin: a frame of W = {W}, tau_max = {tau_max} needs {lds_bytes(W, tau_max)} bytes of LDS, "
                         f"the kernel's budget is {LDS_BUDGET_BYTES}")
    if B > 65535:
        raise ValueError(f"pitch_yin: at most 65535 rows per call, got {B}")
    dev = audio.device
    period = torch.empty((B, F), dtype=torch.float32, device=dev)
    aper = torch.empty_like(period)
    energy = torch.empty_like(period)
    dprime = torch.empty((B, F, tau_max + 1), dtype=torch.float32, device=dev) if return_dprime else None
    st = _lib.load().ias_pitch_yin(_lib.ptr(audio), B, T, W, tau_min, tau_max, hop, float(threshold), _lib.ptr(period),
                                   _lib.ptr(aper), _lib.ptr(energy), _lib.ptr(dprime), _lib.stream())
    _lib.check(st, "ias_pitch_yin")
    return (period, aper, energy, dprime) if return_dprime else (period, aper, energy)


def _lower_median(values, mask, count):
    """Per row: the lower median of values[mask] (the element of rank (count - 1) // 2); rows with count == 0 give +inf."""
    inf = torch.full_like(values, float("inf"))
    ordered, _i = torch.sort(torch.where(mask, values, inf), dim=1)
    at = ((count - 1).clamp_min(0) // 2).unsqueeze(1)
    return torch.gather(ordered, 1, at).squeeze(1)


def aggregate_pitch(period, aperiodicity, energy, sample_rate, threshold=0.15, gate_db=-30.0, min_voiced=3):
    """Frames -> one note per sound; plain torch on the inputs' device (CPU tensors too), no host read.

    period, aperiodicity, energy: [N, F] as ``pitch_yin`` returns them.  A frame is voiced when its aperiodicity is below
    ``threshold`` and its energy is within ``gate_db`` (negative, a power ratio in dB) of the row's loudest frame, which
    must itself be > 0.  A sound is voiced when it has at least ``min_voiced`` voiced frames.  ``midi`` is the lower median
    of 69 + 12 log2(sample_rate / period / 440) over the sound's voiced frames (the element of rank (n - 1) // 2 of n), NaN
    when the sound is unvoiced; ``confidence`` is 1 - the lower median of the aperiodicity over the same frames, 0 when
    unvoiced."""
    if period.dim() != 2 or period.shape != aperiodicity.shape or period.shape != energy.shape:
        raise ValueError(f"aggregate_pitch: period, aperiodicity and energy must share one [N, F] shape, got "
                         f"{tuple(period.shape)}, {tuple(aperiodicity.shape)}, {tuple(energy.shape)}")
    if int(min_voiced) < 1:
        raise ValueError(f"aggregate_pitch: min_voiced must be >= 1, got {min_voiced}")
    period, aperiodicity, energy = period.float(), aperiodicity.float(), energy.float()
    loudest = energy.max(dim=1, keepdim=True).values
    gate = loudest * (10.0 ** (float(gate_db) / 10.0))
    frame_voiced = (aperiodicity < float(threshold)) & (loudest > 0.0) & (energy >= gate)
    frame_midi = 69.0 + 12.0 * torch.log2(float(sample_rate) / period / 440.0)
    count = frame_voiced.sum(dim=1)
    voiced = count >= int(min_voiced)
    midi = _lower_median(frame_midi, frame_voiced, count)
    aper = _lower_median(aperiodicity, frame_voiced, count)
    nan = torch.full_like(midi, float("nan"))
    return PitchEstimate(midi=torch.where(voiced, midi, nan), voiced=voiced,
                         confidence=torch.where(voiced, 1.0 - aper, torch.zeros_like(aper)), frame_midi=frame_midi,
                         frame_voiced=frame_voiced)


def midi_to_hz(midi):
    return 440.0 * 2.0 ** ((float(midi) - 69.0) / 12.0)


def yin_plan(sample_rate, midi_lo=21.0, midi_hi=108.0):
    """-> (W, tau_min, tau_max) of ``estimate_pitch``: tau_max = ceil(rate / hz(midi_lo)), W = tau_max, tau_min = max(2,
    floor(rate / hz(midi_hi)))."""
    if not float(midi_lo) < float(midi_hi):
        raise ValueError(f"pitch: need midi_lo < midi_hi, got {midi_lo} and {midi_hi}")
    tau_max = int(math.ceil(float(sample_rate) / midi_to_hz(midi_lo)))
    tau_min = max(2, int(math.floor(float(sample_rate) / midi_to_hz(midi_hi))))
    if tau_min > tau_max:
        raise ValueError(f"pitch: the range MIDI {midi_lo}..{midi_hi} holds no lag >= 2 at {sample_rate} Hz")
    return tau_max, tau_min, tau_max


@torch.no_grad()
def estimate_pitch(audio, sample_rate, midi_lo=21.0, midi_hi=108.0, hop=512, threshold=0.15, gate_db=-30.0, min_voiced=3):
    """audio [N, T] on the device -> ``PitchEstimate``: ``pitch_yin`` over the lags of MIDI ``midi_lo`` .. ``midi_hi`` with
    a window of the longest period, then ``aggregate_pitch``.  One kernel launch and a handful of torch operations; the
    host reads nothing back."""
    W, tau_min, tau_max = yin_plan(sample_rate, midi_lo, midi_hi)
    audio = audio.detach().to(torch.float32).contiguous()
    period, aper, energy = pitch_yin(audio, W, tau_min, tau_max, hop, threshold=threshold)
    return aggregate_pitch(period, aper, energy, sample_rate, threshold=threshold, gate_db=gate_db, min_voiced=min_voiced)


_F0 = S.INDEX[("keyboard", "midi_f0")]
_TUNING = (S.INDEX[("vco_1", "tuning")], S.INDEX[("vco_2", "tuning")])
_LEVEL = (S.INDEX[("mixer", "vco_1")], S.INDEX[("mixer", "vco_2")])
_TUNING_LO, _TUNING_HI = S.PARAMS[_TUNING[0]][2], S.PARAMS[_TUNING[0]][3]
_F0_HI = S.PARAMS[_F0][3]


def retune(params01, estimate):
    """Move the keyboard of every start of every voiced sound onto the estimated note -> a new tensor.

    ``params01``: [N, 78] or [N, S, 78] in 0..1; ``estimate``: a ``PitchEstimate`` of the N sounds.  Per start: k is the
    oscillator with the larger ``mixer.vco_k`` level (a tie: vco_1), tuning its ``vco_k.tuning`` in semitones (linear,
    -24..24), and ``keyboard.midi_f0`` becomes clamp(midi - tuning, 0, 127) / 127.  No other column changes, and the rows
    of unvoiced sounds come back with the same bits.  From the centre start (tuning 0, symmetric depths 0) the voice then
    sounds at exactly ``midi``.

    NOT compensated: the pitch modulation.  The ``mod_matrix`` routes into ``vco_k_pitch`` and the oscillators'
    ``mod_depth`` shift and bend the sounding pitch of a start that has them away from ``midi``, and the quieter
    oscillator keeps its own tuning; the fit is left to sort that out."""
    if params01.dim() not in (2, 3) or params01.shape[-1] != S.NPARAMS:
        raise ValueError(f"retune: params01 must be [N, {S.NPARAMS}] or [N, S, {S.NPARAMS}], got {tuple(params01.shape)}")
    N = params01.shape[0]
    if tuple(estimate.midi.shape) != (N,) or tuple(estimate.voiced.shape) != (N,):
        raise ValueError(f"retune: the estimate is of {tuple(estimate.midi.shape)} sounds, params01 of {N}")
    p = params01
    midi = estimate.midi.to(device=p.device, dtype=p.dtype)
    voiced = estimate.voiced.to(device=p.device)
    if p.dim() == 3:
        midi, voiced = midi.unsqueeze(1), voiced.unsqueeze(1)
    second = p[..., _LEVEL[1]] > p[..., _LEVEL[0]]
    tuning01 = torch.where(second, p[..., _TUNING[1]], p[..., _TUNING[0]])
    tuning = _TUNING_LO + (_TUNING_HI - _TUNING_LO) * tuning01
    f0 = (midi - tuning).clamp(0.0, _F0_HI) / _F0_HI
    out = p.clone()
    out[..., _F0] = torch.where(voiced, f0, p[..., _F0])
    return out

"""Match report: how near a render is to its target, in figures that do not depend on the loss that was fitted.

Every quality figure of sound matching used to be the matcher's own loss, so runs under different ``--loss`` choices shared
no scale and a stage that moves the note (``--pitch``) could not show it.  ``spectral_report`` (ias_spectral_report,
csrc/report_kernels.hip, include/ias_hip_report.h) compares two frames-major spectrogram tensors per sound: log-spectral
distance, spectral convergence, the mean absolute log difference and a mel-cepstral distance, over the frames that sound.
``Reporter`` runs it on a linear-magnitude STFT and on the mel spectrogram of the config, and adds a pitch error
(``pitch.estimate_pitch`` on both sides) and an envelope error (``envelope.envelope_frames``).  Forward only: no figure here
is a loss (``match_audio.py --report``).
"""
import ctypes
import math
from dataclasses import dataclass, fields

import torch

from . import _lib
from .envelope import envelope_frames
from .pitch import estimate_pitch
from .spectral import VALUE_MAG, MelSpectrogram, STFTPlan

MAX_BINS, MAX_COEF, MAX_DCT_BINS = 2048, 32, 256        # ias_spectral_report's limits (include/ias_hip_report.h)
COLUMNS = ("lsd_db", "spectral_convergence", "log_l1_db", "mcd_db", "frames")
CHUNK_ROWS = 128                                        # rows per pass of ``Reporter``
ENVELOPE_W, ENVELOPE_HOP = 1024, 256
FLOOR_MIN = 1e-30                                       # keeps every floor a normal fp32 number


def dct_table(n_in, n_coef):
    """ias_report_build_dct: the host fp32 table [n_coef, n_in], row c - 1 = sqrt(2 / n_in) cos(pi c (2 k + 1) / (2 n_in)),
    the orthonormal DCT-II without its row 0, computed in fp64 and rounded once."""
    n_in, n_coef = int(n_in), int(n_coef)
    if n_in < 1 or n_coef < 1 or n_coef >= n_in:
        raise ValueError(f"dct_table: need 1 <= n_coef < n_in, got n_in = {n_in}, n_coef = {n_coef}")
    out = torch.empty((n_coef, n_in), dtype=torch.float32)
    _lib.check(_lib.load().ias_report_build_dct(n_in, n_coef, ctypes.c_void_p(out.data_ptr())), "ias_report_build_dct")
    return out


def spectral_report(values, target_values, floor_rows, power, dct=None):
    """One call of ias_spectral_report (include/ias_hip_report.h): values and target_values [B, F, K] (device fp32,
    contiguous, frames-major: ``STFTPlan.values`` / ``MelSpectrogram.frames_major``), floor_rows [B] fp32, ``power`` 1
    (magnitudes) or 2 (powers), ``dct`` None or a device copy of ``dct_table(K, C)`` -> [B, 5] fp64 on the device, columns
    ``COLUMNS``; column 3 is 0 without ``dct``.  A row's five numbers do not depend on the other rows or on its place in the
    batch (same bits).  The floors are raised to ``FLOOR_MIN`` on the device, so every entry the kernel sees is > 0."""
    for name, t in (("values", values), ("target_values", target_values)):
        if t.dim() != 3 or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"spectral_report: {name} must be a contiguous float32 [B, F, K] tensor, got {t.dtype} "
                             f"{tuple(t.shape)}")
    if values.shape != target_values.shape:
        raise ValueError(f"spectral_report: values {tuple(values.shape)} and target_values {tuple(target_values.shape)} "
                         f"differ in shape")
    B, F, K = values.shape
    if floor_rows.dtype != torch.float32 or tuple(floor_rows.shape) != (B,) or not floor_rows.is_contiguous():
        raise ValueError(f"spectral_report: floor_rows must be a contiguous float32 [{B}] tensor, got {floor_rows.dtype} "
                         f"{tuple(floor_rows.shape)}")
    if int(power) not in (1, 2) or float(power) != int(power):
        raise ValueError(f"spectral_report: power must be 1 or 2, got {power}")
    if B < 1 or F < 1 or K < 1:
        raise ValueError(f"spectral_report: need B, F, K >= 1, got {tuple(values.shape)}")
    if B > 65535 or K > MAX_BINS:
        raise ValueError(f"spectral_report: at most 65535 rows and {MAX_BINS} bins per call, got B = {B}, K = {K}")
    C = 0
    if dct is not None:
        if dct.dim() != 2 or dct.dtype != torch.float32 or not dct.is_contiguous() or dct.shape[1] != K:
            raise ValueError(f"spectral_report: dct must be a contiguous float32 [C, {K}] tensor, got {dct.dtype} "
                             f"{tuple(dct.shape)}")
        C = dct.shape[0]
        if not 1 <= C <= MAX_COEF or C >= K or K > MAX_DCT_BINS:
            raise ValueError(f"spectral_report: with dct need 1 <= C <= {MAX_COEF}, C < K <= {MAX_DCT_BINS}, got C = {C}, "
                             f"K = {K}")
    lib = _lib.load()
    floors = floor_rows.clamp_min(FLOOR_MIN)
    nch = lib.ias_spectral_report_partials_count(F)
    _lib.check(min(nch, 0), "ias_spectral_report_partials_count")
    partials = torch.empty((B, nch, 6), dtype=torch.float64, device=values.device)
    out = torch.empty((B, 5), dtype=torch.float64, device=values.device)
    st = lib.ias_spectral_report(_lib.ptr(values), _lib.ptr(target_values), _lib.ptr(floors), _lib.ptr(dct), B, F, K, C,
                                 int(power), _lib.ptr(partials), _lib.ptr(out), _lib.stream())
    _lib.check(st, "ias_spectral_report")
    return out


def floor_rows(target_values, power, dynamic_range_db):
    """[B] fp32 on the device: clamp(rowmax(target values) 10^(-dynamic_range_db power / 20), min=FLOOR_MIN)."""
    peak = target_values.reshape(target_values.shape[0], -1).max(dim=1).values
    return (peak * 10.0 ** (-float(dynamic_range_db) * float(power) / 20.0)).clamp_min(FLOOR_MIN).contiguous()


@dataclass
class ReportTarget:
    """What ``Reporter`` keeps of the targets (``Reporter.target``): every field a device tensor over the N sounds."""
    values: torch.Tensor            # [N, F, K] fp32: linear magnitudes
    floors: torch.Tensor            # [N] fp32
    mel_values: torch.Tensor        # [N, F', n_mels] fp32
    mel_floors: torch.Tensor        # [N] fp32
    midi: torch.Tensor              # [N] fp32: the target's note, NaN when unvoiced
    voiced: torch.Tensor            # [N] bool
    rms: torch.Tensor               # [N, F''] fp32: envelope frames

    def rows(self, lo, hi):
        return ReportTarget(**{f.name: getattr(self, f.name)[lo:hi] for f in fields(self)})


@dataclass
class MatchReport:
    """[N] device tensors, one entry per sound."""
    lsd_db: torch.Tensor                # fp64: log-spectral distance of the linear magnitudes, dB
    spectral_convergence: torch.Tensor  # fp64: ||T - V|| / ||T|| of the linear magnitudes
    logmel_l1_db: torch.Tensor          # fp64: mean |log mel difference|, dB
    mcd_db: torch.Tensor                # fp64: mel-cepstral distance (coefficients 1 .. n_mfcc), dB
    frames: torch.Tensor                # int64: counted frames of the linear plan
    mel_frames: torch.Tensor            # int64: counted frames of the mel plan
    envelope_db: torch.Tensor           # fp64: mean |RMS envelope difference| over the target's sounding frames, dB
    f0_cents: torch.Tensor              # fp64: 100 (midi of the render - midi of the target), NaN where unvoiced
    voiced: torch.Tensor                # bool: both sides are voiced

    def as_records(self):
        """-> one plain dict per sound, ready for JSON: floats, ints and bools, a NaN written as None.  The one host read."""
        cols = {f.name: getattr(self, f.name).cpu().tolist() for f in fields(self)}
        recs = []
        for i in range(len(cols["lsd_db"])):
            rec = {}
            for name, col in cols.items():
                x = col[i]
                rec[name] = None if isinstance(x, float) and math.isnan(x) else x
            recs.append(rec)
        return recs


class Reporter:
    """``Reporter(sample_rate)(audio, target_audio)`` -> ``MatchReport`` of audio [N, T] against target_audio [N, T].

    Two spectral plans, each one ``spectral_report``: the linear one, ``STFTPlan(n_fft=1024, hop_length=256)`` (or
    ``stft_kwargs``) read as magnitudes (power 1), gives ``lsd_db``, ``spectral_convergence`` and ``frames``; the mel one,
    ``MelSpectrogram(sample_rate=sample_rate, **mel_kwargs)`` (its defaults are conf/config.yaml's ``mel`` block) read
    through ``frames_major`` at its own power, gives ``logmel_l1_db``, ``mcd_db`` over ``n_mfcc`` coefficients and
    ``mel_frames``.  Per plan the floor of a row is ``floor_rows``: ``dynamic_range_db`` below the target's largest value.
    ``f0_cents`` compares ``pitch.estimate_pitch`` of both sides; ``envelope_db`` is the mean, over the target's frames
    whose RMS (``envelope.envelope_frames``, W 1024, hop 256) is above its peak RMS 10^(-dynamic_range_db / 20), of
    |20 log10(max(rms_x, floor) / max(rms_y, floor))| with that threshold as the floor (0 for a silent target).

    ``target(y)`` computes what depends on the targets alone, to be passed as ``target=`` to any number of calls.  Rows go
    through in chunks of at most ``CHUNK_ROWS``; the host reads nothing back.  The tables move to the device of the first
    audio they see."""

    def __init__(self, sample_rate, stft_kwargs=None, mel_kwargs=None, n_mfcc=13, dynamic_range_db=80.0):
        if not float(sample_rate) > 0.0:
            raise ValueError(f"Reporter: sample_rate must be > 0, got {sample_rate}")
        if not 0.0 < float(dynamic_range_db) < float("inf"):
            raise ValueError(f"Reporter: dynamic_range_db must be finite and > 0, got {dynamic_range_db}")
        self.sample_rate = sample_rate
        self.dynamic_range_db = float(dynamic_range_db)
        kw = dict(n_fft=1024, hop_length=256)
        kw.update(stft_kwargs or {})
        self.plan = STFTPlan(**kw)
        kw = dict(mel_kwargs or {})
        kw.setdefault("sample_rate", sample_rate)
        self.mel = MelSpectrogram(**kw)
        self.mel_power = int(self.mel.power)
        n_mels, n_mfcc = self.mel.plan.n_out, int(n_mfcc)
        if not 1 <= n_mfcc <= MAX_COEF or n_mfcc >= n_mels or n_mels > MAX_DCT_BINS:
            raise ValueError(f"Reporter: need 1 <= n_mfcc <= {MAX_COEF} and n_mfcc < n_mels <= {MAX_DCT_BINS}, got "
                             f"n_mfcc = {n_mfcc}, n_mels = {n_mels}")
        self.dct = dct_table(n_mels, n_mfcc)
        self._device = None

    def _to(self, device):
        if self._device != device:
            self.plan, self.mel, self.dct = self.plan.to(device), self.mel.to(device), self.dct.to(device)
            self._device = device

    @staticmethod
    def _audio(x, what):
        if x.dim() != 2:
            raise ValueError(f"Reporter: {what} must be [N, T], got {tuple(x.shape)}")
        return x.detach().to(torch.float32).contiguous()

    def _target_rows(self, y):
        values = self.plan.values(y, VALUE_MAG)
        mel_values = self.mel.frames_major(y)
        est = estimate_pitch(y, self.sample_rate)
        return ReportTarget(values=values, floors=floor_rows(values, 1, self.dynamic_range_db), mel_values=mel_values,
                            mel_floors=floor_rows(mel_values, self.mel_power, self.dynamic_range_db), midi=est.midi,
                            voiced=est.voiced, rms=envelope_frames(y, ENVELOPE_W, ENVELOPE_HOP))

    @torch.no_grad()
    def target(self, y):
        """target audio [N, T] -> ``ReportTarget``: its values and floors under both plans, its note and its envelope."""
        y = self._audio(y, "target_audio")
        self._to(y.device)
        parts = [self._target_rows(y[lo:lo + CHUNK_ROWS]) for lo in range(0, y.shape[0], CHUNK_ROWS)]
        if len(parts) == 1:
            return parts[0]
        return ReportTarget(**{f.name: torch.cat([getattr(p, f.name) for p in parts]) for f in fields(ReportTarget)})

    def _rows(self, x, tg):
        lin = spectral_report(self.plan.values(x, VALUE_MAG), tg.values, tg.floors, 1)
        mel = spectral_report(self.mel.frames_major(x), tg.mel_values, tg.mel_floors, self.mel_power, dct=self.dct)
        est = estimate_pitch(x, self.sample_rate)
        voiced = est.voiced & tg.voiced
        nan = torch.full_like(lin[:, 0], float("nan"))
        cents = torch.where(voiced, 100.0 * (est.midi.double() - tg.midi.double()), nan)
        rms_x, rms_y = envelope_frames(x, ENVELOPE_W, ENVELOPE_HOP).double(), tg.rms.double()
        gate = rms_y.max(dim=1, keepdim=True).values * 10.0 ** (-self.dynamic_range_db / 20.0)
        sounding = rms_y > gate
        floor = gate.clamp_min(FLOOR_MIN)
        err = (20.0 * torch.log10(rms_x.clamp_min(floor) / rms_y.clamp_min(floor))).abs()
        env = (err * sounding).sum(dim=1) / sounding.sum(dim=1).clamp_min(1)
        return MatchReport(lsd_db=lin[:, 0], spectral_convergence=lin[:, 1], logmel_l1_db=mel[:, 2], mcd_db=mel[:, 3],
                           frames=lin[:, 4].long(), mel_frames=mel[:, 4].long(), envelope_db=env, f0_cents=cents,
                           voiced=voiced)

    @torch.no_grad()
    def __call__(self, audio, target_audio=None, target=None):
        """audio [N, T] against ``target_audio`` [N, T] or the ``target`` that ``self.target`` made of it -> ``MatchReport``."""
        x = self._audio(audio, "audio")
        if (target_audio is None) == (target is None):
            raise ValueError("Reporter: pass exactly one of target_audio and target")
        self._to(x.device)
        N = x.shape[0]
        if N < 1:
            raise ValueError("Reporter: audio has no rows")
        if target is None:
            y = self._audio(target_audio, "target_audio")
            if y.shape != x.shape:
                raise ValueError(f"Reporter: audio {tuple(x.shape)} and target_audio {tuple(y.shape)} differ in shape")
        elif target.values.shape[0] != N or target.rms.shape[1] != (x.shape[1] - ENVELOPE_W) // ENVELOPE_HOP + 1:
            raise ValueError(f"Reporter: the target is of {target.values.shape[0]} sounds of another length, audio "
                             f"{tuple(x.shape)}")
        parts = []
        for lo in range(0, N, CHUNK_ROWS):
            hi = min(lo + CHUNK_ROWS, N)
            tg = target.rows(lo, hi) if target is not None else self._target_rows(y[lo:hi])
            parts.append(self._rows(x[lo:hi], tg))
        if len(parts) == 1:
            return parts[0]
        return MatchReport(**{f.name: torch.cat([getattr(p, f.name) for p in parts]) for f in fields(MatchReport)})

"""fp64 numpy restatement of the contracts of ias_onset_flux, ias_onset_pick, ias_segment_gather and ias_segment_scatter
(include/ias_hip.h), of the descriptor logic of ``onset.split_notes``, and the note sequences of the onset tests.

Written from the contracts' text, not from the kernels.  The mel spectrogram of ``detect`` is torch.stft in fp64 (centred,
reflect padding, periodic Hann window, power 2) through the project's ``melscale_fbanks``."""
import numpy as np
import torch

import pitch_model as pm


# ------------------------------------------------------------------------------------------------ the four contracts
def logmel(mel, gamma):
    """mel [..., M] -> fp32(log1p((double)gamma (double)mel)), gamma as the fp32 the entry receives."""
    g = np.float64(np.float32(gamma))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return np.log1p(g * np.asarray(mel, dtype=np.float32).astype(np.float64)).astype(np.float32)


def flux_from_logmel(L, lag):
    """L [F, M] fp32 -> flux [F] fp32: per frame one fp64 chain over m ascending of the positive part of the exact
    difference to the frame ``lag`` earlier (+0 before the first frame), divided by M, rounded to fp32 once."""
    L = np.asarray(L, dtype=np.float32).astype(np.float64)
    F, M = L.shape
    prev = np.zeros_like(L)
    if lag < F:
        prev[lag:] = L[:F - lag]
    with np.errstate(invalid="ignore"):
        diff = L - prev
        pos = np.where(diff > 0.0, diff, 0.0)
    acc = np.zeros(F)
    for m in range(M):                                                 # the chain: ascending m, every frame at once
        acc = acc + pos[:, m]
    return (acc / np.float64(M)).astype(np.float32)


def flux(mel, lag, gamma):
    return flux_from_logmel(logmel(mel, gamma), lag)


def pick(x, pre_max, post_max, pre_avg, post_avg, delta, wait, K):
    """x [F] fp32 -> (frames [K] int32, strength [K] fp32, count)."""
    x = np.asarray(x, dtype=np.float32)
    F = len(x)
    d = np.float64(np.float32(delta))
    accepted = []
    with np.errstate(invalid="ignore"):
        for f in range(F):
            lo, hi = max(0, f - pre_max), min(F - 1, f + post_max)
            if not all(x[f] >= x[g] for g in range(lo, hi + 1)):
                continue
            lo, hi = max(0, f - pre_avg), min(F - 1, f + post_avg)
            s = np.float64(0.0)
            for g in range(lo, hi + 1):
                s = s + np.float64(x[g])
            if not np.float64(x[f]) >= s / np.float64(hi - lo + 1) + d:
                continue
            if not accepted or f - accepted[-1] > wait:
                accepted.append(f)
    frames = np.full(K, -1, dtype=np.int32)
    strength = np.zeros(K, dtype=np.float32)
    n = min(len(accepted), K)
    frames[:n] = accepted[:n]
    strength[:n] = x[accepted[:n]]
    return frames, strength, len(accepted)


def fade_factor(t, length, fade):
    """fp32((float)(length - t) * inv_fade) with inv_fade = fp32(1 / fade)."""
    return np.float32(np.float32(length - t) * np.float32(1.0 / fade))


def gather(audio, row, start, length, faded, T, fade):
    audio = np.asarray(audio, dtype=np.float32)
    N, L = audio.shape
    out = np.zeros((len(row), T), dtype=np.float32)
    for s in range(len(row)):
        for t in range(min(int(length[s]), T)):
            i = int(start[s]) + t
            v = audio[row[s], i] if 0 <= row[s] < N and 0 <= i < L else np.float32(0.0)
            if faded[s] and t >= int(length[s]) - fade:
                v = np.float32(v * fade_factor(t, int(length[s]), fade))
            out[s, t] = v
    return out


def scatter(notes, row, start, length, faded, fade, gain, N, L):
    notes = np.asarray(notes, dtype=np.float32)
    T = notes.shape[1]
    out = np.zeros((N, L), dtype=np.float32)
    for s in range(len(row)):
        if not 0 <= row[s] < N:
            continue
        for t in range(min(int(length[s]), T)):
            i = int(start[s]) + t
            if not 0 <= i < L:
                continue
            v = np.float32(notes[s, t] * np.float32(gain[s]))
            if faded[s] and t >= int(length[s]) - fade:
                v = np.float32(v * fade_factor(t, int(length[s]), fade))
            out[row[s], i] = v
    return out


def descriptors(lengths, samples, T):
    """The segments of ``onset.split_notes``: lengths [N], samples [N, K] (negative: unused) -> lists (row, start,
    length, faded) in row order."""
    row, start, length, faded = [], [], [], []
    for i, n in enumerate(int(v) for v in lengths):
        ons = []
        for s in (int(v) for v in samples[i]):
            if 0 <= s < n and (not ons or s != ons[-1]):
                ons.append(s)
        if not ons:
            ons = [0]
        for k, s in enumerate(ons):
            nxt = ons[k + 1] if k + 1 < len(ons) else None
            end = min(e for e in (nxt, s + T, n) if e is not None)
            row.append(i)
            start.append(s)
            length.append(max(end - s, 0))
            faded.append(int(end < n))
    return row, start, length, faded


# ------------------------------------------------------------------------------------------------ the detector
def mel_power(x, rate, n_fft, hop, n_mels):
    """x [T] -> [F, n_mels] fp64 mel power values, F = 1 + T // hop."""
    from inverse_audio_synthesis_amd.spectral import melscale_fbanks
    xt = torch.from_numpy(np.asarray(x, dtype=np.float64))
    spec = torch.stft(xt, n_fft, hop_length=hop, window=torch.hann_window(n_fft, dtype=torch.float64), center=True,
                      pad_mode="reflect", return_complex=True)
    power = spec.real ** 2 + spec.imag ** 2                                       # [n_fft / 2 + 1, F]
    fb = melscale_fbanks(n_fft // 2 + 1, 0.0, float(rate // 2), n_mels, rate).double()
    return (power.T @ fb).numpy()


def detect(x, rate, n_fft=1024, hop=256, n_mels=128, lag=2, gamma=100.0, pre_max=3, post_max=3, pre_avg=10, post_avg=10,
           delta=0.2, wait=4, K=256):
    """``onset.detect_onsets`` for one row -> (samples [count] int, frames [count], flux [F] fp32)."""
    fl = flux(mel_power(x, rate, n_fft, hop, n_mels).astype(np.float32), lag, gamma)
    frames, _strength, count = pick(fl, pre_max, post_max, pre_avg, post_avg, delta, wait, K)
    frames = frames[:min(count, K)].astype(np.int64)
    return np.maximum(frames - lag, 0) * hop, frames, fl


# ------------------------------------------------------------------------------------------------ test signals
# (wave, MIDI, amplitude, onset in seconds): four decaying notes in three seconds
NOTES = (("saw", 48.0, 0.5, 0.0625), ("sine", 60.0, 0.3, 0.7716), ("square", 55.0, 0.5, 1.466),
         ("saw_noise", 67.0, 0.1, 2.25))
SECONDS = 3.0
ATTACK, DECAY = 0.002, 0.15


def note_onsets(rate, notes=NOTES):
    return np.array([int(round(t * rate)) for _k, _m, _a, t in notes])


def note_sequence(rate, notes=NOTES, seconds=SECONDS, noise=0.0, seed=0):
    """fp32 [seconds rate]: every note a ``pitch_model.tone`` from its onset to the end under a 2 ms linear attack and an
    exp(-t / 0.15 s) decay, summed; ``noise``: the standard deviation of added white noise."""
    T = int(round(seconds * rate))
    x = np.zeros(T)
    for i, ((kind, midi, amp, _t), at) in enumerate(zip(notes, note_onsets(rate, notes))):
        n = T - at
        t = np.arange(n) / rate
        env = np.minimum(t / ATTACK, 1.0) * np.exp(-t / DECAY)
        x[at:] += (amp / 0.5) * pm.tone(kind, midi, rate, n, seed=100 + i).astype(np.float64) * env
    if noise > 0.0:
        x = x + noise * np.random.default_rng(seed + 7).standard_normal(T)
    return x.astype(np.float32)


SAW_PERIOD = 125                                                       # samples: 128 Hz at 16 kHz


def detector_rows(rate):
    """-> rows [5, T] fp32: the notes, the notes in 1e-3 white noise, silence, white noise of standard deviation 0.1, and
    a steady saw.  The saw's period is a whole number of samples (SAW_PERIOD): ``pitch_model.tone``'s saw is not
    band-limited, and at a fractional period its aliased partials beat, which is not a steady sound."""
    T = int(round(SECONDS * rate))
    saw_midi = 69.0 + 12.0 * np.log2(rate / SAW_PERIOD / 440.0)
    rows = [note_sequence(rate), note_sequence(rate, noise=1e-3), np.zeros(T, dtype=np.float32),
            (0.1 * pm.tone("noise", 0, rate, T, seed=41)).astype(np.float32), pm.tone("saw", saw_midi, rate, T)]
    return np.stack(rows)

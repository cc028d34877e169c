"""fp64 numpy restatement of the ias_pitch_yin contract (include/ias_hip.h) and the test signals of the pitch tests.

Written from the contract's text, not from the kernel: the difference function d and the energy as plain fp64 sums, the
running sum c in fp64, d' = d tau / c (1 at tau = 0 and where c == 0), the pick and the parabolic refinement on d' rounded
to fp32, and the aggregation through ``pitch.aggregate_pitch`` (plain torch, here on CPU tensors)."""
import numpy as np
import torch


def num_frames(T, W, tau_max, hop):
    return (T - W - tau_max) // hop + 1


def difference(x, W, tau_max, hop):
    """x [T] -> (d [F, tau_max + 1] with d[:, 0] = 0, energy [F]) in fp64."""
    x = np.asarray(x, dtype=np.float64)
    F = num_frames(len(x), W, tau_max, hop)
    assert F >= 1
    starts = np.arange(F) * hop
    base = x[starts[:, None] + np.arange(W)[None, :]]                  # [F, W]
    d = np.zeros((F, tau_max + 1))
    for tau in range(1, tau_max + 1):
        diff = base - x[starts[:, None] + np.arange(W)[None, :] + tau]
        d[:, tau] = (diff * diff).sum(axis=1)
    return d, (base * base).sum(axis=1)


def dprime(x, W, tau_max, hop):
    """-> (d' [F, tau_max + 1] fp64 (unrounded), c [F, tau_max + 1], energy [F])."""
    d, energy = difference(x, W, tau_max, hop)
    c = np.cumsum(d, axis=1)
    tau = np.arange(tau_max + 1, dtype=np.float64)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        dp = np.where(c == 0.0, 1.0, d * tau / c)
    dp[:, 0] = 1.0
    return dp, c, energy


def refine(dp_row, tau, tau_min, tau_max):
    """The contract's period for the picked lag ``tau`` of one frame's d' (any float dtype; computed in fp64)."""
    if tau_min < tau < tau_max:
        y0, y1, y2 = (float(dp_row[tau - 1]), float(dp_row[tau]), float(dp_row[tau + 1]))
        den = y0 - 2.0 * y1 + y2
        if den > 0.0:
            return tau + (y0 - y2) / (2.0 * den)
    return float(tau)


def pick(dp, tau_min, tau_max, threshold):
    """dp [F, tau_max + 1] -> (tau [F] int, period [F] fp64, aperiodicity [F] in dp's dtype).  The comparisons are made on
    the values as given: hand it fp32 to restate the contract, the kernel's own output to check the kernel's pick."""
    dp = np.asarray(dp)
    thr = dp.dtype.type(threshold)
    F = dp.shape[0]
    taus, periods, aper = np.zeros(F, dtype=np.int64), np.zeros(F), np.zeros(F, dtype=dp.dtype)
    for f in range(F):
        row = dp[f]
        seg = row[tau_min:tau_max + 1]
        below = np.nonzero(seg < thr)[0]
        if len(below):
            t = tau_min + int(below[0])
            while t + 1 <= tau_max and row[t + 1] < row[t]:
                t += 1
        else:
            t = tau_min + int(np.argmin(seg))                          # argmin: the first of equal minima
        taus[f], periods[f], aper[f] = t, refine(row, t, tau_min, tau_max), row[t]
    return taus, periods, aper


def yin(x, W, tau_min, tau_max, hop, threshold):
    """The whole contract for one row -> (period [F] fp64, aperiodicity [F] fp32, energy [F] fp64, tau [F])."""
    dp, _c, energy = dprime(x, W, tau_max, hop)
    taus, periods, aper = pick(dp.astype(np.float32), tau_min, tau_max, np.float32(threshold))
    return periods, aper, energy, taus


def frame_midi(period, rate):
    return 69.0 + 12.0 * np.log2(rate / np.asarray(period, dtype=np.float64) / 440.0)


def estimate(rows, rate, W, tau_min, tau_max, hop, threshold=0.15, gate_db=-30.0, min_voiced=3):
    """rows [N, T] -> pitch.PitchEstimate from the model's frames, aggregated by pitch.aggregate_pitch on CPU tensors."""
    from inverse_audio_synthesis_amd.pitch import aggregate_pitch
    out = [yin(r, W, tau_min, tau_max, hop, threshold) for r in rows]
    as_t = lambda k: torch.from_numpy(np.stack([o[k] for o in out]).astype(np.float32))   # noqa: E731
    return aggregate_pitch(as_t(0), as_t(1), as_t(2), rate, threshold=threshold, gate_db=gate_db, min_voiced=min_voiced)


# ------------------------------------------------------------------------------------------------ test signals
def midi_hz(m):
    return 440.0 * 2.0 ** ((m - 69.0) / 12.0)


def tone(kind, midi, rate, T, seed=0):
    """fp32 [T]: "sine", naive (not band-limited) "saw" and "square", "saw_noise" (the saw plus white noise of 0.05 of its
    standard deviation), "noise" (white, ``midi`` unused)."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.standard_normal(T).astype(np.float32)
    ph = (np.arange(T) * (midi_hz(midi) / rate)) % 1.0
    if kind == "sine":
        y = np.sin(2.0 * np.pi * ph)
    elif kind == "square":
        y = np.where(ph < 0.5, 1.0, -1.0)
    elif kind in ("saw", "saw_noise"):
        y = 2.0 * ph - 1.0
        if kind == "saw_noise":
            y = y + 0.05 * y.std() * rng.standard_normal(T)
    else:
        raise ValueError(kind)
    return (0.5 * y).astype(np.float32)


TONE_KINDS = ("sine", "saw", "square", "saw_noise")
TONE_MIDIS = tuple(36.0 + 3.7 * i for i in range(10))                  # 36 .. 69.3: MIDI 36 to 72 in steps of 3.7

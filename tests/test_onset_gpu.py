"""ias_onset_flux, ias_onset_pick, ias_segment_gather and ias_segment_scatter on the GPU against the fp64 model of their
contracts (tests/onset_model.py), their bit guarantees across batch layouts, ``detect_onsets`` / ``split_notes`` /
``join_notes`` end to end on the note sequences, and ``match_audio.py --split``."""
import functools
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import onset_model as om

pytestmark = pytest.mark.gpu

RATE = 16000
HOP = 256


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _offset_copy(t, off):
    """A contiguous copy of ``t`` whose first element sits ``off`` floats past a 16-byte boundary."""
    flat = torch.zeros(t.numel() + 8, dtype=t.dtype, device=t.device)
    flat[off:off + t.numel()] = t.reshape(-1)
    view = flat[off:off + t.numel()].view(t.shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * off
    return view


# ------------------------------------------------------------------------------------------------ flux
# (B, F, M, lag): M and F multiples of neither the 16-frame tile nor the wave, more than one tile; every frame before lag
FLUX_CASES = [(3, 37, 40, 2), (2, 130, 128, 1), (1, 5, 7, 4), (1, 2, 3, 2)]
GAMMA = 100.0


@functools.lru_cache(maxsize=None)
def _flux_inputs(case):
    B, F, M, lag = FLUX_CASES[case]
    rng = np.random.default_rng(20 + case)
    mel = (rng.random((B, F, M)) ** 4 * 10.0).astype(np.float32)
    if B > 1:
        mel[1] = 0.0                                                   # an all-zero row
    mel[0, 0, 0] = np.float32(1e-42)                                   # a subnormal
    mel[0, 0, M - 1] = np.float32(1e30)
    if F > lag:
        mel[0, lag] = mel[0, 0]                                        # an exact repeat between lagged frames
        mel[0, F - 1, : M // 2] = mel[0, F - 1 - lag, : M // 2]
    mel[B - 1, F // 2, M // 2] = 0.0
    return mel


@functools.lru_cache(maxsize=None)
def _flux_kernel(case):
    from inverse_audio_synthesis_amd.onset import onset_flux
    lag = FLUX_CASES[case][3]
    flux, logmel = onset_flux(torch.from_numpy(_flux_inputs(case)).cuda(), lag=lag, gamma=GAMMA, return_logmel=True)
    torch.cuda.synchronize()
    return flux.cpu().numpy(), logmel.cpu().numpy()


@pytest.mark.parametrize("case", range(len(FLUX_CASES)))
def test_flux_matches_the_model(lib, dev, case):
    """(a) logmel within 1 fp32 ulp of the model's fp32(log1p(gamma mel)) (the device's fp64 log1p is not correctly
    rounded, so the one rounding to fp32 can fall the other way); (b) the model's flux computed from the KERNEL's logmel is
    the kernel's flux, bit for bit."""
    B, F, M, lag = FLUX_CASES[case]
    mel = _flux_inputs(case)
    flux, logmel = _flux_kernel(case)
    assert flux.shape == (B, F) and logmel.shape == (B, F, M)
    want = om.logmel(mel, GAMMA)
    ulp = np.spacing(np.abs(want))
    off = np.abs(logmel.astype(np.float64) - want.astype(np.float64)) / ulp
    print(f"case {case}: logmel differs in {(off > 0).sum()} of {off.size} values, at most {off.max():.1f} ulp")
    assert off.max() <= 1.0
    assert (logmel[mel == 0.0] == 0.0).all() and not np.signbit(logmel[mel == 0.0]).any()
    for b in range(B):
        assert np.array_equal(_bits(flux[b]), _bits(om.flux_from_logmel(logmel[b], lag))), b
    if B > 1:
        assert (flux[1] == 0.0).all()
    if F > lag:
        assert flux[0, lag] == 0.0                                     # the repeated frame: every difference is exactly 0


@pytest.mark.parametrize("case", range(len(FLUX_CASES)))
def test_flux_bits_do_not_depend_on_the_batch(lib, dev, case):
    """Rows permuted, the batch padded with other rows, a row alone at an offset of 1 to 3 floats, logmel = NULL: the same
    bits per frame."""
    from inverse_audio_synthesis_amd.onset import onset_flux
    B, F, M, lag = FLUX_CASES[case]
    x = torch.from_numpy(_flux_inputs(case)).to(dev)
    ref_flux, ref_logmel = _flux_kernel(case)
    plain = onset_flux(x, lag=lag, gamma=GAMMA)
    assert np.array_equal(_bits(plain.cpu().numpy()), _bits(ref_flux))
    extra = torch.from_numpy(np.random.default_rng(9).random((2, F, M)).astype(np.float32)).to(dev)
    perm = list(range(B))[::-1]
    mixed = torch.cat([extra[:1], x[perm], extra[1:]]).contiguous()
    got_flux, got_logmel = onset_flux(mixed, lag=lag, gamma=GAMMA, return_logmel=True)
    assert np.array_equal(_bits(got_flux[1:1 + B].cpu().numpy()), _bits(ref_flux[perm]))
    assert np.array_equal(_bits(got_logmel[1:1 + B].cpu().numpy()), _bits(ref_logmel[perm]))
    for off in (1, 2, 3):
        b = off % B
        got_flux, got_logmel = onset_flux(_offset_copy(x[b:b + 1], off), lag=lag, gamma=GAMMA, return_logmel=True)
        assert np.array_equal(_bits(got_flux[0].cpu().numpy()), _bits(ref_flux[b]))
        assert np.array_equal(_bits(got_logmel[0].cpu().numpy()), _bits(ref_logmel[b]))


# ------------------------------------------------------------------------------------------------ pick
# 1, 70 and 1000 frames fit one 1024-frame pass of the workgroup; 2500 takes three (the two mask buffers alternate)
PICK_F = (1, 70, 1000, 2500)
PICK = dict(pre_max=3, post_max=3, pre_avg=10, post_avg=10, delta=0.2, wait=4)
PICK_K = 4


@functools.lru_cache(maxsize=None)
def _pick_inputs(F):
    """[3, F]: a row with a plateau, two peaks closer than wait, peaks at frame 0 and F - 1 and more onsets than K; an
    all-zero row; the first row with a NaN."""
    rng = np.random.default_rng(F)
    x = np.zeros((3, F), dtype=np.float32)
    r = x[0]
    r[:] = 0.01 * rng.random(F).astype(np.float32)
    r[0] = 1.0
    r[F - 1] = 1.5
    if F >= 70:
        r[10:12] = 2.0                                                 # equal neighbours
        r[30], r[33] = 2.5, 3.0                                        # 3 frames apart: inside each other's maximum window
        r[40], r[44] = 2.0, 2.25                                       # 4 frames apart: two maxima, the second within wait
        for f in range(55, F - 5, 37):
            r[f] = 1.0 + 0.001 * f
    x[2] = x[0]
    x[2, min(57, F - 1)] = np.nan                                      # in the windows of the peak at 55
    return x


@functools.lru_cache(maxsize=None)
def _pick_model(F):
    return [om.pick(r, K=PICK_K, **PICK) for r in _pick_inputs(F)]


def _run_pick(x, K=PICK_K):
    from inverse_audio_synthesis_amd.onset import onset_pick
    frames, strength, count = onset_pick(x, max_onsets=K, **PICK)
    torch.cuda.synchronize()
    return frames.cpu().numpy(), strength.cpu().numpy(), count.cpu().numpy()


@pytest.mark.parametrize("F", PICK_F)
def test_pick_matches_the_model(lib, dev, F):
    x = _pick_inputs(F)
    frames, strength, count = _run_pick(torch.from_numpy(x).to(dev))
    assert frames.dtype == np.int32 and frames.shape == (3, PICK_K) and count.shape == (3,)
    for b, (wf, ws, wc) in enumerate(_pick_model(F)):
        assert frames[b].tolist() == wf.tolist() and int(count[b]) == wc, (b, frames[b], wf, count[b], wc)
        assert np.array_equal(_bits(strength[b]), _bits(ws))
    assert int(count[1]) == 0 and (frames[1] == -1).all() and (strength[1] == 0).all()
    if F >= 70:
        wf, _ws, wc = _pick_model(F)[0]
        assert wc > PICK_K and wf.tolist() == [0, 10, 33, 40]          # 11: the plateau's second frame; 30 < 33; 44 waits
        assert _pick_model(F)[2][2] < wc                               # the NaN takes candidates away


@pytest.mark.parametrize("F", PICK_F)
def test_pick_does_not_depend_on_the_batch(lib, dev, F):
    x = torch.from_numpy(_pick_inputs(F)).to(dev)
    ref = _run_pick(x, K=64)
    for b, (wf, _ws, wc) in enumerate(_pick_model(F)):                 # K = 64: every onset of the 70- and 1000-frame rows
        assert int(ref[2][b]) == wc and ref[0][b, :PICK_K].tolist() == wf.tolist()
    extra = torch.from_numpy(np.random.default_rng(3).random((2, F)).astype(np.float32)).to(dev)
    perm = [2, 0, 1]
    got = _run_pick(torch.cat([extra[:1], x[perm], extra[1:]]).contiguous(), K=64)
    for g, want in zip(got, ref):
        assert np.array_equal(g[1:4].view(np.uint32), want[perm].view(np.uint32))
    for off in (1, 2, 3):
        b = off % 3
        got = _run_pick(_offset_copy(x[b:b + 1], off), K=64)
        for g, want in zip(got, ref):
            assert np.array_equal(g[0].view(np.uint32), want[b].view(np.uint32))


# ------------------------------------------------------------------------------------------------ gather / scatter
SEG_N, SEG_L, SEG_T, SEG_FADE = 2, 4099, 1000, 64
# (row, start, length, faded): starts at every 16-byte phase (L is odd, so row 1 shifts the phase once more), a length of
# T, a length below the fade, faded and unfaded notes, the last of row 0 running past L; no two overlap
SEGMENTS = [(0, 0, 1000, 1), (0, 1001, 700, 0), (0, 1702, 10, 1), (0, 1803, 999, 1), (0, 3599, 1000, 1),
            (1, 3, 500, 0), (1, 600, 1000, 0), (1, 2001, 333, 1)]
# descriptors a caller should not produce: rows outside [0, N), a negative start, a negative length, a length over T; no
# two overlap
HOSTILE = [(-1, 0, 100, 1), (2, 5, 100, 0), (0, -7, 50, 1), (1, 4090, 1000, 0), (1, 10, -5, 1), (0, 2000, 1500, 1)]


def _desc(segs, dev):
    cols = list(zip(*segs))
    return (torch.tensor(cols[0], dtype=torch.int32, device=dev), torch.tensor(cols[1], dtype=torch.int32, device=dev),
            torch.tensor(cols[2], dtype=torch.int32, device=dev), torch.tensor(cols[3], dtype=torch.uint8, device=dev))


def _gather(lib, audio, segs, T=SEG_T, fade=SEG_FADE):
    from inverse_audio_synthesis_amd import _lib
    row, start, length, faded = _desc(segs, audio.device)
    out = torch.full((len(segs), T), float("nan"), dtype=torch.float32, device=audio.device)
    st = lib.ias_segment_gather(_lib.ptr(audio), audio.shape[0], audio.shape[1], _lib.ptr(row), _lib.ptr(start),
                                _lib.ptr(length), _lib.ptr(faded), len(segs), T, fade, 1.0 / fade, _lib.ptr(out),
                                _lib.stream())
    assert st == 0
    return out


def _scatter(lib, notes, segs, gain, N=SEG_N, L=SEG_L, fade=SEG_FADE):
    from inverse_audio_synthesis_amd import _lib
    row, start, length, faded = _desc(segs, notes.device)
    out = torch.zeros((N, L), dtype=torch.float32, device=notes.device)
    g = torch.tensor(gain, dtype=torch.float32, device=notes.device)
    st = lib.ias_segment_scatter(_lib.ptr(notes), N, L, _lib.ptr(row), _lib.ptr(start), _lib.ptr(length), _lib.ptr(faded),
                                 len(segs), notes.shape[1], fade, 1.0 / fade, _lib.ptr(g), _lib.ptr(out), _lib.stream())
    assert st == 0
    return out


@functools.lru_cache(maxsize=None)
def _seg_audio():
    return np.random.default_rng(77).standard_normal((SEG_N, SEG_L)).astype(np.float32)


@pytest.mark.parametrize("segs", [SEGMENTS, HOSTILE], ids=["segments", "hostile"])
def test_gather_and_scatter_match_the_model(lib, dev, segs):
    audio = _seg_audio()
    cols = list(zip(*segs))
    got = _gather(lib, torch.from_numpy(audio).to(dev), segs).cpu().numpy()
    want = om.gather(audio, *cols, SEG_T, SEG_FADE)
    assert np.array_equal(_bits(got), _bits(want))
    notes = np.random.default_rng(78).standard_normal((len(segs), SEG_T)).astype(np.float32)
    gain = [0.5 + 0.37 * s for s in range(len(segs))]
    back = _scatter(lib, torch.from_numpy(notes).to(dev), segs, gain).cpu().numpy()
    assert np.array_equal(_bits(back), _bits(om.scatter(notes, *cols, SEG_FADE, gain, SEG_N, SEG_L)))


def test_gather_at_every_phase_of_both_sides(lib, dev):
    """T = 1001 moves the note buffers through every 16-byte phase as well, and the audio sits 1 to 3 floats past a
    16-byte boundary: every pairing of load and store phase."""
    audio = _seg_audio()
    segs = [(s % 2, 1012 * (s // 2) + s % 4, 1001 - 3 * s, s % 2) for s in range(8)]      # no two overlap
    want = om.gather(audio, *zip(*segs), 1001, SEG_FADE)
    for off in (0, 1, 2, 3):
        a = _offset_copy(torch.from_numpy(audio).to(dev), off)
        assert np.array_equal(_bits(_gather(lib, a, segs, T=1001).cpu().numpy()), _bits(want))
    gain = [1.0 + 0.1 * s for s in range(8)]
    back = _scatter(lib, torch.from_numpy(want).to(dev), segs, gain).cpu().numpy()
    assert np.array_equal(_bits(back), _bits(om.scatter(want, *zip(*segs), SEG_FADE, gain, SEG_N, SEG_L)))


def test_gather_then_scatter_returns_the_audio(lib, dev):
    """Gain 1: the audio's bits outside the fades, exact zeros between the segments."""
    audio = _seg_audio()
    a = torch.from_numpy(audio).to(dev)
    back = _scatter(lib, _gather(lib, a, SEGMENTS), SEGMENTS, [1.0] * len(SEGMENTS)).cpu().numpy()
    covered = np.zeros(audio.shape, dtype=bool)
    plain = np.zeros(audio.shape, dtype=bool)
    for r, s, n, f in SEGMENTS:
        covered[r, s:s + n] = True
        plain[r, s:max(s, s + n - (SEG_FADE if f else 0))] = True
    assert np.array_equal(_bits(back[plain]), _bits(audio[plain]))
    assert (back[~covered] == 0).all() and not np.signbit(back[~covered]).any()
    assert (np.abs(back[covered & ~plain]) <= np.abs(audio[covered & ~plain])).all() and (covered & ~plain).sum() > 0


def test_split_and_join_notes(lib, dev):
    """``split_notes`` builds the model's descriptors on the device and gathers; ``join_notes`` scatters them back."""
    from inverse_audio_synthesis_amd.onset import join_notes, split_notes
    audio = _seg_audio()
    lengths = [4099, 3000]
    samples = [[100, 900, 1500, 4000, -1], [-1, -1, -1, -1, -1]]
    seg = split_notes(torch.from_numpy(audio).to(dev), torch.tensor(lengths), torch.tensor(samples, device=dev), SEG_T,
                      SEG_FADE)
    row, start, length, faded = om.descriptors(lengths, samples, SEG_T)
    assert (seg.row.tolist(), seg.start.tolist(), seg.length.tolist(), seg.faded.tolist()) == (row, start, length, faded)
    assert seg.row.dtype == torch.int32 and seg.faded.dtype == torch.uint8 and seg.audio.shape == (5, SEG_T)
    want = om.gather(audio, row, start, length, faded, SEG_T, SEG_FADE)
    assert np.array_equal(_bits(seg.audio.cpu().numpy()), _bits(want))
    gain = [1.0, 0.5, 2.0, 1.0, 0.25]
    back = join_notes(seg.audio, seg, 2, SEG_L, torch.tensor(gain)).cpu().numpy()
    assert np.array_equal(_bits(back), _bits(om.scatter(want, row, start, length, faded, SEG_FADE, gain, 2, SEG_L)))


# ------------------------------------------------------------------------------------------------ detect_onsets
@functools.lru_cache(maxsize=None)
def _rows():
    return om.detector_rows(RATE)


@functools.lru_cache(maxsize=None)
def _model_rows():
    return [om.detect(r, RATE) for r in _rows()]


def test_detect_onsets_on_the_note_sequences(lib, dev):
    """16 kHz, the defaults: the four notes (clean, and in 1e-3 white noise), silence, white noise and a steady saw in one
    batch.  The fp64 model finds exactly the four notes with samples - truth in [-2.23, -1.62] hops, nothing in silence,
    one onset at frame 1 in the noise, and in the saw one at frame 0 and one at the last frame (the reflect padding at the
    end of the file, tests/test_onset_cpu.py).  Asserted on the device: the model's counts, and for the notes
    -3 hops <= samples - truth <= 0 (the model's bound [-2.5, -0.5] hops with half a hop each side for the fp32 mel)."""
    from inverse_audio_synthesis_amd.onset import detect_onsets
    x = torch.from_numpy(_rows()).to(dev)
    res = detect_onsets(x, RATE)
    F = 1 + x.shape[1] // HOP
    assert res.frames.shape == (5, 256) and res.flux.shape == (5, F) and res.samples.dtype == torch.int64
    count = res.count.cpu().numpy()
    frames, samples = res.frames.cpu().numpy(), res.samples.cpu().numpy()
    model = _model_rows()
    print("counts:", count.tolist(), "model:", [len(m[0]) for m in model])
    assert [len(m[0]) for m in model] == [4, 4, 0, 1, 2]
    assert count.tolist() == [len(m[0]) for m in model]
    truth = om.note_onsets(RATE)
    for b in (0, 1):
        err = (samples[b, :4] - truth) / HOP
        print(f"row {b}: samples - truth in hops {err.tolist()}, model {((model[b][0] - truth) / HOP).tolist()}")
        assert err.min() >= -3.0 and err.max() <= 0.0
    assert (frames[2] == -1).all() and (samples[2] == -1).all() and (res.flux[2] == 0).all()
    assert frames[3, 0] <= 1 and samples[3, 0] == 0
    assert frames[4, 0] <= 1 and samples[4, 0] == 0 and frames[4, 1] == F - 1
    for b in range(5):
        assert (frames[b, count[b]:] == -1).all()
        assert (samples[b, :count[b]] == np.maximum(frames[b, :count[b]] - 2, 0) * HOP).all()
    # the flux itself: the fp32 mel of the device against the fp64 one of the model, where there is sound
    worst = max(float(np.abs(res.flux[b].cpu().numpy() - model[b][2]).max()) for b in (0, 1, 3, 4))
    print(f"flux: worst absolute difference to the model {worst:.3e}")


# ------------------------------------------------------------------------------------------------ match_audio.py
def _write_pcm16(path, x, rate):
    pcm = np.clip(np.round(np.asarray(x, dtype=np.float64) * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.tobytes())
    return pcm.astype(np.float64) / 32768.0


def _read_pcm16(path):
    with wave.open(str(path), "rb") as w:
        assert w.getnchannels() == 1 and w.getsampwidth() == 2
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.float64) / 32768.0, w.getframerate()


def _match_audio(tmp_path, *flags):
    from conftest import ROOT
    target = _write_pcm16(tmp_path / "phrase.wav", _rows()[0], RATE)
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "match_audio.py"), str(tmp_path / "phrase.wav"), "torchsynth.rate=16000",
           "torchsynth.buffer_size_seconds=1.0", "--steps", "2", "--out", str(out), *flags]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:]
    return target, out, r.stdout


def test_match_audio_split_entry_point(lib, dev, tmp_path):
    target, out, _log = _match_audio(tmp_path, "--split", "--pitch")
    doc = json.load(open(out / "phrase.notes.json"))
    assert doc["input"] == "phrase.wav" and doc["rate"] == RATE and len(doc["notes"]) == 4
    truth = om.note_onsets(RATE)
    match, rate = _read_pcm16(out / "phrase.match.wav")
    assert rate == RATE and len(match) == 48000
    for note, at, midi in zip(doc["notes"], truth, (48.0, 60.0, 55.0, 67.0)):
        err = (note["onset_sample"] - at) / HOP
        assert -3.0 <= err <= 0.0 and note["onset_seconds"] == note["onset_sample"] / RATE
        assert note["voiced"] is True and abs(note["estimated_midi"] - midi) <= 0.5, (note["estimated_midi"], midi)
        assert len(note["params"]) == 78 and note["strength"] > 0.2 and note["gain"] > 0.0
        a, n = note["onset_sample"], note["length_samples"]
        db = 20.0 * np.log10(np.sqrt((match[a:a + n] ** 2).mean()) / np.sqrt((target[a:a + n] ** 2).mean()))
        print(f"note at {a}: {n} samples, estimated MIDI {note['estimated_midi']:.3f}, gain {note['gain']:.4f}, "
              f"match RMS {db:+.3f} dB against the target's")
        assert abs(db) <= 1.0
    spans = [(n["onset_sample"], n["length_samples"]) for n in doc["notes"]]
    assert all(a + n == b for (a, n), (b, _n) in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] == 48000
    assert doc["notes"][0]["onset_sample"] > 0 and (match[:doc["notes"][0]["onset_sample"]] == 0.0).all()
    assert not os.path.exists(out / "phrase.params.json")


def test_match_audio_without_split_still_crops(lib, dev, tmp_path):
    _target, out, log = _match_audio(tmp_path)
    rec = json.load(open(out / "phrase.params.json"))
    assert rec["input"] == "phrase.wav" and len(rec["params"]) == 78 and "cropped to the synth buffer of 16000" in log
    match, _rate = _read_pcm16(out / "phrase.match.wav")
    assert len(match) == 16000 and not os.path.exists(out / "phrase.notes.json")

#!/usr/bin/env python3
"""Sound matching entry point: fit the 78 Voice parameters to WAV files.

    python match_audio.py in1.wav in2.wav --steps 200 --out DIR [--init center|random|bank] [--starts S]
                          [--bank-batches NB] [--bank-stream CHUNK] [--evolve G] [--evolve-population M]
                          [--evolve-elites K] [--evolve-sigma S0] [--pitch] [--pitch-lo MIDI] [--pitch-hi MIDI]
                          [--envelope] [--envelope-generations G] [--envelope-population M]
                          [--split] [--onset-delta D] [--max-notes K] [--fade-ms MS] [--shared] [--own M.N,M.N,...]
                          [--gain solved|fitted] [--loss LOSS] [--report]
                          [key=value ...]

``key=value`` are config overrides as for pretrain.py / audio_to_params.py (``torchsynth.rate``,
``torchsynth.buffer_size_seconds``, ``mel.*``); the matcher's own settings are flags.  Input WAVs are 16-, 24- or 32-bit
integer PCM at ``torchsynth.rate``; with ``--resample`` any rate is read and brought to ``torchsynth.rate`` on the device
(``resample.resample``, torchaudio's default sinc resampler), and NAME.match.wav is resampled back to the input's rate.
Several channels are averaged; a file longer or shorter than the synth buffer is cropped or zero-padded, with a warning.  Per input NAME the script writes NAME.params.json (every
parameter in 0..1 and in its own units, the loss, its initial and final value) and NAME.match.wav (the best render,
16-bit PCM).  ``--loss``: mel_l1 (the ``mel.*`` settings), stft_l1 or multi_resolution_stft (auraloss' three resolutions,
whose 1.1 ms hop constrains the envelopes' short segments better).  ``--init``: center (every parameter 0.5), random
(``--starts`` draws per sound) or bank: a ``retrieval.SpectralBank`` of ``--bank-batches`` x 128 random voices is rendered
and each sound starts from its ``--starts`` nearest voices under the matcher's loss (a mel bank for
multi_resolution_stft); the best start is kept and the JSON record names it (``bank_index``, ``bank_distance``).  With
``--bank-stream CHUNK`` the bank is not kept: ``SpectralBank.search`` renders it CHUNK batches at a time and keeps the
running nearest voices, with the same result, so ``--bank-batches`` is bounded by time and not by memory.
``--evolve G`` (default 0: off) puts an evolutionary search between the start and the fit: ``evolve.evolve_search`` runs G
generations of ``--evolve-population`` candidates per sound (a multiple of 128) from the starts ``--init`` produced, with
the same loss as the bank and ``--seed``; its ``--starts`` best of ``--evolve-elites`` elites become the Adam starts (so
``--starts`` may exceed 1 with ``--init center``), and the JSON record names the kept one (``evolve_index``,
``evolve_distance``) in place of the bank voice.
``--pitch`` (off by default) listens to the targets first: ``pitch.estimate_pitch`` reads each target's note between
``--pitch-lo`` and ``--pitch-hi`` (MIDI, default 21..108) off the waveform and ``pitch.retune`` moves ``keyboard.midi_f0``
of every start ``--init`` produced onto it, before ``--evolve`` and the fit; unvoiced targets keep their starts.  The
JSON record gains ``estimated_midi`` (null when unvoiced), ``voiced`` and ``pitch_confidence``.
``--envelope`` (off by default) reads how long each target sounds and how it rises and falls: ``envelope.fit_envelope``
fits the Voice's envelope law (duration, attack, decay, sustain, release, alpha) to the target's RMS envelope with
``--envelope-generations`` generations of ``--envelope-population`` candidates per sound and ``--seed``, and
``envelope.reshape`` writes it into ``keyboard.duration``, ``adsr_1`` and ``adsr_2`` of every start, after ``--pitch`` and
before ``--evolve`` and the fit; silent targets keep their starts.  The JSON record gains ``envelope``: ``sounding``,
``distance`` and ``start_distance`` (1 - cos^2 between the target's envelope and the law, fitted and at the start) and the
six fitted values in their own units.
``--split`` (off by default) matches a recording note by note.  The files are read whole (after ``--resample``),
``onset.detect_onsets`` finds every file's note onsets on the device (``--onset-delta``; at most ``--max-notes`` per file,
with a warning when there are more) and ``onset.split_notes`` cuts one synth buffer per note from its onset, faded out over
``--fade-ms`` where the next note or the end of the buffer cuts it.  ``--pitch``, ``--init``, ``--evolve`` and the fit then
see the notes exactly as they see files.  Per input NAME the script writes NAME.notes.json ({input, rate, notes}: per
note ``onset_sample``, ``onset_seconds``, ``length_samples``, ``strength``, ``gain`` and the fields of a params.json record)
and NAME.match.wav at the file's full length: the best renders, each scaled by ``gain`` (the RMS of the target note over
the RMS of its render) and put back at its onset (``onset.join_notes``).
``--shared`` (off by default; needs ``--split``, one start per note) fits the notes of a file to ONE instrument.
``--init``, ``--pitch``, ``--envelope`` and ``--evolve`` run per note as before; then the notes' starts are scored once under
the matcher's loss, ``match.tie_starts`` gives every note of a file the best-scoring note's values in the tied columns, and
``SoundMatcher.fit_tied`` fits the file's notes as a group: the columns named by ``--own module.name,...`` (default
``keyboard.midi_f0,keyboard.duration``: the note and its length) stay per note, every other parameter is tied, one value
per file, descending along the mean of the notes' gradients (``ias_match_tied_step``).  NAME.notes.json gains ``shared``
({tied: the tied parameters' names, own, initial_group_loss, group_loss: the mean loss over the file's notes at the start
and at the end}) and its notes agree in every tied column; NAME.preset.json holds the tied parameters once ({input, shared,
params: ``params.json``-style rows}).
``--gain solved|fitted`` (off by default) handles the recording's level as a quantity of its own: every sound (every note
under ``--split``) gets an output gain in dB between -60 and +20, and the loss is taken on the render scaled by it
(``match.apply_gain``), so a quiet take is not paid for with the mixer levels and the envelopes' sustain.  The gain starts
at the closed-form ``match.solve_gain`` of the target against the render of the start the stages before produced; ``solved``
keeps it there, ``fitted`` makes it the 79th column of the same Adam step.  Under ``--shared`` it is per note (the note's
velocity beside tied mixer levels), and the scoring call that picks the reference note is level-matched too.  Every record
gains ``gain_mode``, ``initial_gain_db`` and ``fit_gain_db``; NAME.match.wav and ``--report`` use the gained render; the
``gain`` of a note under ``--split`` is then the RMS ratio against the gained render; NAME.preset.json is unchanged (the gain
is the note's).  The search stages (``--init bank``, ``--evolve``) score their candidates as before, at the synth's own
level: level-matched scoring there is left for a later change.
``--report`` (off by default) compares every best render with its target once after the fit, in figures that do not depend
on ``--loss``: ``report.Reporter`` (the ``mel.*`` settings for its mel plan) gives ``lsd_db``, ``spectral_convergence``,
``logmel_l1_db``, ``mcd_db``, the counted ``frames`` and ``mel_frames``, ``envelope_db``, ``f0_cents`` (null where either side
is unvoiced) and ``voiced``.  Each record (each note under ``--split``) and each stdout line gains ``report``."""
import argparse
import json
import os
import sys
import wave
import warnings
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def _refuse_rate(path, sr, rate, remedy):
    if sr != rate:
        raise ValueError(f"{path}: sample rate {sr} Hz, the synth runs at {rate} Hz (torchsynth.rate); {remedy} "
                         f"torchsynth.rate={sr}")


def read_wav_any_rate(path, rate=None):
    """-> (mono float32 samples in [-1, 1), the file's rate).  16-, 24- or 32-bit little-endian signed integer PCM,
    channels averaged; other widths, and with ``rate`` given any other rate, are refused (ValueError)."""
    with wave.open(path, "rb") as w:
        nch, width, sr, nframes = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        if rate is not None:
            _refuse_rate(path, sr, rate, "resample the file or pass")
        raw = w.readframes(nframes)
    if width == 2:
        x = np.frombuffer(raw, dtype="<i2").astype(np.float64) / 32768.0
    elif width == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        x = np.where(v >= 1 << 23, v - (1 << 24), v).astype(np.float64) / 8388608.0
    elif width == 4:
        x = np.frombuffer(raw, dtype="<i4").astype(np.float64) / 2147483648.0
    else:
        raise ValueError(f"{path}: {8 * width}-bit samples; only 16-, 24- and 32-bit integer PCM are read")
    return x.reshape(-1, nch).mean(axis=1).astype(np.float32), sr


def read_wav(path, rate):
    """-> mono float32 samples in [-1, 1).  16-, 24- or 32-bit integer PCM, channels averaged; any rate but ``rate`` is
    refused (ValueError)."""
    return read_wav_any_rate(path, rate)[0]


def write_wav(path, samples, rate):
    """Mono 16-bit PCM, the inverse of ``read_wav``'s scale (samples clipped to [-1, 32767 / 32768])."""
    x = np.asarray(samples, dtype=np.float64)
    pcm = np.clip(np.round(x * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(rate))
        w.writeframes(pcm.tobytes())


def fit_length(x, length, name="input"):
    """Crop or zero-pad to ``length`` samples, with a warning when the length changes (``name=None``: silently)."""
    if len(x) == length:
        return x
    if name is not None:
        change = "cropped" if len(x) > length else "zero-padded"
        warnings.warn(f"{name}: {len(x)} samples, {change} to the synth buffer of {length}")
    return x[:length] if len(x) > length else np.concatenate([x, np.zeros(length - len(x), dtype=x.dtype)])


def resample_rows(rows, from_rates, to_rates, dev):
    """1-D float32 arrays or tensors, row i at ``from_rates[i]`` -> 1-D device tensors, row i at ``to_rates[i]`` and of
    ``output_length`` of its own length: one ``resample`` call per distinct pair of rates, in ascending order, its rows
    zero-padded to the longest of them (a row's output does not depend on the others)."""
    import torch
    from inverse_audio_synthesis_amd.resample import resample, resample_plan, output_length
    rows = [torch.as_tensor(r) for r in rows]
    pairs = list(zip(from_rates, to_rates))
    out = [None] * len(rows)
    for a, b in sorted(set(pairs)):
        idx = [i for i, ab in enumerate(pairs) if ab == (a, b)]
        y = resample(torch.nn.utils.rnn.pad_sequence([rows[i] for i in idx], batch_first=True).to(dev), a, b)
        o, n, _w, _K = resample_plan(a, b)
        for k, i in enumerate(idx):
            out[i] = y[k, :output_length(len(rows[i]), o, n)]
    return out


def params_record(params01_row):
    """[78] params in 0..1 -> list of {module, name, value01, value} (value in the parameter's own units)."""
    from inverse_audio_synthesis_amd import voice_spec as S
    from inverse_audio_synthesis_amd.voice_grad import _from_0to1
    p = params01_row.detach().double().cpu().reshape(1, -1)
    units = _from_0to1(p)[0]
    return [{"module": m, "name": n, "value01": float(p[0, i]), "value": float(units[i])}
            for i, (m, n, *_r) in enumerate(S.PARAMS)]


@dataclass
class Targets:
    audio: object                   # [N, T] device fp32 at the synth's rate: the sounds to match (files, or notes)
    in_rates: list                  # per file: its own rate
    in_lengths: list                # per file: its length in samples at its own rate
    seg: object = None              # --split: the ``onset.NoteSegments`` of the N notes
    whole: object = None            # --split: the recordings [files, L] at the synth's rate, zero-padded to the longest


@dataclass
class Provenance:
    """Where the kept start of every sound came from, for its record."""
    bank: object = None             # (dist, idx) [N, starts] device tensors: the nearest bank voices, or None
    evolve: object = None           # (dist, idx) [N, starts]: the best elites of the evolutionary search, or None
    pitch: object = None            # ``pitch.PitchResult`` of the N sounds, or None
    envelope: object = None         # ``envelope.EnvelopeFit`` of the N sounds, or None


def split_targets(rows, files, rate, T, args):
    """--split: zero-pad the recordings (1-D device tensors at ``rate``) to the longest, find the onsets and cut one buffer
    of ``T`` samples per note -> (``onset.NoteSegments`` with S notes, the padded recordings [files, L])."""
    import torch
    from inverse_audio_synthesis_amd.onset import detect_onsets, split_notes
    lengths = torch.tensor([int(r.numel()) for r in rows], dtype=torch.int64, device=rows[0].device)
    whole = torch.nn.utils.rnn.pad_sequence(rows, batch_first=True)
    try:
        onsets = detect_onsets(whole, rate, delta=args.onset_delta, max_onsets=args.max_notes)
    except RuntimeError as e:
        raise ValueError(f"--split: {e}")
    for f, c in zip(files, onsets.count.tolist()):
        if c > args.max_notes:
            warnings.warn(f"{f}: {c} onsets, the first {args.max_notes} are kept (--max-notes)")
    seg = split_notes(whole, lengths, onsets, T, int(round(args.fade_ms * 1e-3 * rate)))
    print(f"match_audio.py: {seg.audio.shape[0]} notes in {len(files)} files", flush=True)
    return seg, whole


def load_targets(args, files, rate, T, dev):
    """Read the files, with --resample at any rate and brought to ``rate`` on the device -> ``Targets``: one buffer of ``T``
    samples per file, cropped or zero-padded with a warning, or with --split one per note of the files read whole."""
    import torch
    plain = not (args.resample or args.split)            # then a file is refused or fitted as soon as it is read
    rows, in_rates, in_lengths = [], [], []
    for f in files:
        x, sr = read_wav_any_rate(f, rate if plain else None)
        rows.append(fit_length(x, T, f) if plain else x)
        in_rates.append(sr)
        in_lengths.append(len(x))
    if args.resample:
        rows = resample_rows(rows, in_rates, [rate] * len(files), dev)
        if not args.split:                               # the warnings come rate by rate, as the resampling goes
            for i in sorted(range(len(files)), key=lambda i: in_rates[i]):
                rows[i] = fit_length(rows[i].cpu().numpy(), T, f"{files[i]} (resampled {in_rates[i]} -> {rate} Hz)")
    elif args.split:
        for f, sr in zip(files, in_rates):
            _refuse_rate(f, sr, rate, "pass --resample or")
    if args.split:
        seg, whole = split_targets([torch.as_tensor(r).to(dev) for r in rows], files, rate, T, args)
        return Targets(seg.audio, in_rates, in_lengths, seg, whole)
    return Targets(torch.from_numpy(np.stack(rows)).to(dev), in_rates, in_lengths)


INITS = ("center", "random", "bank")
DEFAULT_OWN = "keyboard.midi_f0,keyboard.duration"   # ``match.DEFAULT_OWN`` as the flag spells it


def parse_own(text):
    """--own: "module.name,module.name,..." -> ((module, name), ...), each checked against ``voice_spec.PARAMS``
    (ValueError naming the unknown one).  An empty string: no own columns."""
    from inverse_audio_synthesis_amd import voice_spec as S
    own = []
    for item in (t.strip() for t in text.split(",") if t.strip()):
        key = tuple(item.split(".", 1))
        if key not in S.INDEX:
            raise ValueError(f"unknown Voice parameter {item!r} (module.name, as in NAME.params.json)")
        if key not in own:
            own.append(key)
    return tuple(own)
BANK_BATCH = 128
ENVELOPE_ELITES = 16                # ``envelope.fit_envelope``'s default


def parse_args(argv=None):
    """The command line -> (args, WAV files, config overrides); refusals exit through ``argparse`` (SystemExit 2)."""
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("inputs", nargs="+", help="WAV files (16/24/32-bit PCM) and key=value config overrides")
    ap.add_argument("--out", required=True, help="output directory")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--init", choices=INITS, default="center")
    ap.add_argument("--starts", type=int, default=1, help="starts per sound (--init random or bank; center: 1)")
    ap.add_argument("--bank-batches", type=int, default=32, help="--init bank: voice batches of 128 in the bank")
    ap.add_argument("--bank-stream", type=int, default=None, metavar="CHUNK",
                    help="--init bank: search the bank CHUNK batches at a time instead of keeping it in memory")
    ap.add_argument("--loss", choices=("mel_l1", "stft_l1", "multi_resolution_stft"), default="mel_l1")
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--beta1", type=float, default=0.9)
    ap.add_argument("--beta2", type=float, default=0.999)
    ap.add_argument("--eps", type=float, default=1e-8)
    ap.add_argument("--batch-size", type=int, default=128, help="sounds fitted at once (at most)")
    ap.add_argument("--seed", type=int, default=0, help="seed of --init random and of --evolve")
    ap.add_argument("--evolve", type=int, default=0, metavar="G",
                    help="generations of evolutionary search between the start and the fit (0: none)")
    ap.add_argument("--evolve-population", type=int, default=4 * BANK_BATCH, metavar="M",
                    help="--evolve: candidates per sound and generation, a multiple of 128")
    ap.add_argument("--evolve-elites", type=int, default=8, metavar="K", help="--evolve: elites kept per sound (1..64)")
    ap.add_argument("--evolve-sigma", type=float, default=0.2, metavar="S0",
                    help="--evolve: initial standard deviation of every free parameter")
    ap.add_argument("--resample", action="store_true",
                    help="read files at any rate and resample them to torchsynth.rate on the device; NAME.match.wav is "
                         "written at the input's rate")
    ap.add_argument("--pitch", action="store_true",
                    help="estimate each target's note and start keyboard.midi_f0 there (pitch.estimate_pitch / retune)")
    ap.add_argument("--pitch-lo", type=float, default=21.0, metavar="MIDI", help="--pitch: lowest note searched")
    ap.add_argument("--pitch-hi", type=float, default=108.0, metavar="MIDI", help="--pitch: highest note searched")
    ap.add_argument("--envelope", action="store_true",
                    help="fit the Voice's envelope law to each target's RMS envelope and start keyboard.duration and both "
                         "ADSRs there (envelope.fit_envelope / reshape)")
    ap.add_argument("--envelope-generations", type=int, default=16, metavar="G", help="--envelope: generations searched")
    ap.add_argument("--envelope-population", type=int, default=512, metavar="M",
                    help="--envelope: candidates per sound and generation (at least the 16 elites kept)")
    ap.add_argument("--split", action="store_true",
                    help="find the note onsets of every file and match it note by note (onset.detect_onsets / split_notes); "
                         "writes NAME.notes.json and a NAME.match.wav of the file's full length")
    ap.add_argument("--onset-delta", type=float, default=0.2, metavar="D",
                    help="--split: how far the spectral flux must rise above its moving mean at an onset")
    ap.add_argument("--max-notes", type=int, default=256, metavar="K", help="--split: notes kept per file")
    ap.add_argument("--fade-ms", type=float, default=5.0, metavar="MS",
                    help="--split: linear fade-out of a note that is cut by the next onset or by the synth buffer")
    ap.add_argument("--shared", action="store_true",
                    help="--split: fit the notes of a file to one shared preset (SoundMatcher.fit_tied); only the --own "
                         "columns differ from note to note; writes NAME.preset.json")
    ap.add_argument("--own", default=DEFAULT_OWN, metavar="M.N,M.N,...",
                    help="--shared: the parameters every note keeps for itself, as module.name")
    ap.add_argument("--gain", choices=("solved", "fitted"), default=None,
                    help="an output gain in dB per sound beside the 78 parameters: solved in closed form against the "
                         "start's render (solved) and then fitted by the same Adam step (fitted)")
    ap.add_argument("--report", action="store_true",
                    help="compare each best render with its target in loss-independent figures (report.Reporter) and "
                         "write them into every record and stdout line as `report`")
    args = ap.parse_args(argv)
    files = [a for a in args.inputs if "=" not in a]
    overrides = [a for a in args.inputs if "=" in a]
    if not files:
        ap.error("no input WAV files")
    if args.starts < 1:
        ap.error("--starts must be >= 1")
    if args.evolve < 0:
        ap.error("--evolve must be >= 0")
    if args.evolve_population < 1 or args.evolve_population % BANK_BATCH != 0:
        ap.error(f"--evolve-population must be a positive multiple of {BANK_BATCH}")
    if not 1 <= args.evolve_elites <= 64:
        ap.error("--evolve-elites must be in 1..64")
    if not 0.0 <= args.evolve_sigma < float("inf"):
        ap.error("--evolve-sigma must be finite and >= 0")
    if args.evolve > 0:
        if args.starts > args.evolve_elites:
            ap.error("--evolve: --starts must not exceed --evolve-elites")
        if args.evolve_population > (1 << 31) // args.evolve:
            ap.error("--evolve: --evolve-population x --evolve must not exceed 2^31")
    if args.init == "center" and args.starts != 1 and args.evolve == 0:
        ap.error("--init center has one start per sound: --starts must be 1")
    if not args.pitch_lo < args.pitch_hi:
        ap.error("--pitch-lo must be below --pitch-hi")
    if args.envelope_generations < 1:
        ap.error("--envelope-generations must be >= 1")
    if args.envelope_population < ENVELOPE_ELITES:
        ap.error(f"--envelope-population must be >= {ENVELOPE_ELITES}")
    if args.envelope_population > (1 << 31) // args.envelope_generations:
        ap.error("--envelope-population x --envelope-generations must not exceed 2^31")
    if not 0.0 < args.onset_delta < float("inf"):
        ap.error("--onset-delta must be finite and > 0")
    if args.max_notes < 1:
        ap.error("--max-notes must be >= 1")
    if not 0.0 <= args.fade_ms < float("inf"):
        ap.error("--fade-ms must be finite and >= 0")
    if args.bank_batches < 1:
        ap.error("--bank-batches must be >= 1")
    if args.bank_stream is not None:
        if args.init != "bank":
            ap.error("--bank-stream needs --init bank")
        if args.bank_stream < 1:
            ap.error("--bank-stream must be >= 1")
        if args.starts > 64:
            ap.error("--bank-stream keeps at most 64 starts per sound")
    if args.shared:
        if not args.split:
            ap.error("--shared needs --split")
        if args.starts > 1:
            ap.error("--shared fits one start per note: --starts must be 1" + (" (with --evolve too)" if args.evolve else ""))
    try:
        args.own = parse_own(args.own)
    except ValueError as e:
        ap.error(f"--own: {e}")
    return args, files, overrides


def search_stage(cfg, matcher, args, rate, dev):
    """-> (voice, loss) of --init bank and --evolve: a Voice of ``BANK_BATCH`` rows and the matcher's loss, or a mel loss
    (the ``mel.*`` settings) where that is multi_resolution_stft, which is not the L1 of one array."""
    from inverse_audio_synthesis_amd.spectral import MelSpectrogramL1
    from inverse_audio_synthesis_amd.voice import SynthConfig, Voice
    voice = Voice(SynthConfig(batch_size=BANK_BATCH, sample_rate=rate,
                              buffer_size_seconds=cfg.torchsynth.buffer_size_seconds,
                              reproducible=cfg.torchsynth.reproducible)).to(dev)
    if args.loss != "multi_resolution_stft":
        return voice, matcher.loss
    kw = dict(cfg.mel)
    kw.setdefault("sample_rate", rate)
    return voice, MelSpectrogramL1(**kw).to(dev)


def initial_starts(args, stage, target, prov):
    """--init -> the starts [N, 78] or [N, S, 78] (None: the centre); --init bank names its voices in ``prov``."""
    import torch
    N, nS = target.shape[0], args.starts
    if args.init == "random":
        init = torch.rand((N * nS, 78), generator=torch.Generator().manual_seed(args.seed)).to(target.device)
        return init.reshape(N, nS, 78) if nS > 1 else init
    if args.init != "bank":
        return None
    from inverse_audio_synthesis_amd.retrieval import SpectralBank
    voice, loss = stage
    if args.bank_stream is not None:
        chunk = min(args.bank_stream, args.bank_batches)
        nbytes = SpectralBank.nbytes(voice, loss, chunk)
        print(f"match_audio.py: searching a spectral bank of {args.bank_batches * BANK_BATCH} voices in chunks of "
              f"{chunk * BANK_BATCH} ({nbytes} bytes)", flush=True)
        dist, idx, init = SpectralBank.search(voice, loss, range(args.bank_batches), target_audio=target, k=nS,
                                              chunk_batches=chunk)
        prov.bank = (dist, idx)
        return init
    nbytes = SpectralBank.nbytes(voice, loss, args.bank_batches)
    print(f"match_audio.py: building a spectral bank of {args.bank_batches * BANK_BATCH} voices ({nbytes} bytes)",
          flush=True)
    bank = SpectralBank(voice, loss, range(args.bank_batches))
    prov.bank = bank.nearest(target_audio=target, k=nS)
    return bank.params01[prov.bank[1].reshape(-1)].reshape(N, -1, 78)


def written_out(init, target):
    """The starts as a tensor a stage can retune or reshape: ``init``, or with --init center (None) the centre matrix."""
    import torch
    if init is None:
        init = torch.full((target.shape[0], 78), 0.5, dtype=torch.float32, device=target.device)
    return init


def pitch_stage(args, target, rate, init, prov):
    """--pitch: estimate every target's note (``prov.pitch``) and move ``keyboard.midi_f0`` of its starts onto it."""
    from inverse_audio_synthesis_amd.pitch import estimate_pitch, retune
    try:
        prov.pitch = estimate_pitch(target, rate, midi_lo=args.pitch_lo, midi_hi=args.pitch_hi)
    except ValueError as e:
        sys.exit(f"match_audio.py: --pitch: {e}")
    return retune(written_out(init, target), prov.pitch)


def envelope_stage(args, target, rate, init, prov):
    """--envelope: fit every target's envelope (``prov.envelope``) and write it into its starts."""
    from inverse_audio_synthesis_amd.envelope import fit_envelope, reshape
    try:
        prov.envelope = fit_envelope(target, rate, generations=args.envelope_generations,
                                     population=args.envelope_population, elites=ENVELOPE_ELITES, seed=args.seed)
    except ValueError as e:
        sys.exit(f"match_audio.py: --envelope: {e}")
    return reshape(written_out(init, target), prov.envelope)


def evolve_stage(args, stage, target, init, prov):
    """--evolve: the search from ``init`` -> its --starts best elites as the starts; ``prov`` names them."""
    from inverse_audio_synthesis_amd.evolve import evolve_search
    print(f"match_audio.py: evolutionary search, {args.evolve} generations of {args.evolve_population} candidates per "
          f"sound, {args.evolve_elites} elites", flush=True)
    found = evolve_search(*stage, target_audio=target, generations=args.evolve, population=args.evolve_population,
                          elites=args.evolve_elites, init_params01=init, sigma0=args.evolve_sigma, seed=args.seed)
    nS = args.starts
    prov.evolve, prov.bank = (found.dist[:, :nS], found.idx[:, :nS]), None   # the kept start is no longer a bank voice
    return found.params01[:, :nS].contiguous() if nS > 1 else found.params01[:, 0].contiguous()


def shared_stage(args, matcher, tg, init):
    """--shared: score the notes' starts once under the matcher's loss, give every note of a file the best-scoring note's
    tied columns and fit each file's notes as one group -> (a ``MatchResult`` of the notes for their records, the
    ``shared`` block of every file)."""
    from inverse_audio_synthesis_amd import voice_spec as S
    from inverse_audio_synthesis_amd.match import MatchResult, tie_starts
    init = written_out(init, tg.audio)
    if init.dim() == 3:                              # --init bank: [N, 1, 78], the one start of every note
        init = init[:, 0].contiguous()
    tied = matcher.tied_mask(args.own)
    score = matcher.fit(tg.audio, init_params01=init, steps=0, gain=args.gain).loss     # --gain: ranked level-matched
    init = tie_starts(init, tg.seg.row, tied, score)
    res = matcher.fit_tied(tg.audio, tg.seg.row, init_params01=init, own=args.own, steps=args.steps, return_audio=True,
                           gain=args.gain)
    names = [f"{m}.{n}" for (m, n, *_r), t in zip(S.PARAMS, tied.tolist()) if t]
    shared = [{"tied": names, "own": [f"{m}.{n}" for m, n in args.own], "initial_group_loss": a, "group_loss": b}
              for a, b in zip(res.initial_group_loss.tolist(), res.group_loss.tolist())]
    rows = tg.seg.row.long()
    return MatchResult(params01=res.params01, loss=res.loss, initial_loss=res.initial_loss, skipped=res.skipped[rows],
                       audio=res.audio, gain_db=res.gain_db, initial_gain_db=res.initial_gain_db), shared


def preset_doc(name, shared, note):
    """NAME.preset.json: the tied parameters once, as the ``params_record`` rows of one of the file's notes."""
    tied = set(shared["tied"])
    return {"input": name, "shared": shared, "params": [p for p in note["params"] if f"{p['module']}.{p['name']}" in tied]}


def report_stage(cfg, rate, audio, target):
    """--report: the best renders against their targets -> one dict of ``report.MatchReport``'s fields per sound."""
    from inverse_audio_synthesis_amd.report import Reporter
    try:
        return Reporter(rate, mel_kwargs=dict(cfg.mel))(audio, target).as_records()
    except ValueError as e:
        sys.exit(f"match_audio.py: --report: {e}")


def record(args, res, prov, i, name, reports=None):
    """The fields of sound i's params.json record; with --report, ``reports[i]`` as ``report``."""
    rec = {"input": name, "loss_kind": args.loss, "steps": args.steps,
           "initial_loss": float(res.initial_loss[i]), "final_loss": float(res.loss[i]),
           "skipped": int(res.skipped[i]), "init": args.init, "params": params_record(res.params01[i])}
    if args.gain is not None:
        rec["gain_mode"] = args.gain
        rec["initial_gain_db"], rec["fit_gain_db"] = float(res.initial_gain_db[i]), float(res.gain_db[i])
    s = 0
    if res.start is not None:
        s = rec["start"] = int(res.start[i])
    if prov.bank is not None:
        rec["bank_index"], rec["bank_distance"] = int(prov.bank[1][i, s]), float(prov.bank[0][i, s])
    if prov.evolve is not None:
        rec["evolve_generations"], rec["evolve_population"] = args.evolve, args.evolve_population
        rec["evolve_index"], rec["evolve_distance"] = int(prov.evolve[1][i, s]), float(prov.evolve[0][i, s])
    if prov.pitch is not None:
        rec["voiced"] = bool(prov.pitch.voiced[i])
        rec["estimated_midi"] = float(prov.pitch.midi[i]) if rec["voiced"] else None
        rec["pitch_confidence"] = float(prov.pitch.confidence[i])
    if prov.envelope is not None:
        from inverse_audio_synthesis_amd.envelope import COLUMNS
        fit = prov.envelope
        rec["envelope"] = {"sounding": bool(fit.sounding[i]), "distance": float(fit.dist[i]),
                           "start_distance": float(fit.start_dist[i]),
                           **{name: float(v) for name, v in zip(COLUMNS, fit.units[i])}}
    if reports is not None:
        rec["report"] = reports[i]
    return rec


def file_docs(args, files, rate, tg, res, prov, reports=None):
    """-> (the best renders [files, T], NAME.params.json's content per file, its stdout line per file)."""
    docs = [record(args, res, prov, i, os.path.basename(f), reports) for i, f in enumerate(files)]
    if args.resample:
        for doc, sr in zip(docs, tg.in_rates):
            doc["input_rate"], doc["synth_rate"] = int(sr), rate
    keys = ("input", "initial_loss", "final_loss") + (("report",) if reports is not None else ())
    return res.audio, docs, [{key: doc[key] for key in keys} for doc in docs]


def notes_docs(args, files, rate, tg, res, prov, reports=None, shared=None):
    """--split -> (the recordings [files, L] put together from the best renders, NAME.notes.json's content per file, its
    stdout line per file); with --shared, ``shared[i]`` as file i's ``shared``."""
    from inverse_audio_synthesis_amd.onset import join_notes, note_gains
    seg = tg.seg
    gain = note_gains(seg.audio, res.audio, seg.length)
    joined = join_notes(res.audio.contiguous(), seg, tg.whole.shape[0], tg.whole.shape[1], gain)
    rows, starts, lengths = seg.row.tolist(), seg.start.tolist(), seg.length.tolist()
    gains, strengths = gain.tolist(), seg.strength.tolist()
    docs = []
    for i, f in enumerate(files):
        notes = []
        for s in [s for s, r in enumerate(rows) if r == i]:
            note = {"onset_sample": starts[s], "onset_seconds": starts[s] / rate, "length_samples": lengths[s],
                    "strength": strengths[s], "gain": gains[s]}
            note.update(record(args, res, prov, s, os.path.basename(f), reports))
            notes.append(note)
        docs.append({"input": os.path.basename(f), "rate": rate, "notes": notes})
        if args.resample:
            docs[i]["input_rate"] = int(tg.in_rates[i])
        if shared is not None:
            docs[i]["shared"] = shared[i]
    lines = [{"input": doc["input"], "notes": len(doc["notes"]), "final_loss": [n["final_loss"] for n in doc["notes"]]}
             for doc in docs]
    if shared is not None:
        for line, block in zip(lines, shared):
            line["group_loss"] = block["group_loss"]
    if reports is not None:
        for line, doc in zip(lines, docs):
            line["report"] = [n["report"] for n in doc["notes"]]
    return joined, docs, lines


def write_outputs(args, files, rate, tg, audio, docs, lines):
    """Per input NAME: ``docs[i]`` as NAME.notes.json (--split) or NAME.params.json, row i of audio [files, L] (on the
    device, at ``rate``) as NAME.match.wav, with --resample at the file's own rate, and ``lines[i]`` to stdout."""
    if args.resample:
        host = [y.cpu().numpy() for y in resample_rows(list(audio), [rate] * len(files), tg.in_rates, audio.device)]
    else:
        host = audio.cpu().numpy()
    for i, f in enumerate(files):
        name = os.path.splitext(os.path.basename(f))[0]
        with open(os.path.join(args.out, name + (".notes.json" if args.split else ".params.json")), "w") as fh:
            json.dump(docs[i], fh, indent=1)
        if args.shared:
            with open(os.path.join(args.out, name + ".preset.json"), "w") as fh:
                json.dump(preset_doc(docs[i]["input"], docs[i]["shared"], docs[i]["notes"][0]), fh, indent=1)
        x = fit_length(host[i], tg.in_lengths[i], None) if args.split else host[i]
        write_wav(os.path.join(args.out, name + ".match.wav"), x, tg.in_rates[i])
        print(json.dumps(lines[i]), flush=True)


def main(argv=None):
    args, files, overrides = parse_args(argv)

    import torch
    from inverse_audio_synthesis_amd.config import load_config
    from inverse_audio_synthesis_amd.match import SoundMatcher
    from inverse_audio_synthesis_amd.voice import SynthConfig, Voice
    cfg = load_config(os.path.join(ROOT, "conf"), "config", overrides)
    rate = int(cfg.torchsynth.rate)
    dev = torch.device("cuda:0")
    synth = dict(sample_rate=rate, buffer_size_seconds=cfg.torchsynth.buffer_size_seconds,
                 reproducible=cfg.torchsynth.reproducible)
    try:
        tg = load_targets(args, files, rate, SynthConfig(batch_size=1, **synth).buffer_size, dev)
        N = tg.audio.shape[0]                            # with --split the notes are the sounds: the Voice is built now
        voice = Voice(SynthConfig(batch_size=max(1, min(N * args.starts, int(args.batch_size))), **synth)).to(dev)
    except ValueError as e:
        sys.exit(f"match_audio.py: {e}")
    matcher = SoundMatcher(voice, loss=args.loss, mel_kwargs=dict(cfg.mel), lr=args.lr, betas=(args.beta1, args.beta2),
                           eps=args.eps)
    stage = search_stage(cfg, matcher, args, rate, dev) if args.init == "bank" or args.evolve > 0 else None
    prov = Provenance()
    init = initial_starts(args, stage, tg.audio, prov)
    if args.pitch:
        init = pitch_stage(args, tg.audio, rate, init, prov)
    if args.envelope:
        init = envelope_stage(args, tg.audio, rate, init, prov)
    if args.evolve > 0:
        init = evolve_stage(args, stage, tg.audio, init, prov)
    shared = None
    if args.shared:
        res, shared = shared_stage(args, matcher, tg, init)
    else:
        res = matcher.fit(tg.audio, init_params01=init, steps=args.steps, return_audio=True, gain=args.gain)
    os.makedirs(args.out, exist_ok=True)
    reports = report_stage(cfg, rate, res.audio, tg.audio) if args.report else None
    if args.split:
        audio, docs, lines = notes_docs(args, files, rate, tg, res, prov, reports, shared)
    else:
        audio, docs, lines = file_docs(args, files, rate, tg, res, prov, reports)
    write_outputs(args, files, rate, tg, audio, docs, lines)


if __name__ == "__main__":
    main()

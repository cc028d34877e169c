"""What the stage benchmarks (scripts/bench_*.py) share, so that their figures are comparable by construction: the event
timer, the child-process runner, the loss summary and the 16-target experiment of DESIGN.md section 4.6.  Not a benchmark
itself; ``bench.py`` does not use it."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MEL = dict(n_fft=1024, hop_length=512, n_mels=128, power=2.0)
TARGETS, TARGET_SEED, BANK_BATCHES, STARTS, FIT_STEPS = 16, 10_000, 32, 4, 200


def event_ms(fn, reps, passes=1):
    """Time a launch by device events: one call first (tables, allocations), then ``passes`` windows of ``reps`` calls
    between two events -> the ms per call of every window."""
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(passes):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return out


def spread(times, scale=1.0, digits=2):
    """Times of several windows -> {min, median, max}, each times ``scale`` and rounded."""
    return {"min": round(min(times) * scale, digits), "median": round(statistics.median(times) * scale, digits),
            "max": round(max(times) * scale, digits)}


def json_line(cmd):
    """Run a benchmark of the project in a process of its own -> the last JSON line it printed."""
    r = subprocess.run([sys.executable] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or not lines:
        raise RuntimeError(f"{' '.join(cmd)} failed:\n{r.stdout[-2000:]}")
    return json.loads(lines[-1])


def rounded(xs, digits=4):
    return [round(float(x), digits) for x in xs]


def loss_summary(loss, every="all"):
    """Final losses [N] -> their median, best and worst, and all of them under the key ``every``."""
    return {"median": round(float(loss.median()), 4), "best": round(float(loss.min()), 4),
            "worst": round(float(loss.max()), 4), every: rounded(loss)}


# ------------------------------------------------------------------ the experiment of DESIGN.md section 4.6
def design_voice(dev):
    """The 128-row Voice of 4 s @ 44.1 kHz every stage is timed on."""
    from inverse_audio_synthesis_amd.voice import SynthConfig, Voice
    return Voice(SynthConfig(batch_size=128, sample_rate=44100, buffer_size_seconds=4.0, reproducible=False)).to(dev)


def mel_matcher(voice):
    from inverse_audio_synthesis_amd.match import SoundMatcher
    return SoundMatcher(voice, loss="mel_l1", mel_kwargs=MEL)


def target_params01():
    """[16, 78] on the host: the parameters of the 16 targets, the first rows of the draw of seed 10 000 (in no bank)."""
    import torch
    return torch.rand((128, 78), generator=torch.Generator().manual_seed(TARGET_SEED))[:TARGETS]


def targets(voice):
    """[16, T]: the 16 targets, rendered in their own rows of the whole draw."""
    import torch
    draw = torch.rand((128, 78), generator=torch.Generator().manual_seed(TARGET_SEED))
    return voice.render(draw.to(voice.params01.device))[:TARGETS].contiguous()


def nearest_starts(bank, tgt, k=STARTS):
    """-> (dist [16, k], the parameters [16, k, 78]) of the k nearest voices of a resident ``SpectralBank``; the
    experiment's bank is ``SpectralBank(voice, matcher.loss, range(BANK_BATCHES))``: 4 096 voices."""
    d, idx = bank.nearest(target_audio=tgt, k=k)
    return d, bank.params01[idx.reshape(-1)].reshape(tgt.shape[0], k, 78)


def fit_starts(matcher, tgt, starts, pairs=(), steps=FIT_STEPS, every="all"):
    """Fit every entry of ``starts`` (name -> init_params01 [16, 78] or [16, S, 78]; None: the centre) for ``steps`` Adam
    steps -> (the ``MatchResult`` per name, a dict with the ``loss_summary`` per name and, per pair (a, b), how many
    targets b ends below (``b_wins``) and above (``b_losses``) a)."""
    fits = {name: matcher.fit(tgt, init_params01=init, steps=steps) for name, init in starts.items()}
    q = {name: loss_summary(res.loss.cpu(), every) for name, res in fits.items()}
    for a, b in pairs:
        q[b + "_wins"] = int((fits[b].loss < fits[a].loss).sum())
        q[b + "_losses"] = int((fits[b].loss > fits[a].loss).sum())
    return fits, q

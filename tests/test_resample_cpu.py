"""Band-limited resampler without a GPU: the C ABI's host side (plan, filter table, output length, refusals), the Python
mirror's refusals and match_audio.py's 24-bit reading and --resample flag.  The fp64 restatement of torchaudio's
formula below is also the reference of tests/test_resample_gpu.py."""
import ctypes
import math
import wave

import numpy as np
import pytest
import torch

import match_audio as ma

KAISER_BETA = 14.769656459379492
# orig -> new: (o, n, K)
RATIOS = {(48000, 44100): (160, 147, 174), (44100, 48000): (147, 160, 161), (96000, 44100): (320, 147, 348),
          (192000, 44100): (640, 147, 694), (32000, 44100): (320, 441, 334), (16000, 44100): (160, 441, 174),
          (22050, 44100): (1, 2, 15), (88200, 44100): (2, 1, 28)}


def ref_plan(orig, new, lowpass_filter_width=6, rolloff=0.99):
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * rolloff
    width = math.ceil(lowpass_filter_width * o / base)
    return o, n, width, 2 * width + o


def ref_taps(orig, new, lowpass_filter_width=6, rolloff=0.99, method="hann", beta=KAISER_BETA):
    """[n, K] fp64: torchaudio's _get_sinc_resample_kernel restated in numpy."""
    o, n, width, K = ref_plan(orig, new, lowpass_filter_width, rolloff)
    base, w = min(o, n) * rolloff, float(lowpass_filter_width)
    i, j = np.arange(K, dtype=np.float64), np.arange(n, dtype=np.float64)
    t = np.clip(((i[None, :] - width) / o - j[:, None] / n) * base, -w, w)
    if method == "hann":
        win = np.cos(t * np.pi / w / 2) ** 2
    else:
        win = np.i0(beta * np.sqrt(1 - (t / w) ** 2)) / np.i0(beta)
    t = t * np.pi
    k = np.where(t == 0, 1.0, np.sin(t) / np.where(t == 0, 1.0, t))
    return k * (win * (base / o))


def ref_resample(x, orig, new, **kw):
    """x [B, T] -> [B, ceil(n T / o)] fp64: the padded strided correlation of torchaudio's _apply_sinc_resample_kernel."""
    o, n, width, K = ref_plan(orig, new, kw.get("lowpass_filter_width", 6), kw.get("rolloff", 0.99))
    taps = ref_taps(orig, new, **kw)
    x = np.asarray(x, dtype=np.float64)
    B, T = x.shape
    xp = np.concatenate([np.zeros((B, width)), x, np.zeros((B, width + o))], axis=1)
    nb = T // o + 1
    idx = np.arange(nb)[:, None] * o + np.arange(K)[None, :]
    y = np.einsum("bqi,ji->bqj", xp[:, idx], taps).reshape(B, nb * n)
    return y[:, :-(-n * T // o)]


def _method(name):
    return {"hann": 0, "kaiser": 1}[name]


def _plan(lib, orig, new, lw=6, rolloff=0.99, method=0, beta=KAISER_BETA):
    plan = (ctypes.c_int * 4)()
    st = lib.ias_resample_plan(orig, new, lw, rolloff, method, beta, plan)
    return st, tuple(plan)


def _taps(lib, orig, new, lw=6, rolloff=0.99, method="hann", beta=KAISER_BETA):
    st, (o, n, width, K) = _plan(lib, orig, new, lw, rolloff, _method(method), beta)
    assert st == 0
    out = np.empty((n, K), dtype=np.float32)
    ptr = out.ctypes.data_as(ctypes.c_void_p)
    assert lib.ias_resample_build_taps(orig, new, lw, rolloff, _method(method), beta, ptr) == 0
    return out


@pytest.mark.parametrize("ratio", list(RATIOS), ids=[f"{a}-{b}" for a, b in RATIOS])
def test_plan_matches_the_table(lib, ratio):
    st, plan = _plan(lib, *ratio)
    assert st == 0
    o, n, K = RATIOS[ratio]
    assert plan == ref_plan(*ratio)
    assert (plan[0], plan[1], plan[3]) == (o, n, K)
    assert plan[3] == 2 * plan[2] + plan[0]


def test_plan_table_sizes():
    # the issue's table: 48k -> 44.1k is 100 KB, 32k -> 44.1k 575 KB, 22.05k -> 44.1k 0.1 KB
    sizes = {r: 4 * n * K for r, (o, n, K) in RATIOS.items()}
    assert sizes[(48000, 44100)] == 102312 and sizes[(32000, 44100)] == 589176 and sizes[(22050, 44100)] == 120


@pytest.mark.parametrize("method", ["hann", "kaiser"])
@pytest.mark.parametrize("ratio,lw,rolloff", [(r, 6, 0.99) for r in RATIOS] + [((48000, 44100), 3, 0.9),
                                                                                ((44100, 16000), 10, 0.95),
                                                                                ((16000, 48000), 4, 1.0)])
def test_taps_match_fp64_restatement(lib, method, ratio, lw, rolloff):
    got = _taps(lib, *ratio, lw=lw, rolloff=rolloff, method=method)
    ref = ref_taps(*ratio, lowpass_filter_width=lw, rolloff=rolloff, method=method)
    assert got.shape == ref.shape
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= 2 * ulp).all(), float((err / ulp).max())


def test_kaiser_beta_changes_the_table(lib):
    a = _taps(lib, 48000, 44100, method="kaiser")
    b = _taps(lib, 48000, 44100, method="kaiser", beta=8.0)
    assert not np.array_equal(a, b)
    assert np.allclose(b, ref_taps(48000, 44100, method="kaiser", beta=8.0), rtol=0, atol=1e-7)


def test_refusals(lib):
    ARG, UNSUP = -1, -2
    for orig, new in ((0, 44100), (44100, 0), (-48000, 44100), (48000, -1)):
        assert _plan(lib, orig, new)[0] == ARG, (orig, new)
    for lw in (0, -6):
        assert _plan(lib, 48000, 44100, lw=lw)[0] == ARG
    for rolloff in (0.0, -0.5, 1.0001, math.nan, math.inf):
        assert _plan(lib, 48000, 44100, rolloff=rolloff)[0] == ARG, rolloff
    assert _plan(lib, 48000, 44100, rolloff=1.0)[0] == 0
    assert _plan(lib, 48000, 44100, method=2)[0] == ARG
    assert _plan(lib, 48000, 44100, method=1, beta=math.nan)[0] == ARG
    assert _plan(lib, 48000, 44100, method=0, beta=math.nan)[0] == 0           # Hann ignores beta
    # 44100 -> 44101 reduces to o = 44100, n = 44101: a 1.9e9-tap table, over the 16 Mi cap
    assert _plan(lib, 44100, 44101)[0] == UNSUP
    assert lib.ias_resample_build_taps(44100, 44101, 6, 0.99, 0, 0.0, ctypes.c_void_p(8)) == UNSUP
    assert lib.ias_resample_build_taps(48000, 44100, 6, 0.99, 0, 0.0, None) == ARG
    # the device entry point refuses before launching anything (no GPU is touched here)
    fake = ctypes.c_void_p(16)
    assert lib.ias_resample(None, fake, fake, 1, 100, 160, 147, 7, 174, None) == ARG
    assert lib.ias_resample(fake, fake, fake, 0, 100, 160, 147, 7, 174, None) == ARG
    assert lib.ias_resample(fake, fake, fake, 1, 0, 160, 147, 7, 174, None) == ARG
    assert lib.ias_resample(fake, fake, fake, 1, 100, 160, 147, 7, 175, None) == ARG       # K != 2 width + o
    assert lib.ias_resample(fake, fake, fake, 70000, 100, 160, 147, 7, 174, None) == UNSUP
    assert lib.ias_resample(fake, fake, fake, 1, 100, 44100, 44101, 7, 44114, None) == UNSUP


def test_output_length(lib):
    for T in (1, 2, 159, 160, 161, 173, 174, 1000, 192000, 176399, 2 ** 31 - 1):
        for o, n in ((160, 147), (147, 160), (1, 2), (2, 1), (640, 147), (320, 441)):
            assert lib.ias_resample_out_len(T, o, n) == -(-n * T // o), (T, o, n)
    assert lib.ias_resample_out_len(1, 160, 147) == 1
    assert lib.ias_resample_out_len(173, 160, 147) == 159               # T < K
    assert lib.ias_resample_out_len(192000, 160, 147) == 176400
    assert lib.ias_resample_out_len(0, 160, 147) < 0 and lib.ias_resample_out_len(5, 0, 1) < 0


def test_reference_restatement_shapes():
    x = np.random.default_rng(0).uniform(-1, 1, (2, 173))
    assert ref_resample(x, 48000, 44100).shape == (2, 159)
    assert ref_resample(x[:, :1], 48000, 44100).shape == (2, 1)


def test_python_mirror_refusals(lib):
    from inverse_audio_synthesis_amd.resample import Resample, resample, resample_plan
    assert resample_plan(48000, 44100) == (160, 147, 7, 174)
    assert resample_plan(48000.0, 44100, resampling_method="kaiser_window") == (160, 147, 7, 174)
    with pytest.raises(RuntimeError, match="ROCm device"):
        resample(torch.zeros(2, 100), 48000, 44100)
    with pytest.raises(RuntimeError, match="ROCm device"):
        Resample(48000, 44100)(torch.zeros(100))
    with pytest.raises(ValueError, match="Invalid resampling method"):
        resample(torch.zeros(100), 48000, 44100, resampling_method="linear")
    with pytest.raises(ValueError, match="integer"):
        resample(torch.zeros(100), 44100.5, 48000)
    with pytest.raises(ValueError, match="positive"):
        resample_plan(0, 48000)
    with pytest.raises(RuntimeError, match="IAS_ERR_UNSUPPORTED"):
        resample_plan(44100, 44101)
    with pytest.raises(RuntimeError, match="IAS_ERR_ARG"):
        resample_plan(48000, 44100, rolloff=1.5)
    m = Resample(48000, 44100, resampling_method="sinc_interp_kaiser")
    assert tuple(m.kernel.shape) == (147, 174) and m.kernel.dtype == torch.float32


def _write_24(path, frames, sr):
    v = np.asarray(frames, dtype=np.int64)
    u = (v & 0xFFFFFF).astype(np.uint32)
    raw = np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=-1).astype(np.uint8)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(v.shape[1])
        w.setsampwidth(3)
        w.setframerate(sr)
        w.writeframes(raw.tobytes())


def test_read_wav_24_bit(tmp_path):
    mono = np.array([[0], [1], [-1], [2 ** 23 - 1], [-2 ** 23], [4096], [-123456]])
    _write_24(tmp_path / "m.wav", mono, 44100)
    x = ma.read_wav(str(tmp_path / "m.wav"), 44100)
    assert x.dtype == np.float32
    assert np.array_equal(x, (mono[:, 0] / 2.0 ** 23).astype(np.float32))
    stereo = np.array([[2 ** 22, -2 ** 22], [100, 300], [-2 ** 23, 2 ** 23 - 1], [7, 8]])
    _write_24(tmp_path / "s.wav", stereo, 48000)
    x, sr = ma.read_wav_any_rate(str(tmp_path / "s.wav"))
    assert sr == 48000
    assert np.array_equal(x, (stereo.astype(np.float64) / 2.0 ** 23).mean(axis=1).astype(np.float32))
    with pytest.raises(ValueError, match="48000 Hz.*44100 Hz"):
        ma.read_wav(str(tmp_path / "s.wav"), 44100)


def test_match_audio_accepts_resample():
    args, files, overrides = ma.parse_args(["a.wav", "b.wav", "torchsynth.rate=16000", "--out", "o", "--resample"])
    assert args.resample and files == ["a.wav", "b.wav"] and overrides == ["torchsynth.rate=16000"]
    args, _f, _o = ma.parse_args(["a.wav", "--out", "o"])
    assert not args.resample

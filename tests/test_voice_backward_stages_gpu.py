"""The two staged entry points of the Voice backward at the C level: ``ias_voice_backward`` (audio rate) and
``ias_voice_control_backward_ws`` (control rate) take a leading ``stage``; stage 0 followed by stage 1 on the same
buffers launches the kernels of stage -1 on the same buffers, so every output must be the same bits.  The scratch and
output buffers hold 0xFF bytes in the run that does everything at once and zeros in the staged run: a stage that read
what it did not write would show up as a difference.

Shapes (GRAD_TILE = 4096, sample rate 44100, control rate 441, T = 8200: three tiles, the last one ragged), one per
branch of ias_voice_backward, scale = (Tc - 1) / (T - 1):
* Tc = 83: scale * 16 = 0.16 <= 1, kslots = int(scale * 4096) + 3 = 43, 3 * 5 * 43 * 16 + 8 = 10328 <= 4 T = 32800: the
  lane-consecutive ("fold") form;
* Tc = 400: scale * 16 = 0.78 <= 1, kslots = 202, 3 * 5 * 202 * 16 + 8 = 48488 > 32800: not the fold form;
  nint = min(40, int(4608 / (8199 / 399 + 2)) - 1) = 40 >= 1 and 5 * 400 * 16 + 8 = 32008 <= 32800: the first form."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

B, SR, T = 2, 44100, 8200
OK, ARG = 0, -1


def _voice(dev, sec):
    from inverse_audio_synthesis_amd.voice import SynthConfig, Voice
    return Voice(SynthConfig(batch_size=B, sample_rate=SR, buffer_size_seconds=sec, reproducible=False)).to(dev)


@functools.lru_cache(maxsize=None)
def _inputs(dev, Tc):
    """Everything the audio-rate adjoint reads, computed once per Tc and left unchanged: the control signals of the
    seeded parameters at Tc control points, the noise and a cotangent at T samples, and the rownorm of a render whose
    peaks exceed 1."""
    from inverse_audio_synthesis_amd.voice_grad import normalisation_rows
    p = torch.rand(B, 78, generator=torch.Generator().manual_seed(162)).to(dev)    # (row peaks of the mix: 2.80, 1.58)
    vc = _voice(dev, (Tc + 0.5) / 441.0)
    assert vc.synthconfig.control_buffer_size == Tc
    ctrl, vconst = vc.control_signals(p)
    va = _voice(dev, (T + 0.5) / SR)
    assert va.synthconfig.buffer_size == T
    audio = va.render(p)
    peaks = va.read_peaks()
    assert (peaks > 1.0).all(), peaks.tolist()
    g = torch.randn(B, T, generator=torch.Generator().manual_seed(18)).to(dev)
    return dict(p=p, ctrl=ctrl, vconst=vconst, noise=va.noise, g=g, rownorm=normalisation_rows(g, audio, peaks))


def _audio_rate(lib, dev, Tc, rownorm, staged):
    """-> (status, partials, g_ctrl, g_scal); scratch and outputs start as 0xFF bytes (all at once) or zeros (staged)."""
    from inverse_audio_synthesis_amd._lib import ptr, stream
    x = _inputs(dev, Tc)
    ntiles, ns = lib.ias_voice_grad_tiles(T), lib.ias_voice_grad_nscalars()

    def buf(shape, dtype):
        t = torch.empty(shape, dtype=dtype, device=dev)
        t.view(torch.uint8).fill_(0 if staged else 0xFF)
        return t

    planes, tile_sums = buf((B, lib.ias_voice_grad_nplanes(), T), torch.float32), buf((B, ntiles, 2), torch.float64)
    partials, g_ctrl, g_scal = buf((B, ntiles, ns), torch.float64), buf((B, 5, Tc), torch.float32), buf((B, ns), torch.float64)
    tail = (B, T, Tc, SR, stream())
    full = (ptr(x["ctrl"]), ptr(x["vconst"]), ptr(x["noise"]), ptr(x["g"]), ptr(rownorm), ptr(planes), ptr(tile_sums),
            ptr(partials), ptr(g_ctrl), ptr(g_scal)) + tail
    if staged:      # stage 0 sees no cotangent: NULL for everything on that side
        st = lib.ias_voice_backward(0, ptr(x["ctrl"]), ptr(x["vconst"]), None, None, None, ptr(planes), ptr(tile_sums), None,
                                    None, None, *tail)
        assert st == OK
        st = lib.ias_voice_backward(1, *full)
    else:
        st = lib.ias_voice_backward(-1, *full)
    torch.cuda.synchronize()
    return st, partials, g_ctrl, g_scal


@pytest.mark.parametrize("with_rownorm", [False, True])
@pytest.mark.parametrize("Tc", [83, 400])
def test_audio_rate_stage_0_then_1_equals_stage_minus_1(lib, dev, Tc, with_rownorm):
    rownorm = _inputs(dev, Tc)["rownorm"] if with_rownorm else None
    st, *whole = _audio_rate(lib, dev, Tc, rownorm, staged=False)
    assert st == OK
    st, *halves = _audio_rate(lib, dev, Tc, rownorm, staged=True)
    assert st == OK
    for name, a, b in zip(("partials", "g_ctrl", "g_scal"), whole, halves):
        assert torch.equal(a, b), (name, (a != b).sum().item())


@pytest.mark.parametrize("Tc", [83, 400])
def test_control_rate_stage_0_then_1_equals_stage_minus_1(lib, dev, Tc):
    from inverse_audio_synthesis_amd._lib import ptr, stream
    p = _inputs(dev, Tc)["p"]
    st, _, g_ctrl, g_scal = _audio_rate(lib, dev, Tc, None, staged=False)
    assert st == OK
    nws = int(lib.ias_voice_control_backward_ws_bytes(B, Tc))
    outs = []
    for staged in (False, True):
        ws = torch.full((nws,), 0 if staged else 0xFF, dtype=torch.uint8, device=dev)
        out = torch.empty(B, 78, device=dev)
        out.view(torch.uint8).fill_(0 if staged else 0xFF)
        tail = (ptr(ws), nws, B, Tc, 441, stream())
        if staged:
            assert lib.ias_voice_control_backward_ws(0, ptr(p), None, None, None, *tail) == OK
        st = lib.ias_voice_control_backward_ws(1 if staged else -1, ptr(p), ptr(g_ctrl), ptr(g_scal), ptr(out), *tail)
        assert st == OK
        torch.cuda.synchronize()
        outs.append(out)
    assert torch.equal(outs[0], outs[1]), (outs[0] != outs[1]).sum().item()


def test_a_stage_other_than_minus_1_0_1_is_an_argument_error(lib, dev):
    from inverse_audio_synthesis_amd._lib import ptr, stream
    Tc = 83
    x = _inputs(dev, Tc)
    ntiles, ns = lib.ias_voice_grad_tiles(T), lib.ias_voice_grad_nscalars()
    planes = torch.zeros(B, lib.ias_voice_grad_nplanes(), T, device=dev)
    tile_sums, partials = (torch.zeros(B, ntiles, n, dtype=torch.float64, device=dev) for n in (2, ns))
    g_ctrl, g_scal = torch.zeros(B, 5, Tc, device=dev), torch.zeros(B, ns, dtype=torch.float64, device=dev)
    ws = torch.zeros(int(lib.ias_voice_control_backward_ws_bytes(B, Tc)), dtype=torch.uint8, device=dev)
    out = torch.zeros(B, 78, device=dev)
    for stage in (-2, 2):
        assert lib.ias_voice_backward(stage, ptr(x["ctrl"]), ptr(x["vconst"]), ptr(x["noise"]), ptr(x["g"]), None, ptr(planes),
                                      ptr(tile_sums), ptr(partials), ptr(g_ctrl), ptr(g_scal), B, T, Tc, SR, stream()) == ARG
        assert lib.ias_voice_control_backward_ws(stage, ptr(x["p"]), ptr(g_ctrl), ptr(g_scal), ptr(out), ptr(ws), ws.numel(),
                                                 B, Tc, 441, stream()) == ARG

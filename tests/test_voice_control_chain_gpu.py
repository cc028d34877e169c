"""The control pass as two launches (csrc/voice_ctrl_kernels.hip: voice_chain_slim_kernel -- one workgroup per LFO with its
whole chain, the two envelope rows it reads kept in LDS, and one per audio ADSR -- and voice_modmix_slim_kernel): every output
word against two references, bit for bit (torch.equal on the int32 views, so the sign of a zero counts):

  * the diagnostic library's IAS_VOICE_CTRL=libm form (the round-1 kernels on the device math library), and
  * the oracle's control signals on the CPU (math "cr").  Where the oracle has a NaN (every parameter 0: the LFO shape
    weights are 0 / 0) the kernels must have one too; which NaN a host's 0 / 0 gives (x86: the negative one) is not part of
    the contract, so against the oracle NaNs are compared by position and every other word by its bits.  Against the libm form
    NaNs are compared by their bits as well.

Outputs: ctrl [B,5,Tc], vconst [B,16], the eight intermediate rows, the ten debug rows when requested.  The oracle's control
pass defines eleven of vconst's twelve used words; kpart (pi x the partials constant of the audio half, which the oracle never
forms as one fp32 number) and the four pad words are compared with the libm form only.

Shapes: the smallest at which the indexing can go wrong -- Tc = 2 (the minimum), 163 (less than one 64-point chunk per wave
of the scan, not a multiple of 64), 441 (the envelope loops' second trip is ragged), 1025 (one point past four full trips and
past four mod-matrix workgroups), 1764 (the headline's) at B = 3, 4096 (the limit of this form; its 68 KB of LDS need the
attribute) at B = 2, 4097 (the round-1 kernels take over).  All at 16 kHz, so the workspaces stay small; only the control pass runs."""
import pytest
import torch

from oracle import synth_oracle as so
from oracle import synth_spec as S

pytestmark = pytest.mark.gpu

CONTROL_RATE = 441
SHAPES = [(3, 2), (3, 163), (3, 441), (3, 1025), (3, 1764), (2, 4096), (2, 4097)]        # (B, Tc)
PARAM_SETS = ["seed0", "seed1", "zeros", "ones", "short_key"]
ADSRS = ("adsr_1", "adsr_2", "lfo_1_amp_adsr", "lfo_2_amp_adsr", "lfo_1_rate_adsr", "lfo_2_rate_adsr")


def _params(kind, B):
    if kind == "zeros":         # log2(0) in every curve, zero durations against eps, saturated ramps
        return torch.zeros(B, S.NPARAMS)
    if kind == "ones":
        return torch.ones(B, S.NPARAMS)
    p = torch.rand(B, S.NPARAMS, generator=torch.Generator().manual_seed({"seed0": 100, "seed1": 101, "short_key": 102}[kind]))
    if kind == "short_key":     # the key is released inside every attack: new_attack = note_on, new_decay = 0
        p[:, S.INDEX[("keyboard", "duration")]] = 0.02
        for mod in ADSRS:
            p[:, S.INDEX[(mod, "attack")]] = torch.linspace(0.7, 1.0, B)
        for i, (_mod, _name, _lo, _hi, _curve, sym) in enumerate(S.PARAMS):
            if sym:             # voice 0: the centre of every symmetric range (dist == 0)
                p[0, i] = 0.5
    return p


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _same_values(a, b):
    """bit equality except that any NaN equals any NaN"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(_bits(a)[~na], _bits(b)[~nb])


@pytest.fixture(scope="module")
def diag():
    from inverse_audio_synthesis_amd import _lib
    return _lib.load_diag()


def _control(l, params, B, Tc, dev, with_dbg=True):
    """ias_voice_control of library ``l`` -> (ctrl, vconst, rows, dbg or None) on the CPU; buffers start as NaN"""
    from inverse_audio_synthesis_amd import _lib
    nan = float("nan")
    ctrl = torch.full((B, 5, Tc), nan, device=dev)
    vconst = torch.full((B, 16), nan, device=dev)
    rows = torch.full((B, 8, Tc), nan, device=dev)
    dbg = torch.full((B, 10, Tc), nan, device=dev) if with_dbg else None
    _lib.check(l.ias_voice_control(_lib.ptr(params), _lib.ptr(ctrl), _lib.ptr(vconst), _lib.ptr(rows), _lib.ptr(dbg), B, Tc,
                                   CONTROL_RATE, _lib.stream()), "ias_voice_control")
    torch.cuda.synchronize()
    return ctrl.cpu(), vconst.cpu(), rows.cpu(), (dbg.cpu() if with_dbg else None)


def _oracle_vconst(p):
    """IasVoiceConst words 0-5 and 7-11 from the oracle's mapped parameters (fp32 operations as voice_math.h states them)"""
    midi_f0, shape = p("keyboard", "midi_f0"), p("vco_2", "shape")
    return torch.stack([midi_f0 + p("vco_1", "tuning"), p("vco_1", "mod_depth"), p("vco_1", "initial_phase"),
                        midi_f0 + p("vco_2", "tuning"), p("vco_2", "mod_depth"), p("vco_2", "initial_phase"), shape,
                        1.0 - shape / 2.0, p("mixer", "vco_1"), p("mixer", "vco_2"), p("mixer", "noise")], dim=1).float()


@pytest.mark.parametrize("kind", PARAM_SETS)
@pytest.mark.parametrize("B,Tc", SHAPES)
def test_control_chain_equals_the_library_form_and_the_oracle(lib, diag, dev, monkeypatch, B, Tc, kind):
    from inverse_audio_synthesis_amd.voice import SynthConfig, Voice
    sec = (Tc + 0.5) / CONTROL_RATE
    v = Voice(SynthConfig(batch_size=B, sample_rate=16000, buffer_size_seconds=sec, reproducible=False)).to(dev)
    assert v.synthconfig.control_buffer_size == Tc
    p_cpu = _params(kind, B)
    params = p_cpu.to(dev)

    got = _control(lib, params, B, Tc, dev)
    names = ("ctrl", "vconst", "rows", "debug rows")
    # without the debug rows the other three are the same words
    for name, a, b in zip(names[:3], got, _control(lib, params, B, Tc, dev, with_dbg=False)):
        assert _same(a, b), ("no debug rows", name)
    # the same pass into a workspace (what the render reads)
    ws = v.new_workspace(dev)
    v.render_control(ws, params)
    ws_ctrl, ws_vconst = v.rendered_control(ws)
    assert _same(ws_ctrl.cpu(), got[0]) and _same(ws_vconst.cpu(), got[1])

    # reference 1: the round-1 kernels on the device math library
    monkeypatch.setenv("IAS_VOICE_CTRL", "libm")
    ref = _control(diag, params, B, Tc, dev)
    monkeypatch.delenv("IAS_VOICE_CTRL")
    for name, a, b in zip(names, got, ref):
        assert _same(a, b), ("libm form", name, (_bits(a) != _bits(b)).sum().item())

    # reference 2: the oracle
    cfg = so.VoiceConfig(batch_size=B, sample_rate=16000, buffer_size_seconds=sec)
    assert cfg.control_buffer_size == Tc
    o_ctrl, o_p, o_dbg = so.control_signals(cfg, p_cpu, "cr", True)
    if kind == "short_key":
        assert all((o_p("keyboard", "duration") < o_p(mod, "attack")).all() for mod in ADSRS)
    assert torch.isnan(o_ctrl).any() == (kind == "zeros")
    assert _same_values(got[0], o_ctrl.float()), ("oracle", "ctrl", (_bits(got[0]) != _bits(o_ctrl.float())).sum().item())
    assert _same_values(got[3], o_dbg.float()), ("oracle", "debug rows", (_bits(got[3]) != _bits(o_dbg.float())).sum().item())
    o_rows = torch.cat([o_dbg[:, 0:6], o_dbg[:, 8:10]], dim=1).float()
    assert _same_values(got[2], o_rows), ("oracle", "rows")
    o_vconst = _oracle_vconst(o_p)
    g_vconst = got[1][:, [0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11]]
    assert _same_values(g_vconst, o_vconst), ("oracle", "vconst", (_bits(g_vconst) != _bits(o_vconst)).nonzero().tolist())

"""The audio-rate Voice render restated in plain differentiable torch, with its inputs as the HIP backward sees them: the
control-rate signals, the 12 per-voice constants (``voice_grad.SCALARS`` order, the first 12 floats of IasVoiceConst) and
the noise row.  The formula is the one at the head of csrc/voice_grad_kernels.hip:

  upc   = Upsample(linear, align_corners)(ctrl)                                                  [B,5,T]
  arg_v = cumsum(2 pi 440 2^((clamp(f0_v + depth_v upc_pitch_v, 0, 127) - 69) / 12) / sr) + phi_v
  mix   = lvl0 cos(arg_1) upc_amp1 + lvl1 gain tanh(kpart sin(arg_2) / 2) (1 + shape cos(arg_2)) upc_amp2
        + lvl2 noise upc_ampn
  audio = mix / peak on rows with peak = max |mix| > 1                                           (normalize)

``gain`` is an input of its own (the kernel's GS_GAIN), not 1 - shape / 2, and kpart is pi * partials, hence the / 2
inside the tanh.  Everything is evaluated in the dtype of ``ctrl`` (fp64: the gradient reference; fp32: the yardstick for
what single precision costs).  torch.autograd through ``mix`` is the definition the audio-rate adjoint is tested against.
Test support: no test lives here."""
import math

import torch

SCALARS = ("f0_1", "depth_1", "phi_1", "f0_2", "depth_2", "phi_2", "kpart", "shape", "gain", "lvl0", "lvl1", "lvl2")
PITCH_1, AMP_1, PITCH_2, AMP_2, AMP_N = range(5)          # rows of ctrl (voice_spec.MOD_OUTPUTS)
DURATION = 1                                              # column of keyboard.duration among the 78 parameters

# (sample rate, seconds, control rate, T, form of ias_voice_backward: 0 lane-consecutive "fold", 1 first form); the
# backward's tile is 4096 samples
CASES = (
    (16000, 0.25, 441, 4000, 0),          # one partial tile
    (16000, 0.512, 441, 8192, 0),         # exactly two tiles, 16-byte path
    (16000, 0.5625625, 441, 9001, 0),     # two tiles + a ragged one, T % 4 != 0
    (44100, 0.2, 441, 8820, 0),           # three tiles
    (16000, 0.3, 500, 4800, 1),           # per-tile interval sums do not fit the spare plane: first form
)


def params_in_buffer(params01, seconds):
    """``params01`` [B,78] with keyboard.duration (0.01 + 3.99 u^2 s) mapped to 0.25 .. 0.75 of the buffer, so that the
    note ends and the release starts inside it."""
    p = params01.clone()
    dur = seconds * (0.25 + 0.5 * p[:, DURATION].double())
    p[:, DURATION] = torch.sqrt((dur - 0.01) / 3.99).to(p.dtype)
    return p


def upsample(ctrl, T):
    """nn.Upsample(size=T, mode="linear", align_corners=True) written out: [B,C,Tc] -> [B,C,T]."""
    Tc = ctrl.shape[-1]
    pos = torch.arange(T, dtype=ctrl.dtype, device=ctrl.device) * ((Tc - 1) / (T - 1))
    i0 = pos.floor().long().clamp_(0, Tc - 1)
    i1 = (i0 + 1).clamp_(max=Tc - 1)
    w1 = (pos - i0.to(ctrl.dtype)).clamp_(0.0, 1.0)
    return ctrl[..., i0] * (1.0 - w1) + ctrl[..., i1] * w1


def pitch(ctrl, scal, T, osc):
    """The UNCLAMPED pitch argument f0 + depth * upc_pitch of oscillator ``osc`` (1 or 2) -> [B,T]."""
    row, k = (PITCH_1, 0) if osc == 1 else (PITCH_2, 3)
    return scal[:, k:k + 1] + scal[:, k + 1:k + 2] * upsample(ctrl[:, row:row + 1], T)[:, 0]


def _phase(ctrl, scal, T, sr, osc):
    midi = torch.clamp(pitch(ctrl, scal, T, osc), 0.0, 127.0)       # the clamp passes the gradient on the closed interval
    inc = (2.0 * math.pi * 440.0 / sr) * torch.exp2((midi - 69.0) / 12.0)
    k = 2 if osc == 1 else 5
    return torch.cumsum(inc, dim=1) + scal[:, k:k + 1]


def mix(ctrl, scal, noise, T, sr, normalize=False):
    """ctrl [B,5,Tc], scal [B,12], noise [B,T] -> audio [B,T]."""
    assert ctrl.shape[1] == 5 and scal.shape[1] == len(SCALARS) and noise.shape == (ctrl.shape[0], T)
    s = {name: scal[:, i:i + 1] for i, name in enumerate(SCALARS)}
    upc = upsample(ctrl, T)
    arg1, arg2 = _phase(ctrl, scal, T, sr, 1), _phase(ctrl, scal, T, sr, 2)
    vco_1 = torch.cos(arg1) * upc[:, AMP_1]
    vco_2 = s["gain"] * torch.tanh(s["kpart"] * torch.sin(arg2) / 2.0) * (1.0 + s["shape"] * torch.cos(arg2)) * upc[:, AMP_2]
    out = s["lvl0"] * vco_1 + s["lvl1"] * vco_2 + s["lvl2"] * (noise.to(ctrl.dtype) * upc[:, AMP_N])
    if normalize:
        peak = out.abs().max(dim=1, keepdim=True)[0]
        out = torch.where(peak > 1.0, out / peak.clamp_min(1.0), out)        # (no 0 / 0 in the branch not taken)
    return out

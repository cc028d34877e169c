"""VICReg model + loss -- drop-in for the reference's vicreg.py on MI355X.

Same public names and contracts: ``VICReg(cfg, backbone_audio, backbone_param)`` with
``.forward(audio, params) -> (x, y)`` and ``.loss(x, y) -> (loss, repr_loss, std_loss, cov_loss)``
(vicreg.py:11-58), ``Projector(cfg, reprdim)`` (:61-70), ``off_diagonal`` (:73-76),
``FullGatherLayer`` (:79-95, which in the reference raises NameError because ``dist`` is never
imported -- here it works, over RCCL), ``exclude_bias_and_norm`` (:98-99).

The loss forward is the HIP path (csrc/vicreg_kernels.hip: fp32 column statistics, final reduction and the C ABI; the
covariance term as a bf16 MFMA Gram with fp32 accumulation and fused square-sum, B x B in csrc/vicreg_grad_kernels.hip
where the padded batch is no larger than the embedding, else D x D in csrc/vicreg_dxd_kernels.hip).  The backward is HIP
as well (ias_vicreg_backward4_ld, csrc/vicreg_grad_kernels.hip): closed form
with the B x B Gram identity  d cov_loss / d xc = 4/((Bc-1)^2 D) * ((xc xc^T) xc - xc diag(xc^T xc)) -- both
products on the matrix cores, one elementwise epilogue -- so no D x D matrix is ever materialised in either direction.
"""
import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F

from . import _lib


def _cotangent_ptrs(grads):
    """-> ([four device pointers, None where autograd passed None], the fp32 tensors they point into -- keep them alive
    until the launch has been issued)."""
    keep = [None if g is None else g.detach().to(torch.float32).contiguous() for g in grads]
    return [None if k is None else k.data_ptr() for k in keep], keep


def _launch_forward(x_ptr, y_ptr, ld, B, D, consts, device):
    """The loss of x, y [B, D] fp32 at two device pointers with row stride ld floats; consts = (cfg_batch, sim, std, cov).
    -> (out[4] = loss, repr, std, cov; the workspace, which keeps the column statistics / centred bf16 copies the backward
    needs)."""
    lib = _lib.load()
    need = lib.ias_vicreg_workspace_bytes(B, D)
    _lib.check(min(int(need), 0), "ias_vicreg_workspace_bytes")
    ws = torch.empty(int(need), dtype=torch.uint8, device=device)
    out = torch.empty(4, dtype=torch.float32, device=device)
    _lib.check(lib.ias_vicreg_loss_ld(x_ptr, y_ptr, ld, _lib.ptr(out), _lib.ptr(ws), ws.numel(), B, D, *consts, _lib.stream()),
               "ias_vicreg_loss_ld")
    return out, ws


def _launch_backward(x_ptr, y_ptr, ld, grads, gx_ptr, gy_ptr, ldg, ws, B, D, consts):
    """gx, gy [B, D] (row stride ldg) <- the cotangents `grads` of the four outputs, on the workspace of the forward."""
    cot, keep = _cotangent_ptrs(grads)     # (`keep` lives until the launch has been issued)
    _lib.check(_lib.load().ias_vicreg_backward4_ld(x_ptr, y_ptr, ld, *cot, gx_ptr, gy_ptr, ldg, _lib.ptr(ws), ws.numel(), B, D,
                                                   *consts, _lib.stream()), "ias_vicreg_backward4_ld")


class _VICRegLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, cfg_batch, sim_coeff, std_coeff, cov_coeff):
        xc, yc = x.detach().contiguous(), y.detach().contiguous()
        _lib.require_f32(xc, yc)
        assert xc.shape == yc.shape and xc.dim() == 2
        B, D = xc.shape
        ctx.consts = (int(cfg_batch), float(sim_coeff), float(std_coeff), float(cov_coeff))
        out, ws = _launch_forward(_lib.ptr(xc), _lib.ptr(yc), D, B, D, ctx.consts, xc.device)
        ctx.save_for_backward(xc, yc, ws)
        # unused outputs (repr / std / cov when only the loss is differentiated) arrive as None in backward instead of as
        # three freshly filled zero tensors
        ctx.set_materialize_grads(False)
        return out[0], out[1], out[2], out[3]

    @staticmethod
    def backward(ctx, g_loss, g_repr, g_std, g_cov):
        x, y, ws = ctx.saved_tensors
        B, D = x.shape
        grads = (g_loss, g_repr, g_std, g_cov)
        if all(g is None for g in grads):
            return None, None, None, None, None, None
        if D % 8 != 0:
            # The backward kernels move 16-byte groups of 8 bf16 columns.  An embedding width that is not a multiple of 8 (none
            # of the reference's configurations; toy shapes) runs them on the inputs padded with zero COLUMNS: a zero column
            # is its own mean, so it adds nothing to any covariance entry, its hinge term is a constant, and every term of
            # the loss carries the same 1 / D -- the gradient of the real columns is the padded one times D8 / D, exactly.
            D8 = (D + 7) // 8 * 8
            xp, yp = x.new_zeros((B, D8)), y.new_zeros((B, D8))
            xp[:, :D].copy_(x)
            yp[:, :D].copy_(y)
            _, wsp = _launch_forward(_lib.ptr(xp), _lib.ptr(yp), D8, B, D8, ctx.consts, x.device)
            gxp, gyp = torch.empty_like(xp), torch.empty_like(yp)
            _launch_backward(_lib.ptr(xp), _lib.ptr(yp), D8, grads, _lib.ptr(gxp), _lib.ptr(gyp), D8, wsp, B, D8, ctx.consts)
            k = float(D8) / float(D)
            return gxp[:, :D] * k, gyp[:, :D] * k, None, None, None, None
        gx, gy = torch.empty_like(x), torch.empty_like(y)
        _launch_backward(_lib.ptr(x), _lib.ptr(y), D, grads, _lib.ptr(gx), _lib.ptr(gy), D, ws, B, D, ctx.consts)
        return gx, gy, None, None, None, None


class _VICRegPairLossFn(torch.autograd.Function):
    """The same loss on xy [B, 2 D] = cat(x, y, dim=1), consumed in place as two column blocks (ias_vicreg_loss_ld) and
    differentiated into ONE [B, 2 D] cotangent (ias_vicreg_backward4_ld): the shape in which the gathered batch arrives
    from, and its gradient goes back to, the single collective of ``gather_rows``.  No split / cat copies."""

    @staticmethod
    def forward(ctx, xy, cfg_batch, sim_coeff, std_coeff, cov_coeff):
        xyc = xy.detach().contiguous()
        _lib.require_f32(xyc)
        assert xyc.dim() == 2 and xyc.shape[1] % 2 == 0
        B, D = xyc.shape[0], xyc.shape[1] // 2
        assert D % 8 == 0, "pair form: embedding width must be a multiple of 8 (use vicreg_loss on the two halves)"
        ctx.consts = (int(cfg_batch), float(sim_coeff), float(std_coeff), float(cov_coeff))
        base = xyc.data_ptr()
        out, ws = _launch_forward(base, base + 4 * D, 2 * D, B, D, ctx.consts, xyc.device)
        ctx.save_for_backward(xyc, ws)
        ctx.set_materialize_grads(False)
        return out[0], out[1], out[2], out[3]

    @staticmethod
    def backward(ctx, g_loss, g_repr, g_std, g_cov):
        xy, ws = ctx.saved_tensors
        B, D = xy.shape[0], xy.shape[1] // 2
        grads = (g_loss, g_repr, g_std, g_cov)
        if all(g is None for g in grads):
            return None, None, None, None, None
        g = torch.empty_like(xy)
        base, gbase = xy.data_ptr(), g.data_ptr()
        _launch_backward(base, base + 4 * D, 2 * D, grads, gbase, gbase + 4 * D, 2 * D, ws, B, D, ctx.consts)
        return g, None, None, None, None


def vicreg_loss(x, y, cfg_batch_size, sim_coeff=25.0, std_coeff=25.0, cov_coeff=1.0):
    """(loss, repr_loss, std_loss, cov_loss) of vicreg.py:35-58 for x, y [B, D] on a ROCm device."""
    return _VICRegLossFn.apply(x, y, cfg_batch_size, sim_coeff, std_coeff, cov_coeff)


def vicreg_loss_pair(xy, cfg_batch_size, sim_coeff=25.0, std_coeff=25.0, cov_coeff=1.0):
    """``vicreg_loss(xy[:, :D], xy[:, D:], ...)`` for xy [B, 2 D] without materialising the halves."""
    return _VICRegPairLossFn.apply(xy, cfg_batch_size, sim_coeff, std_coeff, cov_coeff)


def _gather_active(gather):
    """``gather`` as VICReg.gather_distributed: falsy = local loss; True = gather when the group has more than one rank;
    "always" = gather on a one-rank group too (runs the collective branches on a single GPU: tests, bench)."""
    return bool(gather) and dist.is_available() and dist.is_initialized() and \
        (dist.get_world_size() > 1 or gather == "always")


def global_batch_loss(x, y, batch_per_rank, sim_coeff=25.0, std_coeff=25.0, cov_coeff=1.0, gather=True):
    """The loss of vicreg.py:35-58 with the cross-rank gather the reference keeps commented out (:38-39) switched on: the
    BASELINE configs[3] path, shared by ``VICReg.loss`` and ``bench.py --workload vicreg --gpus N``.

    * ONE collective per direction: ``gather_rows(cat(x, y, dim=1))`` (all-gather forward, reduce-scatter backward) instead
      of one FullGatherLayer per branch; the gathered [W B_l, 2 D] buffer is consumed in place (``vicreg_loss_pair``).
    * Covariance denominator ``batch_per_rank * world - 1``.  vicreg.py:47-48 divides by the CONFIGURED batch size minus
      one; in facebookresearch/vicreg, where the gather is live, that configured size is the global batch.  Here
      ``cfg.vicreg.batch_size`` is the per-rank batch (it sizes the synth: vicreg_audio_params.py:87), so the global value
      is batch_per_rank x world.  Without the gather the denominator stays the configured per-rank value, quirk included.
    * All four terms are taken on the gathered batch.  (The reference computes repr_loss before the commented gather, on
      the local rows; the gathered MSE is the mean of the ranks' local MSEs: the sync_dist-logged metric and, after the
      DDP average, every parameter gradient are the same.)
    Every rank returns the same 4-tuple; a rank's x.grad / y.grad are W x its rows of d loss / d (x_g, y_g), as
    FullGatherLayer's summing backward (vicreg.py:92-95) defines, which the gradient average over ranks turns back into
    d loss / d theta."""
    if not _gather_active(gather):
        return vicreg_loss(x, y, batch_per_rank, sim_coeff, std_coeff, cov_coeff)
    world = dist.get_world_size()
    D = x.shape[1]
    xy = gather_rows(torch.cat([x, y], dim=1))
    if D % 8 != 0:
        return vicreg_loss(xy[:, :D], xy[:, D:], batch_per_rank * world, sim_coeff, std_coeff, cov_coeff)
    return vicreg_loss_pair(xy, batch_per_rank * world, sim_coeff, std_coeff, cov_coeff)


class VICReg(nn.Module):
    def __init__(self, cfg, backbone_audio, backbone_param, gather_distributed=False):
        super().__init__()
        self.cfg = cfg
        self.reprdim = cfg.dim
        self.embeddim = cfg.embeddim
        self.backbone_audio = backbone_audio
        self.backbone_param = backbone_param
        self.projector = Projector(cfg, self.reprdim)
        # the reference keeps the cross-rank gather commented out (vicreg.py:38-39); opt-in here
        self.gather_distributed = gather_distributed

    def forward(self, audio, params):
        return project_pair(self.projector, self.backbone_audio(audio), self.backbone_param(params))

    def loss(self, x, y):
        assert x.shape[1] == self.embeddim
        v = self.cfg.vicreg
        return global_batch_loss(x, y, v.batch_size, v.sim_coeff, v.std_coeff, v.cov_coeff, gather=self.gather_distributed)


def Projector(cfg, reprdim):
    widths = [int(w) for w in (f"{reprdim}-{cfg.vicreg.mlp}" % cfg.embeddim).split("-")]
    layers = []
    for fan_in, fan_out in zip(widths[:-2], widths[1:-1]):
        layers += [nn.Linear(fan_in, fan_out), nn.BatchNorm1d(fan_out), nn.ReLU(True)]
    layers.append(nn.Linear(widths[-2], widths[-1], bias=False))
    return nn.Sequential(*layers)


class _BN1dGroupsFn(torch.autograd.Function):
    """relu?(BatchNorm1d_train(z + lin_bias)) on G stacked row groups, each with its own batch statistics, the running
    statistics updated group after group (csrc/bn_kernels.hip: ias_bn1d_groups_forward / _backward, one launch each)."""

    @staticmethod
    def forward(ctx, z, lin_bias, weight, bias, running_mean, running_var, num_batches_tracked, eps, momentum, groups, relu):
        lib = _lib.load()
        z = z.contiguous()
        _lib.require_f32(z, weight, bias)
        R, Fdim = z.shape
        n = R // groups
        y = torch.empty_like(z)
        mean = torch.empty((groups, Fdim), dtype=torch.float32, device=z.device)
        invstd = torch.empty_like(mean)
        _lib.check(lib.ias_bn1d_groups_forward(_lib.ptr(z), _lib.ptr(lin_bias), _lib.ptr(weight), _lib.ptr(bias),
                                               _lib.ptr(running_mean), _lib.ptr(running_var), _lib.ptr(num_batches_tracked),
                                               _lib.ptr(y), _lib.ptr(mean), _lib.ptr(invstd), groups, n, Fdim, float(eps),
                                               float(momentum), int(relu), _lib.stream()), "ias_bn1d_groups_forward")
        ctx.save_for_backward(z, lin_bias, weight, bias, mean, invstd)
        ctx.groups, ctx.relu = groups, int(relu)
        return y

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        z, lin_bias, weight, bias, mean, invstd = ctx.saved_tensors
        g = g.contiguous()
        R, Fdim = z.shape
        dx = torch.empty_like(z)
        gw = torch.empty_like(weight) if weight is not None else None
        gb = torch.empty_like(bias) if bias is not None else None
        glb = torch.empty_like(lin_bias) if lin_bias is not None else None
        _lib.check(lib.ias_bn1d_groups_backward(_lib.ptr(z), _lib.ptr(lin_bias), _lib.ptr(g), _lib.ptr(weight),
                                                _lib.ptr(bias), _lib.ptr(mean), _lib.ptr(invstd), _lib.ptr(dx), _lib.ptr(gw),
                                                _lib.ptr(gb), _lib.ptr(glb), ctx.groups, R // ctx.groups, Fdim, ctx.relu,
                                                _lib.stream()), "ias_bn1d_groups_backward")
        return dx, glb, gw, gb, None, None, None, None, None, None, None


def _bn1d_hip_ok(m, t, n):
    return (isinstance(m, nn.BatchNorm1d) and m.training and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and
            n >= 2 and m.affine and m.track_running_stats and m.momentum is not None and m.num_batches_tracked is not None
            and not PROJECT_PAIR_TORCH)


class _SplitRowsFn(torch.autograd.Function):
    """t -> (t[:n], t[n:]); the backward is ONE concatenation (two slice nodes cost two zero fills, two copies and an add)."""

    @staticmethod
    def forward(ctx, t, n):
        return t[:n], t[n:]

    @staticmethod
    def backward(ctx, ga, gb):
        return torch.cat([ga, gb], 0), None


PROJECT_PAIR_TORCH = False    # tests / diagnostics: every BatchNorm1d of project_pair through nn.BatchNorm1d


def project_pair(projector, a, b):
    """``projector(a), projector(b)`` (reference vicreg.py:27-30: the shared projector applied to both branches) with
    every Linear run ONCE on the concatenated rows and every BatchNorm1d on each branch alone, in the order a, b -- the
    same statistics, running-stat updates and outputs as two calls.  At embeddim 8192 the two calls cost two weight
    gradients per layer (each a 268 MB write) plus the add that accumulates them; the pair form costs one.
    Training on the GPU: Linear -> BatchNorm1d -> ReLU runs as one GEMM without bias + ONE launch for the Linear's bias,
    both branches' normalisation, the running statistics, their counter and the ReLU (``_BN1dGroupsFn``)."""
    mods = list(projector) if isinstance(projector, nn.Sequential) else None
    if mods is None or a.shape != b.shape or a.dim() != 2 or not all(
            isinstance(m, (nn.Linear, nn.modules.batchnorm._BatchNorm, nn.ReLU)) for m in mods):
        return projector(a), projector(b)
    n = a.shape[0]
    t = torch.cat([a, b], 0)
    i = 0
    while i < len(mods):
        m = mods[i]
        nxt = mods[i + 1] if i + 1 < len(mods) else None
        if isinstance(m, nn.Linear) and nxt is not None and _bn1d_hip_ok(nxt, t, n):
            relu = i + 2 < len(mods) and isinstance(mods[i + 2], nn.ReLU)
            t = _BN1dGroupsFn.apply(F.linear(t, m.weight), m.bias, nxt.weight, nxt.bias, nxt.running_mean, nxt.running_var,
                                    nxt.num_batches_tracked, nxt.eps, nxt.momentum, 2, relu)
            i += 3 if relu else 2
            continue
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            if _bn1d_hip_ok(m, t, n):
                t = _BN1dGroupsFn.apply(t, None, m.weight, m.bias, m.running_mean, m.running_var, m.num_batches_tracked,
                                        m.eps, m.momentum, 2, False)
            else:
                t = torch.cat([m(t[:n]), m(t[n:])], 0)
        else:
            t = m(t)
        i += 1
    if t.is_cuda and not PROJECT_PAIR_TORCH:
        return _SplitRowsFn.apply(t, n)
    return t[:n], t[n:]


def off_diagonal(x):
    """All elements i != j of a square matrix, row-major order (vicreg.py:73-76)."""
    n, m = x.shape
    assert n == m
    return x.flatten()[:-1].view(n - 1, n + 1)[:, 1:].flatten()


class FullGatherLayer(torch.autograd.Function):
    """Gather a tensor from every rank with gradient support (vicreg.py:79-95).

    forward : all_gather -> tuple of world_size tensors (RCCL over xGMI when the backend is nccl).
    backward: the reference stacks the incoming grads, all_reduces the whole [W, B_l, D] stack and keeps
              slice [rank]; that is a reduce_scatter, which moves W times fewer bytes -- used when the
              backend provides it (RCCL), with the all_reduce form as the gloo fallback.  Same result.
    """

    @staticmethod
    def forward(ctx, x):
        world = dist.get_world_size()
        x = x.contiguous()
        if dist.get_backend() == "nccl":
            flat = torch.empty((world,) + tuple(x.shape), dtype=x.dtype, device=x.device)
            dist.all_gather_into_tensor(flat, x)
            return tuple(flat[i] for i in range(world))
        output = [torch.zeros_like(x) for _ in range(world)]
        dist.all_gather(output, x)
        return tuple(output)

    @staticmethod
    def backward(ctx, *grads):
        stacked = torch.stack(grads).contiguous()
        if dist.get_backend() == "nccl":
            out = torch.empty_like(stacked[0])
            dist.reduce_scatter_tensor(out, stacked)
            return out
        dist.all_reduce(stacked)
        return stacked[dist.get_rank()]


class _GatherRowsFn(torch.autograd.Function):
    """``torch.cat(FullGatherLayer.apply(x), dim=0)`` as one [W B_l, ...] tensor: the all-gather lands in the result
    (no tuple of views, no cat), the backward reduce-scatters the cotangent as it stands (no stack)."""

    @staticmethod
    def forward(ctx, x):
        world = dist.get_world_size()
        x = x.contiguous()
        ctx.rows = x.shape[0]
        if dist.get_backend() == "nccl":
            out = torch.empty((world * x.shape[0],) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
            dist.all_gather_into_tensor(out, x)
            return out
        parts = [torch.zeros_like(x) for _ in range(world)]
        dist.all_gather(parts, x)
        return torch.cat(parts, dim=0)

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        if dist.get_backend() == "nccl":
            out = torch.empty((ctx.rows,) + tuple(g.shape[1:]), dtype=g.dtype, device=g.device)
            dist.reduce_scatter_tensor(out, g)
            return out
        g = g.clone()
        dist.all_reduce(g)
        r = dist.get_rank()
        return g[r * ctx.rows:(r + 1) * ctx.rows]


def gather_rows(x):
    """Rows of every rank, rank-major: value and gradient of ``torch.cat(FullGatherLayer.apply(x), dim=0)``."""
    return _GatherRowsFn.apply(x)


def exclude_bias_and_norm(p):
    return p.ndim == 1

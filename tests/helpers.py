import torch


def randn(shape, seed):
    """Seeded CPU randn (same generator the golden script uses)."""
    return torch.randn(shape, generator=torch.Generator(device="cpu").manual_seed(seed))


def checks(t):
    d = t.double()
    return [d.sum().item(), d.abs().sum().item(), (d * d).sum().item()]


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def vicreg_backward_closed_form(x, y, gcoef, cfg_batch, sim, std, cov):
    """The closed-form gradient of the VICReg loss (/root/reference/vicreg.py:35-58) as plain fp32 torch ops on the inputs'
    device: a second definition the HIP backward is tested against, besides autograd through the oracle (test
    infrastructure: the package does not use it).  gcoef: the cotangents of (loss, repr, std, cov)."""
    B, D = x.shape
    a = gcoef[0] * sim + gcoef[1]
    b = gcoef[0] * std + gcoef[2]
    c = gcoef[0] * cov + gcoef[3]
    d_repr = (x - y) * (2.0 / (B * D))

    def branch(v):
        vc = v - v.mean(dim=0)
        m2 = (vc * vc).sum(dim=0)
        s = torch.sqrt(m2 / (B - 1) + 0.0001)
        d_std = -(s < 1).to(v.dtype) / (2.0 * D * (B - 1) * s) * vc
        gram = vc @ vc.T
        d_cov = (gram @ vc - vc * m2) * (4.0 / ((cfg_batch - 1) ** 2 * D))
        return b * d_std + c * d_cov

    return a * d_repr + branch(x), -a * d_repr + branch(y)


SENT, GUARD = -777.0, 64


class Guarded:
    """A device tensor `t` of `shape` inside a 1-D buffer with GUARD sentinels on each side (and sentinels in it until it is
    written): what a kernel stores outside its output, or does not store at all, stays visible.  `sent`: the sentinel
    (NaN for a kernel's INPUTS: a read outside the payload that enters arithmetic poisons the result).  `offset`: `t` starts
    that many elements later (the front guard grows by them), for a payload that is not aligned as the allocation is."""

    def __init__(self, dev, shape, init=None, dtype=torch.float32, sent=SENT, offset=0):
        n = 1
        for d in shape:
            n *= d
        self.sent = sent
        self.lo, self.hi = GUARD + offset, GUARD + offset + n
        self.buf = torch.full((n + 2 * GUARD + offset,), sent, dtype=dtype, device=dev)
        self.t = self.buf[self.lo:self.hi].view(shape)
        if init is not None:
            self.t.copy_(init)

    def is_sent(self, t):
        """Elementwise: does t still hold the sentinel?"""
        return torch.isnan(t) if self.sent != self.sent else t == self.sent

    def guards_intact(self):
        return bool(self.is_sent(self.buf[:self.lo]).all()) and bool(self.is_sent(self.buf[self.hi:]).all())

    def untouched(self):
        return bool(self.is_sent(self.buf).all())

    def cpu(self):
        return self.t.detach().cpu().clone()

"""The harness of tests/test_dwconv_capi_gpu.py and tests/test_stem_capi_gpu.py: one convolution shape's device buffers and
its calls through the C ABI (csrc/conv_kernels.hip), with everything a kernel could get wrong outside its arithmetic made
visible.  Outputs and scratch live between sentinel guards and hold sentinels until written; inputs live between NaN
guards with a finite payload, so a read outside an input that enters arithmetic shows in the result; every buffer is
16-byte aligned, as the library's callers' are."""
import ctypes

import torch

import conv_model as cm
from helpers import Guarded

NAN = float("nan")


class ConvRun:
    """kind "dw": shape (B, C, H, W, K, S), depthwise; kind "stem": shape (B, H, W), Conv2d(3, 16, 3, 2, 1)."""

    def __init__(self, lib, dev, kind, shape):
        self.kind, self.shape, self.dims = kind, shape, tuple(shape)
        if kind == "dw":
            B, C, H, W, K, S = shape
            cin, cout, wshape = C, C, (C, 1, K, K)
            floats = lib.ias_dwconv_weight_scratch_hw(B, C, H, W, K, S)
        else:
            (B, H, W), K, S = shape, 3, 2
            cin, cout, wshape = 3, 16, (16, 3, 3, 3)
            floats = lib.ias_stem_weight_scratch(B)
        self.B, self.H, self.W, self.K, self.S = B, H, W, K, S
        self.Ho, self.Wo = lib.ias_conv_out_size(H, K, S), lib.ias_conv_out_size(W, K, S)
        assert (self.Ho, self.Wo) == (cm.out_size(H, K, S), cm.out_size(W, K, S))
        self.n = wshape[0] * wshape[1] * K * K                    # floats of the weight gradient = of one partial row
        assert floats >= self.n, floats
        self.x = Guarded(dev, (B, cin, H, W), sent=NAN)
        self.w = Guarded(dev, wshape, sent=NAN)
        self.g = Guarded(dev, (B, cout, self.Ho, self.Wo), sent=NAN)
        self.out = {"y": Guarded(dev, (B, cout, self.Ho, self.Wo)), "gw": Guarded(dev, wshape), "gw_multi": Guarded(dev, wshape)}
        if kind == "dw":
            self.out["gx"] = Guarded(dev, (B, cin, H, W))
        self.s1, self.s2 = Guarded(dev, (int(floats),)), Guarded(dev, (int(floats),))
        for b in (self.x, self.w, self.g, self.s1, self.s2, *self.out.values()):
            assert b.t.data_ptr() % 16 == 0

    def load(self, x, w, g):
        self.x.t.copy_(x)
        self.w.t.copy_(w)
        self.g.t.copy_(g)

    def clear(self):
        """Outputs and scratch back to their sentinels."""
        for b in (self.s1, self.s2, *self.out.values()):
            b.t.fill_(b.sent)

    # ---- the entries (status or row count as returned; `null`: the name of one pointer passed as NULL; dims: another tuple)
    def _p(self, buf, name, null):
        from inverse_audio_synthesis_amd import _lib
        return None if name == null else _lib.ptr(buf.t)

    def forward(self, lib, null=None, dims=None):
        from inverse_audio_synthesis_amd import _lib
        entry = lib.ias_dwconv_forward if self.kind == "dw" else lib.ias_stem_forward
        return entry(self._p(self.x, "x", null), self._p(self.w, "w", null), self._p(self.out["y"], "y", null),
                     *(dims or self.dims), _lib.stream())

    def backward_data(self, lib, null=None, dims=None):
        from inverse_audio_synthesis_amd import _lib
        return lib.ias_dwconv_backward_data(self._p(self.g, "g", null), self._p(self.w, "w", null),
                                            self._p(self.out["gx"], "gx", null), *(dims or self.dims), _lib.stream())

    def backward_weight(self, lib, with_gw=True, null=None, dims=None):
        """with_gw: into gw with the entry's own reduction (scratch s1); else gw = NULL, the rows stay in s2."""
        from inverse_audio_synthesis_amd import _lib
        entry = lib.ias_dwconv_backward_weight if self.kind == "dw" else lib.ias_stem_backward_weight
        gw = _lib.ptr(self.out["gw"].t) if with_gw else None
        return entry(self._p(self.x, "x", null), self._p(self.g, "g", null), gw,
                     self._p(self.s1 if with_gw else self.s2, "scratch", null), *(dims or self.dims), _lib.stream())

    def reduce_multi(self, lib, rows):
        from inverse_audio_synthesis_amd import _lib
        from inverse_audio_synthesis_amd.vision import _ReduceItem
        item = _ReduceItem(self.s2.t.data_ptr(), self.out["gw_multi"].t.data_ptr(), self.n, rows)
        return lib.ias_reduce_partials_multi(ctypes.cast(ctypes.pointer(item), ctypes.c_void_p), 1, _lib.stream())

    def run(self, lib, weight_gradient=True, rows_expected=None):
        """Every entry once on the loaded inputs -> the outputs on the CPU, "rows" among them.  Asserted here: the statuses,
        the row count, every guard, every output element written, exactly rows * n floats of each scratch changed and
        the same bits in both, the inputs as they were loaded."""
        self.clear()
        before = [b.t.clone() for b in (self.x, self.w, self.g)]
        assert self.forward(lib) == 0
        names = ["y"]
        if self.kind == "dw":
            assert self.backward_data(lib) == 0
            names.append("gx")
        rows = None
        if weight_gradient:
            rows = self.backward_weight(lib, True)
            assert rows > 0 and rows * self.n <= self.s1.t.numel(), rows
            assert self.backward_weight(lib, False) == rows
            assert self.reduce_multi(lib, rows) == 0
            names += ["gw", "gw_multi"]
            if rows_expected is not None:
                assert rows == rows_expected, (self.shape, rows, rows_expected)
        torch.cuda.synchronize()
        for b, was in zip((self.x, self.w, self.g), before):
            assert b.guards_intact() and torch.equal(b.t, was), "an input was written"
        for k, b in self.out.items():
            assert b.guards_intact(), (self.shape, k, "stored outside the output")
            if k in names:
                assert not bool(b.is_sent(b.t).any()), (self.shape, k, "an output element was never stored")
            else:
                assert b.untouched(), (self.shape, k)
        used = rows * self.n if weight_gradient else 0
        for s in (self.s1, self.s2):
            assert s.guards_intact(), (self.shape, "stored outside the scratch")
            assert not bool(s.is_sent(s.t[:used]).any()), (self.shape, "a partial row element was never stored")
            assert bool(s.is_sent(s.t[used:]).all()), (self.shape, "stored beyond the partial rows")
        assert torch.equal(self.s1.t[:used], self.s2.t[:used])
        res = {k: self.out[k].cpu() for k in names}
        res["rows"] = rows
        return res

    def untouched(self):
        torch.cuda.synchronize()
        return all(b.untouched() for b in (self.s1, self.s2, *self.out.values()))


def same_bits(a, b, names):
    for k in names:
        assert torch.equal(a[k], b[k]), (k, "two runs on the same inputs differ")

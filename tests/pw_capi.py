"""The harness of tests/test_pwconv_capi_gpu.py: one 1x1-convolution shape's device buffers and its calls through the C ABI
(csrc/pointwise_kernels.hip), with everything a kernel could get wrong outside its arithmetic made visible.  Outputs and
scratch live between sentinel guards and hold sentinels until written; inputs live between NaN guards with a finite
payload, so a read outside an input that enters arithmetic shows in the result.  Every buffer is 16-byte aligned unless
`offsets` moves it by a number of floats (the C ABI takes such activations: pw_vec picks narrower loads and stores)."""
import ctypes

import torch

import pw_geometry as pg
from helpers import Guarded

NAN = float("nan")
OUT_SENT = -777.3125      # no integer and no half-integer: the exact input sets cannot produce it
OUTPUTS = ("y", "gx", "gw", "gw_multi")


class PwRun:
    """shape (B, Cin, Cout, HW); offsets: buffer name (x, s, w, g, y, gx, gw, gw_multi, s1, s2) -> floats past 16-byte
    alignment."""

    def __init__(self, lib, dev, shape, offsets=None):
        self.shape = self.dims = tuple(shape)
        B, Cin, Cout, HW = shape
        off = dict(offsets or {})
        self.n = Cout * Cin                                      # floats of the weight gradient = of one partial row
        floats = lib.ias_pwconv_weight_scratch(B, Cin, Cout, HW)
        assert floats == pg.weight_scratch_floats(B, Cin, Cout, HW), (shape, floats)
        self.x = Guarded(dev, (B, Cin, HW), sent=NAN, offset=off.pop("x", 0))
        self.s = Guarded(dev, (B, Cin), sent=NAN, offset=off.pop("s", 0))
        self.w = Guarded(dev, (Cout, Cin), sent=NAN, offset=off.pop("w", 0))
        self.g = Guarded(dev, (B, Cout, HW), sent=NAN, offset=off.pop("g", 0))
        shapes = {"y": (B, Cout, HW), "gx": (B, Cin, HW), "gw": (Cout, Cin), "gw_multi": (Cout, Cin)}
        self.out = {k: Guarded(dev, shapes[k], sent=OUT_SENT, offset=off.pop(k, 0)) for k in OUTPUTS}
        self.s1 = Guarded(dev, (int(floats),), sent=OUT_SENT, offset=off.pop("s1", 0))
        self.s2 = Guarded(dev, (int(floats),), sent=OUT_SENT, offset=off.pop("s2", 0))
        assert not off, off
        self.inputs = (self.x, self.s, self.w, self.g)
        self.bufs = {"x": self.x, "s": self.s, "w": self.w, "g": self.g, "s1": self.s1, "s2": self.s2, **self.out}
        for k, b in self.bufs.items():
            assert b.buf.data_ptr() % 16 == 0 and b.t.data_ptr() % 16 == 4 * ((offsets or {}).get(k, 0) % 4), k

    def load(self, x, s, w, g):
        for b, v in zip(self.inputs, (x, s, w, g)):
            b.t.copy_(v)

    def clear(self):
        """Outputs and scratch back to their sentinels."""
        for b in (self.s1, self.s2, *self.out.values()):
            b.t.fill_(b.sent)

    def vecs(self):
        """VEC of (forward, input gradient, weight gradient) as pw_vec takes it from these buffers' addresses."""
        HW, p = self.shape[3], {k: b.t.data_ptr() for k, b in self.bufs.items()}
        return pg.vec(p["x"], p["y"], HW), pg.vec(p["g"], p["gx"], HW), pg.vec(p["g"], p["x"], HW)

    # ---- the entries (status or row count as returned; `null`: the name of one pointer passed as NULL; dims: another tuple)
    def _p(self, buf, name, null):
        from inverse_audio_synthesis_amd import _lib
        return None if name == null else _lib.ptr(buf.t)

    def forward(self, lib, scaled=False, null=None, dims=None):
        from inverse_audio_synthesis_amd import _lib
        return lib.ias_pwconv_forward(self._p(self.x, "x", null), _lib.ptr(self.s.t) if scaled else None,
                                      self._p(self.w, "w", null), self._p(self.out["y"], "y", null),
                                      *(dims or self.dims), _lib.stream())

    def backward_data(self, lib, null=None, dims=None):
        from inverse_audio_synthesis_amd import _lib
        return lib.ias_pwconv_backward_data(self._p(self.g, "g", null), self._p(self.w, "w", null),
                                            self._p(self.out["gx"], "gx", null), *(dims or self.dims), _lib.stream())

    def backward_weight(self, lib, with_gw=True, scaled=False, null=None, dims=None):
        """with_gw: into gw with the entry's own reduction (scratch s1); else gw = NULL, the rows stay in s2."""
        from inverse_audio_synthesis_amd import _lib
        gw = _lib.ptr(self.out["gw"].t) if with_gw else None
        return lib.ias_pwconv_backward_weight(self._p(self.g, "g", null), self._p(self.x, "x", null),
                                              _lib.ptr(self.s.t) if scaled else None, gw,
                                              self._p(self.s1 if with_gw else self.s2, "scratch", null),
                                              *(dims or self.dims), _lib.stream())

    def reduce_multi(self, lib, rows):
        from inverse_audio_synthesis_amd import _lib
        from inverse_audio_synthesis_amd.vision import _ReduceItem
        item = _ReduceItem(self.s2.t.data_ptr(), self.out["gw_multi"].t.data_ptr(), self.n, rows)
        return lib.ias_reduce_partials_multi(ctypes.cast(ctypes.pointer(item), ctypes.c_void_p), 1, _lib.stream())

    def run(self, lib, scaled=False):
        """Every entry once on the loaded inputs -> the outputs on the CPU, "rows" among them.  Asserted here: the statuses,
        the row count against pw_geometry and the scratch size, every guard, every output element written, exactly
        rows * n floats of each scratch changed and the same bits in both, the inputs as they were loaded, gw and
        gw_multi the same bits."""
        self.clear()
        before = [b.t.clone() for b in self.inputs]
        assert self.forward(lib, scaled) == 0
        assert self.backward_data(lib) == 0
        rows = self.backward_weight(lib, True, scaled)
        assert rows == pg.backward_weight_form(*self.shape, scaled=scaled)["rows"], (self.shape, rows)
        assert rows > 0 and rows * self.n <= self.s1.t.numel(), rows
        assert self.backward_weight(lib, False, scaled) == rows
        assert self.reduce_multi(lib, rows) == 0
        torch.cuda.synchronize()
        for b, was in zip(self.inputs, before):
            assert b.guards_intact() and torch.equal(b.t, was), (self.shape, "an input was written")
        for k, b in self.out.items():
            assert b.guards_intact(), (self.shape, k, "stored outside the output")
            assert not bool(b.is_sent(b.t).any()), (self.shape, k, "an output element was never stored")
        used = rows * self.n
        for s in (self.s1, self.s2):
            assert s.guards_intact(), (self.shape, "stored outside the scratch")
            assert not bool(s.is_sent(s.t[:used]).any()), (self.shape, "a partial row element was never stored")
            assert bool(s.is_sent(s.t[used:]).all()), (self.shape, "stored beyond the partial rows")
        assert torch.equal(self.s1.t[:used], self.s2.t[:used])
        res = {k: self.out[k].cpu() for k in OUTPUTS}
        assert torch.equal(res["gw"], res["gw_multi"]), (self.shape, "the two reductions differ")
        res["rows"] = rows
        return res

    def untouched(self):
        """No output and no scratch element written, every input as loaded (guards included)."""
        torch.cuda.synchronize()
        return all(b.untouched() for b in (self.s1, self.s2, *self.out.values())) and all(b.guards_intact() for b in self.inputs)


def same_bits(a, b, names=OUTPUTS):
    for k in names:
        assert torch.equal(a[k], b[k]), (k, "the same inputs gave other bits")

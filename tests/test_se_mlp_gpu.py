"""ias_se_mlp_forward / _backward (csrc/se_kernels.hip) through the C ABI against the fp64 model of tests/se_mlp_model.py:
the shapes whose dynamic LDS exceeds 64 KB (the pair backward from C = 960 to its cap of 1024, the forward from
C + Cs > 8192 to the ABI's limit of 12288), one sample, the scalar forms, NULL biases, weights that are not 16-byte
aligned, the refused size.  The backward is fed the kernel's own forward outputs z and h, and the model reads its masks
from the same arrays.  Every output lives between guards; every shape runs twice for equal bits."""
import pytest
import torch

import se_mlp_model as sm
from helpers import Guarded

pytestmark = pytest.mark.gpu
FWD, BWD = ("h", "z", "s"), ("gz", "gh", "gp", "gw1", "gb1", "gw2", "gb2")


class Run:
    """Device inputs and guarded outputs of one forward + backward.  `null`: names passed as NULL; `offset`: w1 and w2
    start this many floats into their (16-byte aligned) buffers."""

    def __init__(self, dev, inp, B, C, Cs, null=(), offset=0):
        self.dims = (B, C, Cs)
        self.pooled, self.gs = inp.pooled.to(dev), inp.gs.to(dev)
        for k, shape in (("w1", (Cs, C)), ("w2", (C, Cs))):
            buf = torch.zeros(Cs * C + 4, device=dev)
            w = buf[offset:offset + Cs * C].view(shape)
            w.copy_(getattr(inp, k))
            assert w.data_ptr() % 16 == 4 * offset
            setattr(self, k, w)
        self.b1 = None if "b1" in null else inp.b1.to(dev)
        self.b2 = None if "b2" in null else inp.b2.to(dev)
        shapes = {"h": (B, Cs), "z": (B, C), "s": (B, C), "gz": (B, C), "gh": (B, Cs), "gp": (B, C), "gw1": (Cs, C), "gb1": (Cs,),
                  "gw2": (C, Cs), "gb2": (C,)}
        self.o = {k: (None if k in null else Guarded(dev, shp)) for k, shp in shapes.items()}

    def _p(self, k):
        from inverse_audio_synthesis_amd import _lib
        return None if self.o[k] is None else _lib.ptr(self.o[k].t)

    def forward(self, lib, dims=None):
        from inverse_audio_synthesis_amd import _lib
        p = _lib.ptr
        return lib.ias_se_mlp_forward(p(self.pooled), p(self.w1), p(self.b1), p(self.w2), p(self.b2), self._p("h"), self._p("z"),
                                      self._p("s"), *(dims or self.dims), _lib.stream())

    def backward(self, lib, dims=None):
        from inverse_audio_synthesis_amd import _lib
        p = _lib.ptr
        return lib.ias_se_mlp_backward(p(self.gs), self._p("z"), self._p("h"), p(self.pooled), p(self.w1), p(self.w2),
                                       self._p("gz"), self._p("gh"), self._p("gp"), self._p("gw1"), self._p("gb1"),
                                       self._p("gw2"), self._p("gb2"), *(dims or self.dims), _lib.stream())

    def out(self):
        torch.cuda.synchronize()
        assert all(g.guards_intact() for g in self.o.values() if g is not None)
        return {k: g.cpu() for k, g in self.o.items() if g is not None}


def _both(lib, dev, inp, shape, null=(), offset=0):
    run = Run(dev, inp, *shape, null=null, offset=offset)
    lds_fwd = 8 * (shape[1] + shape[2])
    st = run.forward(lib)
    torch.cuda.synchronize()
    print("SE-LAUNCH forward", shape, f"dynamic LDS {lds_fwd} bytes", "status", st)
    assert st == 0
    st = run.backward(lib)
    torch.cuda.synchronize()
    print("SE-LAUNCH backward", shape, "status", st)
    assert st == 0
    return run.out()


def _assert_within_bounds(out, inp, null, tag):
    b1 = None if "b1" in null else inp.b1
    b2 = None if "b2" in null else inp.b2
    fw = sm.forward(inp.pooled, inp.w1, b1, inp.w2, b2)
    bw = sm.backward(inp.gs, out["z"], out["h"], inp.pooled, inp.w1, inp.w2)     # masks: the arrays the kernel was given
    fr = {}
    for k in out:
        ref = getattr(fw, k) if k in FWD else getattr(bw, k)
        coeff = sm.H_BOUND if k in FWD else sm.GRAD_BOUND
        assert bool(torch.isfinite(out[k]).all()), (tag, k)
        fr[k] = (out[k].double() - ref).abs().max().item() / (coeff * max(1.0, ref.abs().max().item()))
    print("SE-FRACTIONS", tag, {k: round(v, 4) for k, v in fr.items()})
    for k, v in fr.items():
        assert v <= 1.0, (tag, k, v)


@pytest.mark.parametrize("shape", sm.SHAPES, ids=sm.SHAPE_IDS)
def test_every_shape_against_the_fp64_model_twice(lib, dev, shape):
    inp = sm.make_inputs(*shape)
    out = _both(lib, dev, inp, shape)
    _assert_within_bounds(out, inp, (), sm.SHAPE_IDS[sm.SHAPES.index(shape)])
    again = _both(lib, dev, inp, shape)
    for k in out:
        assert torch.equal(out[k], again[k]), k


@pytest.mark.parametrize("shape", sm.VARIANT_SHAPES)
def test_null_biases_are_zero_biases(lib, dev, shape):
    """b1 / b2 / gb1 / gb2 NULL: the outputs of the run with explicit zero biases, bit for bit, without the two bias
    gradients; each pointer alone and all four together."""
    inp = sm.make_inputs(*shape)
    zeros = inp._replace(b1=torch.zeros_like(inp.b1), b2=torch.zeros_like(inp.b2))
    full = _both(lib, dev, zeros, shape)
    for null in (("b1",), ("b2",), ("gb1",), ("gb2",), ("b1", "b2", "gb1", "gb2")):
        ref_inp = inp._replace(b1=zeros.b1 if "b1" in null else inp.b1, b2=zeros.b2 if "b2" in null else inp.b2)
        want = full if ("b1" in null and "b2" in null) else _both(lib, dev, ref_inp, shape)
        out = _both(lib, dev, inp, shape, null=null)
        assert set(out) == set(want) - set(null)
        for k in out:
            assert torch.equal(out[k], want[k]), (null, k)
        _assert_within_bounds(out, inp, null, f"null-{'-'.join(null)}-{shape}")


@pytest.mark.parametrize("shape", sm.VARIANT_SHAPES)
def test_weights_off_16_byte_alignment_take_the_scalar_forms(lib, dev, shape):
    inp = sm.make_inputs(*shape)
    out = _both(lib, dev, inp, shape, offset=1)
    _assert_within_bounds(out, inp, (), f"unaligned-{shape}")
    again = _both(lib, dev, inp, shape, offset=1)
    for k in out:
        assert torch.equal(out[k], again[k]), k


def test_sizes_beyond_the_abi_limit_are_refused(lib, dev):
    """C + Cs = 12289 -> IAS_ERR_ARG from both entries, nothing written; so are non-positive dimensions."""
    B, C, Cs = 1, 12225, 64
    run = Run(dev, sm.make_inputs(B, C, Cs), B, C, Cs)
    for dims in ((B, C, Cs), (0, 8, 8), (1, 0, 8), (1, 8, 0)):
        assert run.forward(lib, dims) == -1, dims
        assert run.backward(lib, dims) == -1, dims
    torch.cuda.synchronize()
    for k, g in run.o.items():
        assert g.untouched(), k

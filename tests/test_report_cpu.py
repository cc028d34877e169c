"""The match report without a GPU: the fp64 model of ias_spectral_report (tests/report_model.py) against a written-out
definition and analytic cases, the host DCT table, the symbol table of include/ias_hip_report.h, and the refusals of the
entry points, which return before any launch."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import report_model as rm
from conftest import ROOT

_CSRC = os.path.join(ROOT, "inverse-audio-synthesis_amd", "csrc")
NAMES = ["ias_report_build_dct", "ias_spectral_report", "ias_spectral_report_partials_count"]
IAS_ERR_ARG, IAS_ERR_UNSUPPORTED = -1, -2


def _written_out(v, t, fl, power, C):
    """The contract of include/ias_hip_report.h as loops over rows, frames, bins and coefficients, in Python floats."""
    B, F, K = v.shape
    a = (20.0 / power) * math.log10(2.0)
    out = np.zeros((B, 5))
    for b in range(B):
        f_b = float(fl[b])
        n, lsd, l1, mcd, num, den = 0, 0.0, 0.0, 0.0, 0.0, 0.0
        for f in range(F):
            d = [math.log2(max(float(v[b, f, k]), f_b)) - math.log2(max(float(t[b, f, k]), f_b)) for k in range(K)]
            for k in range(K):
                num += (float(t[b, f, k]) - float(v[b, f, k])) ** 2
                den += float(t[b, f, k]) ** 2
            if max(max(float(v[b, f, k]), float(t[b, f, k])) for k in range(K)) > f_b:
                n += 1
                lsd += math.sqrt(sum(x * x for x in d) / K)
                l1 += sum(abs(x) for x in d)
                q = 0.0
                for c in range(1, C + 1):
                    m = sum(math.sqrt(2.0 / K) * math.cos(math.pi * c * (2 * k + 1) / (2 * K)) * (math.log(2.0) / power)
                            * d[k] for k in range(K))
                    q += m * m
                mcd += math.sqrt(2.0 * q)
        if n:
            out[b, 0], out[b, 2], out[b, 3] = a * lsd / n, a * l1 / (n * K), (10.0 / math.log(10.0)) * mcd / n
        out[b, 1] = math.sqrt(num) / math.sqrt(den) if den > 0.0 else (math.inf if num > 0.0 else 0.0)
        out[b, 4] = n
    return out


@pytest.mark.parametrize("case", [0, 3, 4])
def test_model_agrees_with_the_written_out_definition(case):
    _B, _F, K, C, power = rm.CASES[case]
    v, t, fl = rm.inputs(case)
    got = rm.report(v, t, fl, power, rm.dct_table(K, C))
    want = _written_out(v, t, fl, power, C)
    assert np.array_equal(got[:, 4], want[:, 4])
    np.testing.assert_allclose(got[:, :4], want[:, :4], rtol=1e-12, atol=1e-13)


def test_inputs_clamp_some_elements_but_not_most():
    """4-8 % of the elements of the counted frames sit under the floor: clamping is exercised and does not dominate.  Rows
    and frames made on purpose: row 1 is v == t, frame 1 of row 0 is uncounted."""
    for case, (B, F, _K, _C, _power) in enumerate(rm.CASES):
        v, t, fl = rm.inputs(case)
        share = rm.clamped_share(v, t, fl)
        print(f"case {rm.CASES[case]}: clamped share per row {np.round(share, 4).tolist()}")
        if v[0].size >= 640:                                             # rows of a handful of elements say nothing
            assert (share > 0.02).all() and (share < 0.12).all(), share
        n = rm.counted(v, t, fl).sum(axis=1)
        assert n[0] == (F - 1 if F > 2 else F)
        if B > 1:
            assert np.array_equal(v[1], t[1])


def test_analytic_cases_of_a_doubled_target():
    """v = 2 t with every element above the floor: every d is exactly 1."""
    rng = np.random.default_rng(3)
    t = (0.5 + rng.random((2, 6, 40))).astype(np.float32)
    v = (2.0 * t).astype(np.float32)
    fl = np.full(2, 1e-3, dtype=np.float32)
    D = rm.dct_table(40, 13)
    r1 = rm.report(v, t, fl, 1, D)
    assert np.allclose(r1[:, 0], 20.0 * math.log10(2.0), rtol=1e-14) and np.allclose(r1[:, 2], r1[:, 0], rtol=1e-14)
    assert np.allclose(r1[:, 1], 1.0, rtol=1e-14) and (np.abs(r1[:, 3]) < 1e-12).all() and (r1[:, 4] == 6).all()
    r2 = rm.report(v, t, fl, 2, D)
    assert np.allclose(r2[:, 0], 10.0 * math.log10(2.0), rtol=1e-14) and np.allclose(r2[:, 2], r2[:, 0], rtol=1e-14)
    # silence on both sides: n = 0 and every figure 0; a silent target under a render: the convergence is +inf
    z = np.zeros((1, 3, 8), dtype=np.float32)
    assert np.array_equal(rm.report(z, z, fl[:1], 1), np.zeros((1, 5)))
    r = rm.report(np.ones_like(z), z, fl[:1], 1)
    assert r[0, 4] == 3 and np.isinf(r[0, 1]) and np.isfinite(r[0, [0, 2]]).all()


@pytest.mark.parametrize("n_in, n_coef", [(128, 13), (256, 32), (5, 3), (64, 20), (3, 1)])
def test_dct_table_is_the_fp64_table_rounded_once(lib, n_in, n_coef):
    from inverse_audio_synthesis_amd.report import dct_table
    got = dct_table(n_in, n_coef).numpy()
    want = rm.dct_table(n_in, n_coef)
    assert got.shape == (n_coef, n_in) and got.dtype == np.float32
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    assert (np.abs(got.astype(np.float64) - want) <= ulp).all()
    assert np.allclose(got.astype(np.float64) @ got.astype(np.float64).T, np.eye(n_coef), atol=1e-6)
    for bad in ((8, 8), (8, 0), (0, 1)):
        with pytest.raises(ValueError):
            dct_table(*bad)
    assert lib.ias_report_build_dct(8, 8, ctypes.c_void_p(got.ctypes.data)) == IAS_ERR_UNSUPPORTED
    assert lib.ias_report_build_dct(8, 0, ctypes.c_void_p(got.ctypes.data)) == IAS_ERR_ARG
    assert lib.ias_report_build_dct(8, 2, None) == IAS_ERR_ARG


def test_report_symbols_are_a_table_of_their_own(lib):
    import subprocess
    from inverse_audio_synthesis_amd import _lib
    assert sorted(_lib.REPORT_SYMBOLS) == NAMES
    assert not set(_lib.REPORT_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.DIAG_SYMBOLS))
    _P, _I = ctypes.c_void_p, ctypes.c_int
    assert _lib.REPORT_SYMBOLS["ias_spectral_report"] == (_I, [_P] * 4 + [_I] * 5 + [_P] * 3)
    assert _lib.REPORT_SYMBOLS["ias_spectral_report_partials_count"] == (ctypes.c_longlong, [_I])
    assert _lib.REPORT_SYMBOLS["ias_report_build_dct"] == (_I, [_I, _I, _P])
    diag = _lib.load_diag()
    for path, bound in ((_lib.LIB_PATH, lib), (_lib.DIAG_LIB_PATH, diag)):
        exported = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
        for name in NAMES:
            assert re.search(rf"\bT {name}\b", exported), f"{path} does not export {name}"
            assert getattr(bound, name).argtypes == _lib.REPORT_SYMBOLS[name][1]


def test_report_kernels_are_compiled_against_the_new_header():
    """report_kernels.hip reaches include/ias_hip_report.h through its includes, declares no ias_* by hand, and keeps to
    the product library's rules: nothing read from the environment, no inline assembly."""
    from test_capi_symbols import _code, _reaches
    path = os.path.join(_CSRC, "report_kernels.hip")
    assert _reaches(path, os.path.join(ROOT, "include", "ias_hip_report.h"), set())
    code = _code(path)
    assert not re.findall(r'extern\s+"C"[^;{]*\bias_\w+\s*\([^;{]*;', code)
    defined = sorted(re.findall(r'extern\s+"C"[^;{(]*\b(ias_\w+)\s*\(', code))
    assert defined == NAMES
    assert "ias_diag_env" not in code and not re.search(r"\basm\b", code)


def _refusal_args():
    """Host buffers that stand in for device memory: every call below returns before a launch could read them."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    return buf, p


def test_partials_count(lib):
    n = lib.ias_spectral_report_partials_count
    assert [n(F) for F in (1, 32, 33, 690)] == [1, 1, 2, 22]
    assert n(0) == IAS_ERR_ARG and n(-5) == IAS_ERR_ARG
    assert n(2 ** 31 - 1) == 2 ** 26


def test_spectral_report_refusals_come_before_any_launch(lib):
    _buf, p = _refusal_args()
    call = lib.ias_spectral_report

    def args(values=p, target=p, floors=p, dct=None, B=2, F=3, K=8, C=0, power=1, partials=p, out=p):
        return values, target, floors, dct, B, F, K, C, power, partials, out, None
    for name in ("values", "target", "floors", "partials", "out"):
        assert call(*args(**{name: None})) == IAS_ERR_ARG, name
    for kw in (dict(B=0), dict(B=-1), dict(F=0), dict(K=0), dict(power=0), dict(power=3), dict(dct=p, C=0, K=64)):
        assert call(*args(**kw)) == IAS_ERR_ARG, kw
    for kw in (dict(B=65536), dict(K=2049), dict(dct=p, C=33, K=64), dict(dct=p, C=8, K=8), dict(dct=p, C=9, K=8),
               dict(dct=p, C=13, K=257)):
        assert call(*args(**kw)) == IAS_ERR_UNSUPPORTED, kw


def test_wrapper_refusals_need_no_device():
    import torch
    from inverse_audio_synthesis_amd.report import spectral_report
    v = torch.zeros((2, 3, 8))
    fl = torch.ones(2)
    for bad in (dict(values=v.double()), dict(values=v[:, :, ::2]), dict(target_values=v[:1]), dict(floor_rows=fl[:1]),
                dict(floor_rows=fl.double()), dict(power=3), dict(power=1.5), dict(dct=torch.zeros((2, 7))),
                dict(dct=torch.zeros((8, 8))), dict(values=torch.zeros((2, 3, 2049)), target_values=torch.zeros((2, 3, 2049)))):
        kw = dict(values=v, target_values=v, floor_rows=fl, power=1, dct=None)
        kw.update(bad)
        with pytest.raises(ValueError, match="spectral_report"):
            spectral_report(**kw)


def test_as_records_writes_nan_as_none():
    import json
    import torch
    from inverse_audio_synthesis_amd.report import MatchReport
    z = torch.tensor([0.5, 1.5], dtype=torch.float64)
    rep = MatchReport(lsd_db=z, spectral_convergence=z, logmel_l1_db=z, mcd_db=z, frames=torch.tensor([3, 4]),
                      mel_frames=torch.tensor([2, 2]), envelope_db=z,
                      f0_cents=torch.tensor([float("nan"), -12.5], dtype=torch.float64), voiced=torch.tensor([False, True]))
    recs = rep.as_records()
    assert len(recs) == 2 and len(recs[0]) == 9
    assert recs[0]["f0_cents"] is None and recs[0]["voiced"] is False and recs[1]["f0_cents"] == -12.5
    assert recs[1]["frames"] == 4 and isinstance(recs[1]["frames"], int)
    assert json.loads(json.dumps(recs, allow_nan=False)) == recs

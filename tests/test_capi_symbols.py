"""The C-ABI library builds, loads, and exports every symbol include/ias_hip.h declares (no compute)."""
import ctypes
import os
import re

from conftest import ROOT


def _declared():
    text = open(os.path.join(ROOT, "include", "ias_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ias_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_exported(lib):
    from inverse_audio_synthesis_amd import _lib
    names = _declared()
    assert len(names) >= 9
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), f"{n} declared in include/ias_hip.h but not exported"
        assert n in _lib.SYMBOLS, f"{n} has no ctypes prototype in _lib.SYMBOLS"
    for n in _lib.SYMBOLS:
        assert n in names, f"{n} bound in _lib.py but not declared in include/ias_hip.h"


_P, _I, _LL, _ULL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong
_F, _D = ctypes.c_float, ctypes.c_double
# Written out by hand from the C declarations: between them every type _lib.parse_prototypes maps.
PINNED = {
    "ias_stft": (_I, [_P] * 8 + [_I] + [_P] * 5 + [_I] * 7 + [_F, _P]),      # 23 arguments, a float among ints
    "ias_evolve_sample": (_I, [_P, _P, _P, _I, _I, _I, _I, _LL, _ULL, _LL, _P, _P]),
    "ias_reduce_partials": (_I, [_P, _LL, _P, _D, _P, _P]),
    "ias_voice_workspace_bytes": (_LL, [_I, _I, _I]),
    "ias_reduce_partials_multi": (_I, [_P, _I, _P]),                        # const IasReduceItem*
    "ias_version": (_I, []),                                                # (void)
}
PINNED_DIAG = {"ias_vicreg_set_form": (_I, [_I])}


def test_prototypes_derived_from_the_headers_match_pinned_ones():
    from inverse_audio_synthesis_amd import _lib
    for table, pinned in ((_lib.SYMBOLS, PINNED), (_lib.DIAG_SYMBOLS, PINNED_DIAG)):
        for name, (res, args) in pinned.items():
            got_res, got_args = table[name]
            assert got_res is res, name
            assert len(got_args) == len(args), name
            for i, (g, a) in enumerate(zip(got_args, args)):
                assert g is a, f"{name}: argument {i} is bound as {g.__name__}, the declaration says {a.__name__}"
    assert len(PINNED["ias_stft"][1]) == 23
    assert len(_lib.SYMBOLS) == 120 and not set(_lib.SYMBOLS) & set(_lib.DIAG_SYMBOLS)   # the diag header's #include is not followed


def test_prototype_parser_is_strict():
    import pytest
    from inverse_audio_synthesis_amd._lib import parse_prototypes
    ok = "/* int ias_no(short a); */ int ias_a(const float* const* x, unsigned long long seed, double d, void* stream); // int ias_b(\n"
    assert parse_prototypes(ok) == {"ias_a": (_I, [_P, _ULL, _D, _P])}
    for bad in ("int ias_a(int n, short s);",                  # parameter type outside the mapping
                "int ias_a(unsigned n);",
                "int ias_a(long n);",
                "int ias_a(int);",                             # unnamed: `long long` could not be told from `long n`
                "int ias_a();",
                "float ias_a(int n);",                         # return type outside the mapping
                "unsigned long long ias_a(int n);",
                "const char* ias_a(int n);",
                "int ias_a(int (*cb)(int), int n);",           # forms it cannot fully match
                "int ias_a(int n) __attribute__((pure));",
                "static inline int ias_a(int n) { return n; }",
                "int ias_a(int n[4]);",
                "int ias_a(int n); int ias_a(int n);"):
        with pytest.raises(ValueError, match="ias_a"):
            parse_prototypes(bad)


_CSRC = os.path.join(ROOT, "inverse-audio-synthesis_amd", "csrc")


def _code(path):
    text = open(path).read()
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)


def _reaches(path, target, seen):
    """does `path` include `target`, directly or through its quoted includes (resolved relative to the including file)?"""
    for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', _code(path), re.M):
        p = os.path.normpath(os.path.join(os.path.dirname(path), inc))
        if p == target or (p not in seen and os.path.exists(p) and not seen.add(p) and _reaches(p, target, seen)):
            return True
    return False


def test_every_file_that_defines_an_entry_point_is_compiled_against_its_declaration():
    """With C linkage nothing but the compiler compares a definition with include/ias_hip.h, and only where it sees both:
    every .hip file with an extern "C" definition includes the header (through csrc/ias_common.h), and none declares an
    ias_* entry point by hand."""
    header = os.path.join(ROOT, "include", "ias_hip.h")
    files = sorted(f for f in os.listdir(_CSRC) if f.endswith(".hip"))
    defining = [f for f in files if re.search(r'extern\s+"C"[^;{]*\{', _code(os.path.join(_CSRC, f)))]
    assert len(defining) >= 23
    for f in defining:
        assert _reaches(os.path.join(_CSRC, f), header, set()), f"{f} defines extern \"C\" functions without include/ias_hip.h"
    for f in files:
        decl = re.findall(r'extern\s+"C"[^;{]*\bias_\w+\s*\([^;{]*;', _code(os.path.join(_CSRC, f)))
        assert not decl, f"{f} re-declares {decl}"


def test_version_and_arg_checks(lib):
    assert lib.ias_version() >= 100
    # pure host-side argument validation (no GPU touched)
    assert lib.ias_pqmf_out_len(176400, 3, 63) == 58800
    assert lib.ias_pqmf_out_len(16000, 3, 63) == 5334
    assert lib.ias_pqmf_out_len(176400, 64, 63) == 2757
    assert lib.ias_voice_workspace_bytes(128, 176400, 1764) > 128 * 5 * 1764 * 4
    assert lib.ias_voice_workspace_bytes(0, 10, 10) < 0


def test_voice_spec_tables_agree():
    from oracle import synth_spec as a
    from inverse_audio_synthesis_amd import voice_spec as b
    assert a.PARAMS == b.PARAMS and a.NPARAMS == b.NPARAMS == 78
    assert (a.CONTROL_RATE, a.EPS, a.NOISE_SEED, a.LFO_EXPONENT) == (b.CONTROL_RATE, b.EPS, b.NOISE_SEED, b.LFO_EXPONENT)


def _declared_in(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ias_[a-z0-9_]+)\s*\(", text)))


def test_product_library_reads_no_environment_and_keeps_no_switch(lib):
    """"reentrant; no global state except read-only tap tables".  The product library does not import
    getenv, contains none of the IAS_* switch names, and does not export the process-wide ias_vicreg_set_form; the
    sources reach the environment only through ias_diag_env(), which is a constant outside -DIAS_DIAG builds."""
    import subprocess
    from inverse_audio_synthesis_amd import _lib
    syms = subprocess.run(["nm", "-D", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "getenv" not in syms
    assert "ias_vicreg_set_form" not in syms
    blob = open(_lib.LIB_PATH, "rb").read()
    for name in (b"IAS_STFT_MFMA", b"IAS_VICREG_DXD", b"IAS_VOICE_PERCU", b"IAS_PQMF_VALU", b"IAS_STFT_V1", b"IAS_BN_UNFUSED"):
        assert name not in blob, name
    csrc = os.path.join(ROOT, "inverse-audio-synthesis_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if f.endswith(".hip"):
            assert "getenv" not in open(os.path.join(csrc, f)).read(), f


# kernels only a diagnostic switch launches (the site table of DESIGN.md section 1), as the prefix of their host stub
DIAG_ONLY_KERNELS = (
    "stft2_kernel<4,", "stft2_kernel<5,", "stft2_kernel<10,",                   # IAS_STFT2_WAVES
    "stft_kernel<10, 10,", "stft_kernel<10, 8,", "stft_kernel<11, 4,",          # IAS_STFT_WAVES
    "stft_grad_wave_kernel<9, false, true,",                                    # IAS_STFT_V1 (spans of linear bins, n_fft 512)
    "stft_mfma_kernel<",                                                        # IAS_STFT_MFMA
    "pqmf_analysis_mod_kernel<",                                                # IAS_PQMF_MOD_WINDOW
    "stem_bwd_weight_kernel<",                                                  # IAS_STEM_GW_LDS
    "voice_control_fused_kernel(",                                              # IAS_VOICE_CTRL=fused
)
# kernels the product dispatch names where a diagnostic alternative stands in front of them
PRODUCT_KERNELS = (
    "stft2_kernel<8, true, 1, 1>", "stft2_kernel<8, false, 2, 2>", "stft2h_kernel<8, 1>",
    "stft_kernel<10, 4,", "stft_kernel<11, 12,", "stft_kernel<9, 4,",
    "stft_grad_wave_kernel<9, true, true,", "stft_grad_wave_kernel<9, false, false,", "stft_grad512_kernel<8, false>",
    "pqmf_analysis_mods_kernel<true>", "pqmf_analysis_mods_kernel<false>",
    "stem_bwd_weight_stage_kernel<3, 16, 5, 2>", "stem_bwd_weight_mfma_kernel<3, 16>",
    "voice_env_kernel(", "voice_lfo_kernel(", "voice_modmix_kernel(",
)


def _device_stubs(path):
    import subprocess
    out = subprocess.run(["nm", "-C", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split("__device_stub__", 1)[1] for l in out.split("\n") if "__device_stub__" in l}


def test_product_library_compiles_only_the_kernels_its_dispatch_reaches(lib):
    """csrc/ias_common.h: a launch only a diagnostic switch reaches stands inside `if constexpr (kIasDiag)`, so the product
    library holds neither the host stub nor the device code of such a kernel; the diagnostic library holds every kernel
    of the product library and the diagnostic ones on top."""
    from inverse_audio_synthesis_amd import _lib
    _lib.load_diag()
    product, diag = _device_stubs(_lib.LIB_PATH), _device_stubs(_lib.DIAG_LIB_PATH)
    assert len(product) > 100 and len(diag) > len(product)
    for prefix in DIAG_ONLY_KERNELS:
        assert not [s for s in product if s.startswith(prefix)], f"{prefix} is in the product library"
        assert [s for s in diag if s.startswith(prefix)], f"{prefix} is not in the diagnostic library"
    for prefix in PRODUCT_KERNELS:
        assert [s for s in product if s.startswith(prefix)], f"{prefix} is not in the product library"
        assert [s for s in diag if s.startswith(prefix)], f"{prefix} is not in the diagnostic library"
    assert product <= diag, sorted(product - diag)


def test_diagnostic_library_exports_the_product_abi_plus_its_own(lib):
    from inverse_audio_synthesis_amd import _lib
    diag = _lib.load_diag()            # binds every product symbol and every diagnostic-only symbol, or raises
    extra = _declared_in("ias_hip_diag.h")
    assert extra == sorted(_lib.DIAG_SYMBOLS) == ["ias_vicreg_set_form"]
    assert diag.ias_version() == lib.ias_version()
    assert diag.ias_vicreg_set_form(7) < 0 and diag.ias_vicreg_set_form(-1) == 0

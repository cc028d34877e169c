"""ctypes binding of the C-ABI HIP library (``csrc/libias_hip.so``, declared in ``include/ias_hip.h``).

The product path has no CPU fallback: if the library is missing or a call returns a
non-zero status, an exception is raised.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# IAS_HIP_LIB: developer override used by scripts/diag to time alternative builds of the same C ABI
LIB_PATH = os.environ.get("IAS_HIP_LIB") or os.path.join(_HERE, "csrc", "libias_hip.so")

_ERRORS = {
    -1: "IAS_ERR_ARG (bad pointer or dimension)",
    -2: "IAS_ERR_UNSUPPORTED (shape outside the kernel's limits)",
    -3: "IAS_ERR_LAUNCH (HIP launch failed)",
    -4: "IAS_ERR_WORKSPACE (workspace too small)",
}

_INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
_VALUE_TYPES = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong,
                "float": ctypes.c_float, "double": ctypes.c_double}
_RETURN_TYPES = ("int", "long long")


def parse_prototypes(text):
    """name -> (restype, argtypes) of every `int | long long ias_*( ... );` declaration in the text of a C header.
    Comments and preprocessor lines are dropped (an #include is not followed); a pointer of any kind is a c_void_p, a
    named value one of _VALUE_TYPES, `(void)` no arguments.  Strict: an ias_* declaration of another form, return type
    or parameter type raises ValueError with the declaration in its message -- a prototype is never guessed."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r'^\s*#.*$|extern\s+"C"\s*\{', " ", text, flags=re.M)
    table = {}
    for stmt in text.split(";"):
        if not re.search(r"\bias_\w*\s*\(", stmt):
            continue
        decl = " ".join(stmt.split())
        m = re.fullmatch(r"([\w ]+?) (ias_\w+) ?\((.*)\)", decl)
        if not m:
            raise ValueError(f"cannot parse the declaration `{decl};`")
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        if ret not in _RETURN_TYPES:
            raise ValueError(f"return type `{ret}` of `{decl};` is not one of {_RETURN_TYPES}")
        args = []
        for param in ([] if params == "void" else params.split(",")):
            if re.fullmatch(r"[\w ]+\*[\w *]*", param.strip()):
                args.append(ctypes.c_void_p)
                continue
            v = re.fullmatch(r"(?:const )?([a-z ]+) \w+", param.strip())
            if not v or v.group(1) not in _VALUE_TYPES:
                raise ValueError(f"parameter `{param.strip()}` of `{decl};` has a type outside {sorted(_VALUE_TYPES)}")
            args.append(_VALUE_TYPES[v.group(1)])
        if name in table:
            raise ValueError(f"{name} is declared twice")
        table[name] = (_VALUE_TYPES[ret], args)
    return table


def _header_prototypes(header):
    with open(os.path.join(_INCLUDE, header)) as f:
        return parse_prototypes(f.read())


# name -> (restype, argtypes), read from the declarations the kernel files are compiled against (csrc/ias_common.h
# includes all five headers): the product ABI, the symbols only the diagnostic library exports, and the entry points of
# the match report (report.py), of the tied fit (match.py: tied_adam_step) and of the output gain (match.py: apply_gain,
# solve_gain), which both libraries export.
SYMBOLS = _header_prototypes("ias_hip.h")
DIAG_SYMBOLS = _header_prototypes("ias_hip_diag.h")
REPORT_SYMBOLS = _header_prototypes("ias_hip_report.h")
TIED_SYMBOLS = _header_prototypes("ias_hip_tied.h")
GAIN_SYMBOLS = _header_prototypes("ias_hip_gain.h")
DIAG_LIB_PATH = os.path.join(_HERE, "csrc", "libias_hip_diag.so")

_lib = None
_diag = None


class HipLibraryMissing(RuntimeError):
    pass


def load():
    """Load libias_hip.so (once).  Raises HipLibraryMissing if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryMissing(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C inverse-audio-synthesis_amd/csrc`.  There is no CPU fallback."
        )
    _lib = _bind(_bind(_bind(_bind(ctypes.CDLL(LIB_PATH), SYMBOLS), REPORT_SYMBOLS), TIED_SYMBOLS), GAIN_SYMBOLS)
    return _lib


def _bind(lib, table):
    for name, (res, args) in table.items():
        fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    return lib


def load_diag():
    """The diagnostic build of the same sources (csrc/libias_hip_diag.so, -DIAS_DIAG: environment switches live,
    superseded kernels and ``ias_vicreg_set_form`` compiled in; include/ias_hip_diag.h).  The rule of the split is at the
    top of csrc/ias_common.h: what only a switch reaches is launched inside ``if constexpr (kIasDiag)``, so the product
    library (262 kernels) holds no kernel its dispatch cannot reach and this one holds those and 39 more (301; the
    inventory is pinned by tests/test_capi_symbols.py).  A SEPARATE library instance:
    nothing the package does goes through it unless a test or a diagnostic script asks for it (``use_library``)."""
    global _diag
    if _diag is None:
        if not os.path.exists(DIAG_LIB_PATH):
            raise HipLibraryMissing(f"{DIAG_LIB_PATH} not found: `make -C inverse-audio-synthesis_amd/csrc`")
        lib = ctypes.CDLL(DIAG_LIB_PATH)
        for table in (SYMBOLS, REPORT_SYMBOLS, TIED_SYMBOLS, GAIN_SYMBOLS, DIAG_SYMBOLS):
            _bind(lib, table)
        _diag = lib
    return _diag


class use_library:
    """``with use_library(load_diag()): ...`` -- route every call of the package through another build of the C ABI for the
    duration of the block (tests and diagnostics that compare kernel variants; never used by the package itself)."""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        global _lib
        load()
        self.saved, _lib = _lib, self.lib
        return self.lib

    def __exit__(self, *exc):
        global _lib
        _lib = self.saved


def check(status, what):
    if status != 0:
        raise RuntimeError(f"{what} failed: {_ERRORS.get(status, status)}")


def ptr(t):
    """Device pointer of a contiguous CUDA(HIP) tensor, or None."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("inverse-audio-synthesis_amd kernels need tensors on a ROCm device (no CPU fallback)")
    if not t.is_contiguous():
        raise RuntimeError("tensor must be contiguous")
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_f32(*ts):
    for t in ts:
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError(f"expected float32, got {t.dtype}")

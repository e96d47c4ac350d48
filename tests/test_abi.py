"""CPU-side checks of the drop-in boundary: the shared library loads and exports every symbol
that include/sl_hip.h declares, and fails loudly (no fallback) when there is no GPU."""

import ctypes as C
import os
import re

import pytest

from conftest import ROOT, _have_gpu
from safe_learning_amd import _hip


def _declared_symbols():
    with open(os.path.join(ROOT, "include", "sl_hip.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sl_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_match_binding():
    assert _declared_symbols() == sorted(_hip.EXPORTS)


def test_library_exports_every_declared_symbol():
    if not os.path.exists(_hip.LIB_PATH):
        from safe_learning_amd._build import build
        build()
    lib = C.CDLL(_hip.LIB_PATH)
    for name in _declared_symbols():
        assert hasattr(lib, name), "libslhip.so does not export %s" % name
    lib.sl_version.restype = C.c_int
    assert lib.sl_version() >= 100


def test_library_exports_nothing_else():
    """-fvisibility=hidden + SL_API: the dynamic symbol table defines the C ABI and nothing of the
    C++ internals (launchers, device stubs, sl_fail)."""
    import subprocess
    if not os.path.exists(_hip.LIB_PATH):
        from safe_learning_amd._build import build
        build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _hip.LIB_PATH], text=True)
    defined = sorted(line.split()[-1] for line in out.splitlines() if " T " in line or " t " in line)
    assert defined == _declared_symbols(), sorted(set(defined) ^ set(_declared_symbols()))


# every ctypes.Structure of _hip.py and the C type it mirrors
STRUCTS = {"GridDesc": "sl_grid_desc", "PolicyDesc": "sl_policy_desc", "DynamicsDesc": "sl_dynamics_desc",
           "ValueDesc": "sl_value_desc", "LipschitzDesc": "sl_lipschitz_desc", "ModelDesc": "sl_model_desc",
           "Key": "sl_key", "GpKernelFactor": "sl_gp_kernel_factor", "GpKernel": "sl_gp_kernel",
           "SuccessorCacheStats": "sl_successor_cache_stats", "ValueSolveStats": "sl_value_solve_stats"}


def test_struct_layout_matches_header():
    """ctypes mirrors must have the C sizes and field offsets (compiled check with the host compiler)."""
    import subprocess
    import tempfile
    mirrors = sorted(name for name, obj in vars(_hip).items()
                     if isinstance(obj, type) and issubclass(obj, C.Structure) and obj is not C.Structure)
    assert mirrors == sorted(STRUCTS), "a Structure of _hip.py without its C name in STRUCTS"
    labels, expected, lines = [], [], []
    for name, cname in STRUCTS.items():
        mirror = getattr(_hip, name)
        labels.append("sizeof(%s)" % cname)
        expected.append(C.sizeof(mirror))
        lines.append('printf("%%zu\\n", sizeof(%s));' % cname)
        for field, _ in mirror._fields_:
            labels.append("%s.%s" % (cname, field))
            expected.append(getattr(mirror, field).offset)
            lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, field))
    lines.append('printf("%zu\\n", sizeof(sl_sweep_result));')
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "sl_hip.h"\nint main(void) {\n%s\nreturn 0;\n}\n'
           % "\n".join(lines))
    with tempfile.TemporaryDirectory() as tmp:
        c = os.path.join(tmp, "layout.c")
        with open(c, "w") as f:
            f.write(src)
        exe = os.path.join(tmp, "layout")
        subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), c, "-o", exe])
        numbers = [int(v) for v in subprocess.check_output([exe]).split()]
    assert len(numbers) == len(expected) + 1
    for label, got, want in zip(labels, numbers, expected):
        assert got == want, "%s: C %d, ctypes %d" % (label, got, want)
    assert numbers[-1] == 8 * _hip.RESULT_WORDS


def _header_prototypes():
    """{name: (return type, [argument types])} of every ``SL_API`` prototype, as C text without the
    argument names."""
    with open(os.path.join(ROOT, "include", "sl_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"SL_API\s+([\w\s\*]+?)\b(sl_\w+)\s*\(([^)]*)\)\s*;", text):
        args = [" ".join(a.split()) for a in args.split(",")]
        if args == ["void"]:
            args = []
        out[name] = (" ".join(ret.split()), [re.sub(r"\s*\w+$", "", a) for a in args])   # (without its name)
    return out


def _same_class(ctype, cdecl):
    """One argument: does the ctypes type pass what the C declaration expects?"""
    if "*" in cdecl:
        return ctype in (C.c_void_p, C.c_char_p) or issubclass(ctype, C._Pointer)
    base = cdecl.replace("const ", "").strip()
    if base in ("int", "int32_t"):
        return ctype is C.c_int and C.sizeof(ctype) == 4
    if base in ("int64_t", "uint64_t"):
        return ctype in (C.c_int64, C.c_uint64)
    if base == "double":
        return ctype is C.c_double
    if base == "sl_key":
        return ctype is _hip.Key
    raise AssertionError("argument type %r of sl_hip.h is not in the test's table" % cdecl)


def test_signatures_match_header():
    """Every prototype of the header against ``_hip.SIGNATURES``: the names, the number of arguments
    and the class of every argument and of the return value."""
    protos = _header_prototypes()
    assert sorted(protos) == sorted(_hip.SIGNATURES) == _declared_symbols()
    for name, (ret, args) in protos.items():
        restype, argtypes = _hip.SIGNATURES[name]
        assert {"int": C.c_int, "const char*": C.c_char_p}[ret] is restype, name
        assert len(args) == len(argtypes), "%s: %d arguments in the header, %d bound" % (name, len(args), len(argtypes))
        for k, (cdecl, ctype) in enumerate(zip(args, argtypes)):
            assert _same_class(ctype, cdecl), "%s, argument %d: %s bound as %s" % (name, k, cdecl, ctype.__name__)


class _StandIn(object):
    """A library object with a settable function per name, like ``ctypes.CDLL`` gives."""

    def __init__(self, names):
        for name in names:
            fn = type("fn", (), {"__call__": lambda self, ctx: b"what went wrong"})()
            fn.__name__ = name
            setattr(self, name, fn)


def _bound_as_declared(lib, name):
    restype, argtypes = _hip.SIGNATURES[name]
    return getattr(lib, name).restype is restype and getattr(lib, name).argtypes == list(argtypes)


def test_loader_binds_every_symbol_or_names_the_missing_one(monkeypatch):
    monkeypatch.delenv("SL_LIB_PATH", raising=False)
    lib = _hip._bind(_StandIn(_hip.SIGNATURES))
    for name in _hip.SIGNATURES:
        assert _bound_as_declared(lib, name), name
    with pytest.raises(_hip.HipEngineError, match=r"\bsl_value_solve\b"):
        _hip._bind(_StandIn(n for n in _hip.SIGNATURES if n != "sl_value_solve"))


def test_loader_skips_symbols_a_development_library_lacks(monkeypatch):
    monkeypatch.setenv("SL_LIB_PATH", "/somewhere/libslhip_dev.so")
    lacking = ("sl_value_solve", "sl_values")
    lib = _hip._bind(_StandIn(n for n in _hip.SIGNATURES if n not in lacking))
    for name in _hip.SIGNATURES:
        assert not hasattr(lib, name) if name in lacking else _bound_as_declared(lib, name), name


def test_loader_makes_a_failed_call_raise(monkeypatch):
    """Every entry point that takes a context and returns a status raises on a status other than 0,
    with the text ``Context.check`` gives; the two whose caller reads the status do not."""
    monkeypatch.delenv("SL_LIB_PATH", raising=False)
    lib = _hip._bind(_StandIn(_hip.SIGNATURES))
    for name, (restype, argtypes) in _hip.SIGNATURES.items():
        fn = getattr(lib, name)
        if restype is C.c_int and argtypes[:1] == (C.c_void_p,) and name not in _hip.UNCHECKED:
            assert fn.errcheck(0, fn, (None,)) == 0
            with pytest.raises(_hip.HipEngineError) as err:
                fn.errcheck(-1, fn, (None,))
            assert str(err.value) == "%s failed (-1): what went wrong" % name
        else:
            assert not hasattr(fn, "errcheck"), name
    assert sorted(n for n in _hip.SIGNATURES if not hasattr(getattr(lib, n), "errcheck")) == [
        "sl_comm_unique_id", "sl_ctx_create", "sl_ctx_destroy", "sl_gp_append_point", "sl_last_error",
        "sl_last_kernel", "sl_version"]


@pytest.mark.skipif(_have_gpu(), reason="only meaningful on a GPU-less host")
def test_no_cpu_fallback():
    import safe_learning_amd as sl
    import numpy as np
    grid = sl.GridWorld([[-1, 1]], 5)
    with pytest.raises(sl.HipEngineError):
        sl.Lyapunov(grid, sl.QuadraticFunction([[1.0]]), sl.LinearSystem((np.array([[1., 1.]]),)),
                    0.4, 0.3, 0.1, sl.LinearSystem((np.array([[-0.1]]),)))


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "safe_learning_amd")
    for dirpath, _, files in os.walk(pkg):
        for name in files:
            if name.endswith((".py", ".hip", ".h", ".cpp")):
                with open(os.path.join(dirpath, name)) as f:
                    text = f.read()
                assert not re.search(r"^\s*(import|from)\s+oracle\b", text, flags=re.M), name
                assert "hostsim" not in text or name == "sl_model.h", name

"""C-ABI checks that run without a GPU: the shared library loads and
exports every symbol include/pam.h declares; host-side queries work."""
import os
import re

import ctypes
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pam.h")
LIB = os.path.join(ROOT, "pylops_mpi_amd", "libpam.so")


def header_symbols():
    src = open(HEADER).read()
    # function declarations: "int pam_xxx(" / "int64_t pam_xxx("
    return sorted(set(re.findall(r"\b(?:int|int64_t)\s+(pam_\w+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.skip("libpam.so not built (run __graft_entry__.build())")
    return ctypes.CDLL(LIB)


def test_header_lists_symbols():
    syms = header_symbols()
    assert "pam_fd_apply" in syms and "pam_dot" in syms
    assert len(syms) >= 14


def test_all_header_symbols_exported(lib):
    for sym in header_symbols():
        assert hasattr(lib, sym), f"{sym} missing from libpam.so"


def test_host_queries(lib):
    lib.pam_version.restype = ctypes.c_int64
    lib.pam_reduce_ws_elems.restype = ctypes.c_int64
    lib.pam_fd_halo_width.restype = ctypes.c_int64
    lib.pam_fd_halo_width.argtypes = [ctypes.c_int]
    assert lib.pam_version() == 1
    assert lib.pam_reduce_ws_elems() >= 256
    assert [lib.pam_fd_halo_width(op) for op in range(14)] == \
        [1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2]
    assert lib.pam_fd_halo_width(99) < 0


def test_ffi_binding_covers_header():
    import sys
    sys.path.insert(0, ROOT)
    from pylops_mpi_amd import _ffi
    for sym in header_symbols():
        assert sym in _ffi._SIGS, f"{sym} not bound in _ffi"


_CTYPE_OF = {"void*": ctypes.c_void_p, "const void*": ctypes.c_void_p,
             "int64_t": ctypes.c_int64, "int": ctypes.c_int,
             "double": ctypes.c_double}


def header_declarations():
    """{name: ([argument ctypes], return ctype)} parsed from pam.h."""
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    decls = {}
    for ret, name, args in re.findall(
            r"\b(int64_t|int)\s+(pam_\w+)\s*\(([^)]*)\)\s*;", src):
        argtypes = []
        for arg in args.split(","):
            arg = " ".join(arg.split())
            if arg == "void":
                continue
            # "const void* x" -> type "const void*", name "x"
            ctype, argname = arg.replace("*", "* ").rsplit(None, 1)
            assert re.fullmatch(r"\w+", argname), arg
            argtypes.append(_CTYPE_OF[ctype.replace(" *", "*")])
        decls[name] = (argtypes, _CTYPE_OF[ret])
    return decls


def test_ffi_signatures_match_header():
    """Every _ffi._SIGS entry restates its pam.h declaration exactly —
    a c_int against an int64_t would corrupt arguments silently."""
    import sys
    sys.path.insert(0, ROOT)
    from pylops_mpi_amd import _ffi
    decls = header_declarations()
    assert sorted(decls) == header_symbols()
    for name, sig in decls.items():
        assert _ffi._SIGS[name] == sig, f"{name}: _SIGS disagrees with pam.h"
    assert sorted(_ffi._SIGS) == sorted(decls), \
        "_ffi._SIGS binds names pam.h does not declare"

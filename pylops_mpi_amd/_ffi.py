"""ctypes binding of the pam C-ABI (include/pam.h -> libpam.so).

The product compute path goes EXCLUSIVELY through this library; there is no
CPU fallback.  If the extension is missing or fails to load, every compute
op raises loudly.
"""
import ctypes
import os

import torch

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                         "libpam.so")
_lib = None
_load_error = None

F64, F32, C128, C64 = 0, 1, 2, 3  # PAM_* dtype codes
_CODES = {torch.float64: F64, torch.float32: F32,
          torch.complex128: C128, torch.complex64: C64}

# include/pam.h, argument for argument (tests/test_cabi.py pins the two
# together): P pointer / stream, L int64_t, I int, D double
P, L, I, D = (ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
              ctypes.c_double)
_SIGS = {
    "pam_version": ([], L),
    "pam_reduce_ws_elems": ([], L),
    "pam_fill": ([P, P, L, D, I], I),
    "pam_neg": ([P, P, P, L, I], I),
    "pam_add": ([P, P, P, P, L, I], I),
    "pam_sub": ([P, P, P, P, L, I], I),
    "pam_mul": ([P, P, P, P, L, I], I),
    "pam_scale": ([P, P, P, D, L, I], I),
    "pam_axpy": ([P, P, P, D, L, I], I),
    "pam_xpby": ([P, P, P, D, L, I], I),
    "pam_axpy_d": ([P, P, P, P, D, L, I], I),
    "pam_xpby_d": ([P, P, P, P, D, L, I], I),
    "pam_scalar_alpha": ([P, P, P, P, D], I),
    "pam_scalar_div": ([P, P, P, P], I),
    "pam_dot": ([P, P, P, L, P, P, I], I),
    "pam_cmul": ([P, P, P, P, L, I], I),
    "pam_cscale": ([P, P, P, D, D, L, I], I),
    "pam_conj": ([P, P, P, L, I], I),
    "pam_thresh": ([P, P, P, L, I, D, I], I),
    "pam_cdot": ([P, P, P, L, I, P, P, I], I),
    "pam_cgemm_batched": ([P, P, P, P, L, L, L, L, L, L, L, I, I, I], I),
    "pam_ctranspose": ([P, P, P, L, L, I, I], I),
    "pam_rfft_strided": ([P, P, P, L, L, I], I),
    "pam_irfft_strided": ([P, P, P, L, L, I], I),
    "pam_rfft_contig": ([P, P, P, L, L, I], I),
    "pam_irfft_contig": ([P, P, P, L, L, I], I),
    "pam_unzip_t": ([P, P, P, L, L, I], I),
    "pam_zip_t": ([P, P, P, L, L, I], I),
    "pam_unzip": ([P, P, P, L, I], I),
    "pam_zip": ([P, P, P, L, I], I),
    "pam_gemm_batched": ([P, P, P, P, L, L, L, L, L, L, L, I, I, I], I),
    "pam_norm_local": ([P, P, L, I, D, P, P, I], I),
    "pam_group_shrink": ([P, I, L, P, P, P, P, P, P, P, P, P, P, P, P, D, L,
                          D, I], I),
    "pam_group_norm": ([P, L, P, P, P, P, L, P, P, I], I),
    "pam_gemv_ws_elems": ([L, L], L),
    "pam_gemv": ([P, I, P, P, P, L, L, P, I], I),
    "pam_gemm": ([P, P, P, P, L, L, L, L, L, L, I, I], I),
    "pam_gemm_kt": ([P, P, P, P, L, L, L, I, I], I),
    "pam_transpose": ([P, P, P, L, L, I], I),
    "pam_fd_halo_width": ([I], L),
    "pam_nsconv": ([P, I, P, P, P, L, L, L, L, L, D, D, I], I),
    "pam_conv1d": ([P, I, P, P, P, L, L, L, L, L, I, I], I),
    "pam_conv1d_variant": ([I, L, L, L], I),
    "pam_conv1d_tile_d": ([I, I, L], L),
    "pam_conv1d_tile_m": ([I, I], L),
    "pam_kirch": ([P, I, P, P, P, P, P, L, L, L, L, I], I),
    "pam_kirch_ws_elems": ([I, L, L, L, L, I], L),
    "pam_kirch_points": ([], L),
    "pam_kirch_chunk": ([L, L, L, L, I], L),
    "pam_kirch_variant": ([L, L, L, L, I], I),
    "pam_kirch_window": ([L, L, L, L, I], L),
    "pam_fd_serial": ([P, I, I, P, P, L, L, L, D, I], I),
    "pam_fd_apply": ([P, I, I, P, P, P, P, L, L, L, L, L, L, D, I], I),
    "pam_fd_variant": ([I, L, L, I], I),
    "pam_fd_band_rows": ([], L),
}


def lib():
    """The loaded C-ABI; raises ImportError if libpam.so is missing."""
    global _lib, _load_error
    if _lib is not None:
        return _lib
    if _load_error is not None:
        raise _load_error
    try:
        so = ctypes.CDLL(_LIB_PATH)
        for name, (argtypes, restype) in _SIGS.items():
            fn = getattr(so, name)
            fn.argtypes = argtypes
            fn.restype = restype
        ver = so.pam_version()
        if ver != 1:
            raise RuntimeError(f"pam ABI version mismatch: {ver}")
    except OSError as e:
        _load_error = ImportError(
            f"pam HIP extension not found/loadable at {_LIB_PATH} "
            f"(build it with __graft_entry__.build()): {e}")
        raise _load_error
    _lib = so
    return so


def available() -> bool:
    try:
        lib()
        return True
    except ImportError:
        return False


def checked(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"pam: {what} failed with code {rc}")


def dtype_code(torch_dtype) -> int:
    try:
        return _CODES[torch_dtype]
    except KeyError:
        raise TypeError(f"pam: unsupported dtype {torch_dtype}") from None

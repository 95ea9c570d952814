"""Tensor-level launch layer over the pam C-ABI (include/pam.h): one
small function per entry point the package uses, taking torch tensors and
plain Python scalars.  Streams, raw pointers, dtype codes, element counts
and return codes are handled HERE and nowhere else.  Before anything is
enqueued a launch checks, in this order:
  * dtypes — every tensor has the dtype the entry point expects (TypeError);
  * sizes — n / M,N,K / nr,nc ... are read off the tensors' shapes; operands
    that disagree raise ValueError (a wrong rank does too: it won't unpack);
  * outputs and in-place operands are contiguous (ValueError) — they are
    never copied, so a result cannot land in a temporary; inputs are made
    contiguous, the copy staying referenced until pam_* has returned;
  * all tensors sit on one device (ValueError) and, LAST, that device is a
    GPU (RuntimeError; then _ffi.lib() raises ImportError without libpam.so).
The stream is the current stream of that device.
"""
from functools import lru_cache

import torch
from torch import Tensor

from . import _ffi
from ._ffi import dtype_code as _code

_REAL_OF = {torch.complex128: torch.float64, torch.complex64: torch.float32}
_F64 = torch.float64


# ------------------------------------------------------------------ checks
# a complex array launched as its interleaved real view: (reals per
# element, code of the matching real type).  Valid for componentwise
# kernels only (add/sub/neg, REAL-alpha scale/axpy/xpby, real stencils).
_AS_REAL = {torch.complex128: (2, _ffi.F64), torch.complex64: (2, _ffi.F32)}


def _real_code(t):
    return _AS_REAL.get(t.dtype) or (1, _code(t.dtype))


def _typed(name, dtype, *ts):
    for t in ts:
        if t.dtype != dtype:
            raise TypeError(f"pam: {name}: expected {dtype}, got {t.dtype}")


def _sized(name, n, *ts):
    for t in ts:
        if t.numel() != n:
            raise ValueError(f"pam: {name}: operand of shape "
                             f"{tuple(t.shape)} should hold {n} elements")


def _shaped(name, shape, *ts):
    for t in ts:
        if t.shape != shape:
            raise ValueError(f"pam: {name}: operand has shape "
                             f"{tuple(t.shape)}, expected {tuple(shape)}")


def _dst(name, t):  # output / in-place operand: never copied
    if not t.is_contiguous():
        raise ValueError(
            f"pam: {name}: output / in-place operand must be contiguous "
            f"(shape {tuple(t.shape)}, strides {t.stride()})")
    return t


def _scalar(name, t, n=1):
    """Device scalar(s): float64, at least ``n`` contiguous elements."""
    if t.dtype != _F64 or t.numel() < n or not t.is_contiguous():
        _typed(name, _F64, t)
        if t.numel() < n:
            raise ValueError(f"pam: {name}: device scalar buffer holds "
                             f"{t.numel()} elements, expected at least {n}")
        _dst(name, t)
    return t


def require_device(*ts) -> int:
    """All tensors on ONE device, and that device a GPU: its index."""
    idx = ts[0].get_device()
    for t in ts:
        if t.get_device() != idx:
            raise ValueError(f"pam: tensors of one call sit on different "
                             f"devices ({ts[0].device} and {t.device})")
    if not ts[0].is_cuda:
        raise RuntimeError(
            "pam: compute ops require a CUDA (MI355X) device tensor — "
            "there is no CPU compute path")
    return idx


# torch.cuda.current_stream(idx).cuda_stream without building the Stream
# object: about 1 us per launch, which the launch-bound paths notice
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (
    lambda idx: torch.cuda.current_stream(idx).cuda_stream)


def _launch(idx, name, argv):
    rc = getattr(_ffi._lib or _ffi.lib(), name)(_raw_stream(idx), *argv)
    if rc:
        _ffi.checked(rc, name)


def _run(name, *args):
    """Call entry point ``name`` on the current stream of the tensors'
    device: tensors go by pointer, None as NULL, scalars as they are.
    ``args`` keeps every tensor (contiguous copies of inputs included)
    alive until the call has returned.  One pass: this is require_device
    plus pointer extraction."""
    argv, first = [], None
    for a in args:
        if isinstance(a, Tensor):
            if first is None:
                first, idx = a, a.get_device()
            elif a.get_device() != idx:
                require_device(first, a)
            a = a.data_ptr()
        argv.append(a)
    if not first.is_cuda:
        require_device(first)
    _launch(idx, name, argv)


def same_memory(a: Tensor, b: Tensor) -> bool:  # same start address
    return a.data_ptr() == b.data_ptr()


# ------------------------------------------------------------ element-wise
def _ew(name, y, ins, pre=(), post=(), as_real=True):
    """pam_X(stream, y, *ins, *pre, n, *post, dtype), same dtype and count
    all round; ``as_real`` launches complex arrays as their real view."""
    dtype, n = y.dtype, y.numel()
    for t in ins:
        if t.dtype != dtype or t.numel() != n:
            _typed(name, dtype, t)
            _sized(name, n, t)
    k, dt = _real_code(y) if as_real else (1, _code(dtype))
    _run(name, _dst(name, y), *[t.contiguous() for t in ins], *pre, k * n,
         *post, dt)


def neg(y, x):  # y = -x
    _ew("pam_neg", y, (x,))


def add(y, a, b):  # y = a + b
    _ew("pam_add", y, (a, b))


def sub(y, a, b):  # y = a - b
    _ew("pam_sub", y, (a, b))


def mul(y, a, b):
    """y = a * b (the complex product for complex dtypes)"""
    _ew("pam_cmul" if y.is_complex() else "pam_mul", y, (a, b),
        as_real=False)


def conj(y, x):
    _ew("pam_conj", y, (x,), as_real=False)


def scale(y, x, alpha: float):  # y = alpha * x, REAL alpha
    _ew("pam_scale", y, (x,), (float(alpha),))


def cscale(y, x, alpha: complex):  # y = alpha * x on complex arrays
    _ew("pam_cscale", y, (x,), (float(alpha.real), float(alpha.imag)),
        as_real=False)


def axpy(y, x, alpha: float):  # y += alpha * x, REAL alpha
    _ew("pam_axpy", y, (x,), (float(alpha),))


def xpby(y, x, beta: float):  # y = x + beta * y, REAL beta
    _ew("pam_xpby", y, (x,), (float(beta),))


def axpy_d(y, x, alpha_t, scale: float = 1.0):
    """y += scale * alpha_t[0] * x, alpha_t a float64 device scalar"""
    _ew("pam_axpy_d", y, (x,),
        (_scalar("pam_axpy_d", alpha_t), float(scale)))


def xpby_d(y, x, beta_t, scale: float = 1.0):
    """y = x + scale * beta_t[0] * y, beta_t a float64 device scalar"""
    _ew("pam_xpby_d", y, (x,), (_scalar("pam_xpby_d", beta_t), float(scale)))


def thresh(y, x, kind: int, t: float):  # 0 soft, 1 hard, 2 half; y may be x
    _ew("pam_thresh", y, (x,), post=(int(kind), float(t)), as_real=False)


_GROUP_MAX = 4          # PAM_GROUP_MAX pointer slots per operand


def _group(name, *seqs):
    """Component lists of one group launch: each 1 to 4 tensors, equally
    many, one dtype and one element count -> (ncomp, dtype, n)."""
    nc = len(seqs[0])
    if not 1 <= nc <= _GROUP_MAX or any(len(s) != nc for s in seqs):
        raise ValueError(f"pam: {name}: expected 1 to {_GROUP_MAX} "
                         f"components per operand, equally many; got "
                         f"{[len(s) for s in seqs]}")
    ts = [t for s in seqs for t in s]
    dtype, n = ts[0].dtype, ts[0].numel()
    _typed(name, dtype, *ts)
    _sized(name, n, *ts)
    return nc, dtype, n


def _slots(ts):  # pointers of the components, unused slots NULL
    return [t.data_ptr() for t in ts] + [None] * (_GROUP_MAX - len(ts))


def group_shrink(ys, xs, mode: int, thresh: float, shift=None,
                 beta: float = 1.0):
    """ys[c] = v[c] * s with v[c] = xs[c] (+ beta * shift[c]) and s from
    rho = sqrt(sum_c |v[c]|^2) at each index: mode 0 the L2,1 prox
    (rho - thresh)_+ / rho, mode 1 the projection min(1, thresh / rho).
    ys, xs, shift: sequences of 1 to 4 tensors; ys[c] may be xs[c]."""
    name = "pam_group_shrink"
    shift = () if shift is None else shift
    nc, dtype, n = _group(name, ys, xs, *((shift,) if len(shift) else ()))
    dt = _code(dtype)
    for y in ys:
        _dst(name, y)
    xs = [t.contiguous() for t in xs]
    shift = [t.contiguous() for t in shift]
    idx = require_device(*ys, *xs, *shift)
    if n:
        _launch(idx, name, (int(mode), nc, *_slots(ys), *_slots(xs),
                            *_slots(shift), float(beta), n, float(thresh),
                            dt))


def scalar_alpha(out, num, den, damp: float):
    """out[0] = |num[0] / (den[0] + damp * den[1])| on device"""
    name = "pam_scalar_alpha"
    _run(name, _scalar(name, out), _scalar(name, num), _scalar(name, den, 2),
         float(damp))


def scalar_div(out, num, den):
    """out[0] = |num[0] / den[0]| on device"""
    _run("pam_scalar_div",
         *[_scalar("pam_scalar_div", t) for t in (out, num, den)])


# -------------------------------------------------------------- reductions
_reduce_scratch = {}    # per device: (ws, out) float64 tensors


def _reduce(name, ins, extras, out, nout, pre=(), slots=0):
    """pam_X(stream, *pre, *ins, n, *extras, ws, out, dtype) -> out;
    ``out`` None selects the per-device cached result buffer, ``slots``
    pads the input pointers with NULLs."""
    dtype, n = ins[0].dtype, ins[0].numel()
    _typed(name, dtype, *ins)
    _sized(name, n, *ins)
    dt = _code(dtype)
    ins = [t.contiguous() for t in ins]
    if out is not None:
        _sized(name, nout, _scalar(name, out))
    idx = require_device(*ins, *(() if out is None else (out,)))
    if idx not in _reduce_scratch:
        nws, dev = int(_ffi.lib().pam_reduce_ws_elems()), ins[0].device
        _reduce_scratch[idx] = (torch.empty(2 * nws, dtype=_F64, device=dev),
                                torch.empty(2, dtype=_F64, device=dev))
    ws, cached = _reduce_scratch[idx]
    out = cached[:nout] if out is None else out
    ptrs = [t.data_ptr() for t in ins] + [None] * (slots - len(ins))
    _launch(idx, name, (*pre, *ptrs, n, *extras, ws.data_ptr(),
                        out.data_ptr(), dt))
    return out


def dot(x, y, out=None):
    """sum(x * y) in float64, real dtypes -> 1-element device tensor"""
    return _reduce("pam_dot", (x, y), (), out, 1)


def cdot(x, y, conjx: bool, out=None):
    """sum(x * y) or sum(conj(x) * y), complex -> (re, im) device tensor"""
    return _reduce("pam_cdot", (x, y), (1 if conjx else 0,), out, 2)


def norm_local(x, op: int, p: float, out=None):  # see pam_norm_local ops
    return _reduce("pam_norm_local", (x,), (int(op), float(p)), out, 1)


def group_norm(xs, out=None):
    """sum_i sqrt(sum_c |xs[c][i]|^2) in float64, xs a sequence of 1 to 4
    tensors -> 1-element device tensor"""
    nc, _, _ = _group("pam_group_norm", xs)
    return _reduce("pam_group_norm", tuple(xs), (), out, 1, pre=(nc,),
                   slots=_GROUP_MAX)


# ------------------------------------------------------- dense GEMV / GEMM
_gemv_scratch = {}      # per device, sized for the largest (nr, nc) seen


def gemv(y, A, x, trans: bool):
    """y = A @ x (trans false) or A^T @ x, row-major real A [nr, nc]"""
    name = "pam_gemv"
    nr, nc = A.shape
    _typed(name, A.dtype, x, y)
    _sized(name, nr if trans else nc, x)
    _sized(name, nc if trans else nr, y)
    _dst(name, y)
    A, x = A.contiguous(), x.contiguous()
    idx = require_device(y, A, x)
    need = int(_ffi.lib().pam_gemv_ws_elems(nr, nc))
    ws = _gemv_scratch.get(idx)
    if ws is None or ws.numel() < need:
        ws = _gemv_scratch[idx] = torch.empty(need, dtype=_F64,
                                              device=y.device)
    _launch(idx, name, (1 if trans else 0, A.data_ptr(), x.data_ptr(),
                        y.data_ptr(), nr, nc, ws.data_ptr(), _code(A.dtype)))


def gemm(C, A, B, accumulate: bool = False):
    """C (+)= A @ B for row-major A [M,K], B [K,N], C [M,N]"""
    if C.is_complex():      # the batched complex kernel with batch 1
        return gemm_batched(C[None], A[None], B[None], False, accumulate)
    (M, K), N = A.shape, B.shape[-1]
    _typed("pam_gemm", C.dtype, A, B)
    _shaped("pam_gemm", (K, N), B)
    _shaped("pam_gemm", (M, N), _dst("pam_gemm", C))
    _run("pam_gemm", A.contiguous(), B.contiguous(), C, M, N, K, K, N, N,
         1 if accumulate else 0, _code(C.dtype))


def gemm_batched(C, A, B, opa: bool = False, accumulate: bool = False):
    """C_b (+)= op(A_b) @ B_b over [batch, ., .] stacks; ``opa`` selects
    the (conjugate-)transpose, A_b then being [K, M]"""
    name = "pam_cgemm_batched" if C.is_complex() else "pam_gemm_batched"
    batch, d1, d2 = A.shape
    (K, M), N = ((d1, d2) if opa else (d2, d1)), B.shape[-1]
    _typed(name, C.dtype, A, B)
    _shaped(name, (batch, K, N), B)
    _shaped(name, (batch, M, N), _dst(name, C))
    _run(name, A.contiguous(), B.contiguous(), C, batch, M, N, K, M * K,
         K * N, M * N, 1 if opa else 0, 1 if accumulate else 0,
         _code(C.dtype))


def transpose(At, A, conj: bool = False):
    """At = A^T for row-major A [nr, nc]; complex dtypes: A^H when
    ``conj`` (the identity on reals)"""
    name = "pam_ctranspose" if A.is_complex() else "pam_transpose"
    nr, nc = A.shape
    _typed(name, A.dtype, At)
    _shaped(name, (nc, nr), _dst(name, At))
    flag = (1 if conj else 0,) if A.is_complex() else ()
    _run(name, A.contiguous(), At, nr, nc, *flag, _code(A.dtype))


# -------------------------------------- complex <-> real, real FFTs (MDC)
def _cplx_real(name, c, r):
    """Dtype pair of a (de)interleave / real-FFT launch."""
    if not c.is_complex():
        raise TypeError(f"pam: {name}: expected complex, got {c.dtype}")
    _typed(name, _REAL_OF[c.dtype], r)


def _zip(name, dst, src, cplx, real, transposed):
    """pam_(un)zip(_t), dst <- src: complex <-> real parts / (re, 0) pairs;
    ``transposed`` pairs complex (nt, m) with real (m, nt)."""
    name += "_t" if transposed else ""
    _cplx_real(name, cplx, real)
    if transposed:
        dims = nt, m = cplx.shape
        _shaped(name, (m, nt), real)
    else:
        dims = (cplx.numel(),)
        _sized(name, *dims, real)
    _run(name, _dst(name, dst), src.contiguous(), *dims, _code(cplx.dtype))


def unzip(dst_real, src_cplx, transposed=False):  # dst = real parts of src
    _zip("pam_unzip", dst_real, src_cplx, src_cplx, dst_real, transposed)


def zip(dst_cplx, src_real, transposed=False):  # dst = (src, 0) pairs
    _zip("pam_zip", dst_cplx, src_real, dst_cplx, src_real, transposed)


def _rfft(name, dst, src, cplx, real, contig):
    """pam_(i)rfft_{contig,strided}, dst <- src, unscaled: m transforms of
    nt real samples <-> nt//2+1 complex bins, along dim 1 of (m, .)
    arrays when ``contig``, else along dim 0 of (., m) arrays."""
    name += "_contig" if contig else "_strided"
    _cplx_real(name, cplx, real)
    m, nt = real.shape if contig else real.shape[::-1]
    _shaped(name, (m, nt // 2 + 1) if contig else (nt // 2 + 1, m), cplx)
    _run(name, src.contiguous(), _dst(name, dst), nt, m, _code(real.dtype))


def rfft(out_cplx, in_real, contig: bool):
    _rfft("pam_rfft", out_cplx, in_real, out_cplx, in_real, contig)


def irfft(out_real, in_cplx, contig: bool):     # may clobber in_cplx
    _rfft("pam_irfft", out_real, in_cplx, in_cplx, out_real, contig)


# ------------------------------------------------ stencils / convolution
@lru_cache(maxsize=None)
def fd_halo_width(op: int) -> int:  # neighbour planes read per side
    return int(_ffi.lib().pam_fd_halo_width(int(op)))


# shortest axis on which the edge fix-ups of an op are defined (include/pam.h,
# the table next to the op codes); every other op, and edge False: 1
_FD_EDGE_MIN = {4: 2, 5: 2, 6: 3, 7: 3, 12: 3, 13: 3}


def fd_min_rows(op: int, edge: bool) -> int:
    return _FD_EDGE_MIN.get(int(op), 1) if edge else 1


def _fd_too_short(name, op, n):  # edge is set
    return ValueError(
        f"pam: {name}: op {op} with edge needs an axis of at least "
        f"{fd_min_rows(op, True)} samples, got {n}")


def fd_apply(y, x, gf, gb, op: int, edge: bool, row0: int, nglob: int,
             rbegin: int, rend: int, coeff: float):
    """Stencil ``op`` along axis 0 of the [nloc, m] block ``x`` into rows
    [rbegin, rend) of ``y``; gf / gb are the [w, m] neighbour planes
    (None at the global edges or where the rows do not need them).
    Complex blocks run as their real view with doubled columns."""
    name = "pam_fd_apply"
    k, dt = _real_code(y)
    nloc, m = x.shape
    if edge and nglob < _FD_EDGE_MIN.get(op, 1):
        raise _fd_too_short(name, op, nglob)
    halo = (fd_halo_width(op), m)
    for t, shape in ((x, y.shape), (gf, halo), (gb, halo)):
        if t is not None and (t.dtype != y.dtype or t.shape != shape):
            _typed(name, y.dtype, t)
            _shaped(name, shape, t)
    if not 0 <= rbegin <= rend <= nloc:
        raise ValueError(f"pam: {name}: rows [{rbegin}, {rend}) outside "
                         f"the {nloc}-row block")
    # spelled out, not _run: 14 arguments on the launch-bound CGLS path
    x, gf, gb = (t if t is None else t.contiguous() for t in (x, gf, gb))
    idx = require_device(*[t for t in (_dst(name, y), x, gf, gb)
                           if t is not None])
    _launch(idx, name, (
        int(op), 1 if edge else 0, x.data_ptr(),
        None if gf is None else gf.data_ptr(),
        None if gb is None else gb.data_ptr(), y.data_ptr(), nloc, k * m,
        int(row0), int(nglob), int(rbegin), int(rend), float(coeff), dt))


FD_ROW, FD_ROLL, FD_BAND = 0, 1, 2  # pam_fd_variant codes


def fd_band_rows() -> int:  # output rows per thread of the row-band kernel
    return int(_ffi.lib().pam_fd_band_rows())


def fd_variant(y, x, gf, gb, rbegin: int, rend: int) -> int:
    """The kernel fd_apply(y, x, gf, gb, ..., rbegin, rend, ...) runs with
    the environment as it is now: FD_ROW, FD_ROLL or FD_BAND.  Host-side
    query; nothing is enqueued."""
    k, dt = _real_code(y)
    x, gf, gb = (t if t is None else t.contiguous() for t in (x, gf, gb))
    aligned = all(t.data_ptr() % 16 == 0 for t in (y, x, gf, gb)
                  if t is not None)
    v = int(_ffi.lib().pam_fd_variant(dt, k * x.shape[1],
                                      int(rend) - int(rbegin),
                                      1 if aligned else 0))
    if v < 0:
        _ffi.checked(v, "pam_fd_variant")
    return v


def fd_serial(y, x, op: int, edge: bool, coeff: float):
    """Stencil ``op`` along dim 1 of the [batch, d, m] block ``x``.
    Complex blocks run as their real view with doubled m."""
    _typed("pam_fd_serial", y.dtype, x)
    k, dt = _real_code(y)
    batch, d, m = x.shape
    _shaped("pam_fd_serial", (batch, d, m), _dst("pam_fd_serial", y))
    if edge and d < _FD_EDGE_MIN.get(op, 1):
        raise _fd_too_short("pam_fd_serial", op, d)
    _run("pam_fd_serial", int(op), 1 if edge else 0, x.contiguous(), y,
         batch, d, k * m, float(coeff), dt)


def nsconv(y, x, hs, forward: bool, oh: float, dh: float):
    """Non-stationary convolution along dim 1 of the [batch, d, m] block
    ``x``, filters hs [nf, hsize] anchored at oh + q * dh."""
    _typed("pam_nsconv", y.dtype, x, hs)
    (batch, d, m), (nf, hsize) = x.shape, hs.shape
    _shaped("pam_nsconv", (batch, d, m), _dst("pam_nsconv", y))
    _run("pam_nsconv", 1 if forward else 0, x.contiguous(), y,
         hs.contiguous(), batch, d, m, nf, hsize, float(oh), float(dh),
         _code(y.dtype))


CONV_PLAIN, CONV_TRACE, CONV_COLUMN = 0, 1, 2  # pam_conv1d_variant codes


def conv1d(y, x, h, adjoint: bool, offset: int, deriv: int = 0):
    """Stationary convolution with the ``nh`` real taps ``h`` along dim 1
    of the [batch, d, m] block ``x``, ``offset`` the tap at lag zero:
    y[b,n,j] = sum_k h[k] * x[b, n-k+offset, j] (forward) or
    sum_k h[k] * x[b, n+k-offset, j] (adjoint), zero-padded at the ends.
    ``deriv`` fuses a first derivative along the same dim (1 centered,
    2 forward; edge False, sampling 1): forward C(Dx), adjoint D^T(C^T x),
    one launch.  Complex blocks run as their real view with doubled m;
    the taps stay real.  ``x`` and ``y`` must not share memory."""
    name = "pam_conv1d"
    rdt = _REAL_OF.get(y.dtype, y.dtype)
    if h.is_complex():
        raise TypeError(f"pam: {name}: complex taps are not supported "
                        f"(got {h.dtype})")
    _typed(name, y.dtype, x)
    _typed(name, rdt, h)
    k, dt = _real_code(y)
    batch, d, m = x.shape
    _shaped(name, (batch, d, m), y)
    if h.ndim != 1 or h.numel() < 1:
        raise ValueError(f"pam: {name}: taps must be 1-D and non-empty, "
                         f"got shape {tuple(h.shape)}")
    nh = h.numel()
    if not 0 <= int(offset) < nh:
        raise ValueError(f"pam: {name}: offset {offset} outside [0, {nh})")
    if int(deriv) not in (0, 1, 2):
        raise ValueError(f"pam: {name}: deriv {deriv} outside 0..2")
    _dst(name, y)
    _run(name, 1 if adjoint else 0, x.contiguous(), y, h.contiguous(),
         batch, d, k * m, nh, int(offset), int(deriv), dt)


def conv1d_variant(x, nh: int) -> int:
    """The kernel conv1d runs on the [batch, d, m] block ``x`` with ``nh``
    taps and the environment as it is now: CONV_PLAIN, CONV_TRACE or
    CONV_COLUMN.  Host-side query; nothing is enqueued."""
    k, dt = _real_code(x)
    _, d, m = x.shape
    v = int(_ffi.lib().pam_conv1d_variant(dt, d, k * m, int(nh)))
    if v < 0:
        _ffi.checked(v, "pam_conv1d_variant")
    return v


def conv1d_tile(variant: int, dtype, nh: int):
    """(tile_d, tile_m) one workgroup of ``variant`` owns for blocks of
    torch ``dtype`` (complex: of its real view) and ``nh`` taps; (0, 0)
    for CONV_PLAIN.  See pam_conv1d_tile_d in include/pam.h."""
    dt = _AS_REAL[dtype][1] if dtype in _AS_REAL else _code(dtype)
    td = int(_ffi.lib().pam_conv1d_tile_d(int(variant), dt, int(nh)))
    tm = int(_ffi.lib().pam_conv1d_tile_m(int(variant), dt))
    if td < 0 or tm < 0:
        _ffi.checked(min(td, tm), "pam_conv1d_tile")
    return td, tm


# ------------------------------------------------------------- Kirchhoff
KIRCH_GATHER, KIRCH_STAGED = 0, 1   # pam_kirch_variant codes
_kirch_scratch = {}     # per (device, dtype), sized for the largest seen


def _kirch_dims(name, d, m, qs, qr):
    """Dtype and shape checks of a pam_kirch block -> (ns, nr, ni, nt)."""
    if d.dtype not in (_F64, torch.float32):
        raise TypeError(f"pam: {name}: expected float64 or float32, got "
                        f"{d.dtype}")
    _typed(name, d.dtype, m, qs, qr)
    ns, nr, nt = d.shape
    (ni,) = m.shape
    _shaped(name, (ns, ni), qs)
    _shaped(name, (nr, ni), qr)
    if min(ns, nr, ni) < 1 or nt < 2:
        raise ValueError(f"pam: {name}: needs ns, nr, ni >= 1 and nt >= 2, "
                         f"got data {tuple(d.shape)}, model {tuple(m.shape)}")
    return ns, nr, ni, nt


def kirchhoff(d, m, qs, qr, adjoint: bool):
    """Kinematic Kirchhoff spread (``adjoint`` false: d <- m, every sample
    of d written) or gather (m <- d) between the model ``m`` (ni,) and the
    data ``d`` (ns, nr, nt), with the traveltime tables in samples
    ``qs`` (ns, ni) and ``qr`` (nr, ni).  See pam_kirch in include/pam.h.
    ``m`` and ``d`` must not share memory."""
    name = "pam_kirch"
    ns, nr, ni, nt = _kirch_dims(name, d, m, qs, qr)
    if adjoint:
        _dst(name, m)
        d = d.contiguous()
    else:
        _dst(name, d)
        m = m.contiguous()
    qs, qr = qs.contiguous(), qr.contiguous()
    idx = require_device(d, m, qs, qr)
    dt = _code(d.dtype)
    need = int(_ffi.lib().pam_kirch_ws_elems(1 if adjoint else 0, ns, nr, ni,
                                             nt, dt))
    ws = None
    if need > 0:
        ws = _kirch_scratch.get((idx, d.dtype))
        if ws is None or ws.numel() < need:
            ws = _kirch_scratch[(idx, d.dtype)] = torch.empty(
                need, dtype=d.dtype, device=d.device)
    _launch(idx, name, (1 if adjoint else 0, m.data_ptr(), d.data_ptr(),
                        qs.data_ptr(), qr.data_ptr(),
                        None if ws is None else ws.data_ptr(), ns, nr, ni,
                        nt, dt))


def _kirch_query(fn, d, m, qs, qr):
    name = "pam_kirch"
    ns, nr, ni, nt = _kirch_dims(name, d, m, qs, qr)
    v = int(getattr(_ffi.lib(), fn)(ns, nr, ni, nt, _code(d.dtype)))
    if v < 0:
        _ffi.checked(v, fn)
    return v


def kirchhoff_points() -> int:  # image points per workgroup of the gather
    return int(_ffi.lib().pam_kirch_points())


def kirchhoff_chunk(d, m, qs, qr) -> int:
    """Traces per partial sum of the gather on that block (ns * nr: the
    traces are not split), the environment as it is now.  Host-side."""
    return _kirch_query("pam_kirch_chunk", d, m, qs, qr)


def kirchhoff_variant(d, m, qs, qr) -> int:
    """The gather's body on that block: KIRCH_GATHER or KIRCH_STAGED."""
    return _kirch_query("pam_kirch_variant", d, m, qs, qr)


def kirchhoff_window(d, m, qs, qr) -> int:
    """Samples of the time window one workgroup of the spread owns."""
    return _kirch_query("pam_kirch_window", d, m, qs, qr)

"""Stationary convolution and post-stack modelling local operators — the
serial pylops operators the reference's post-stack and reflectivity
tutorials place inside MPIBlockDiag (pylops.signalprocessing.Convolve1D,
pylops.avo.poststack.PoststackLinearModelling), on the fused HIP kernel
pam_conv1d (csrc/conv1d.hip).

pylops is not vendored, so the convention is restated in include/pam.h and
locked by tests/convref.py: with ``offset`` the index of the tap at lag
zero,
    forward  y[n] = sum_k h[k] x[n - k + offset]
    adjoint  y[n] = sum_k h[k] x[n + k - offset]
zero-padded at both ends — pylops' "pad h until offset is its centre, then
convolve / correlate in mode same", for odd and even len(h) alike."""
from typing import Tuple, Union

import numpy as np
import torch

from . import kernels
from .distributedarray import as_torch_dtype
from .localops import LocalOperator

_REAL = {torch.complex128: torch.float64, torch.complex64: torch.float32}
_DERIV = {"centered": 1, "forward": 2}
# pam_fd_serial ops (matvec, rmatvec) of the unfused composition
_FD_OPS = {1: (4, 5), 2: (0, 1)}


class Convolve1DLocal(LocalOperator):
    """Convolution with the 1-D real filter ``h`` along ``axis`` of a
    local block of shape ``dims`` (pylops Convolve1D).  ``offset`` is the
    index of the filter's centre, 0 <= offset < len(h).

    ``h`` is a torch tensor or a NumPy array; a NumPy array (or a tensor
    on another device) is moved to the device of the first vector the
    operator is applied to.  A complex ``dtype`` convolves real and
    imaginary parts with the same real taps."""

    _deriv = 0

    def __init__(self, dims: Union[int, Tuple], h, offset: int = 0,
                 axis: int = -1, dtype="float64"):
        self.dims = (dims,) if isinstance(dims, (int, np.integer)) \
            else tuple(int(v) for v in dims)
        ax = axis if axis >= 0 else len(self.dims) + axis
        if not 0 <= ax < len(self.dims):
            raise ValueError(f"axis {axis} out of range for dims {self.dims}")
        self.axis = ax
        self.dtype = np.dtype(dtype)
        tdt = as_torch_dtype(self.dtype)
        if not isinstance(h, torch.Tensor):
            h = torch.from_numpy(np.ascontiguousarray(h))
        if h.ndim != 1 or h.numel() < 1:
            raise ValueError(f"h must be a non-empty 1-D filter, got shape "
                             f"{tuple(h.shape)}")
        if h.is_complex():
            raise TypeError("complex filters are not supported")
        if not 0 <= int(offset) < h.numel():
            raise ValueError(f"offset {offset} outside [0, {h.numel()})")
        self.h = h.to(_REAL.get(tdt, tdt)).contiguous()
        self.offset = int(offset)
        n = int(np.prod(self.dims))
        self.shape = (n, n)
        self.batch = int(np.prod(self.dims[:ax], initial=1))
        self.d = self.dims[ax]
        self.m = int(np.prod(self.dims[ax + 1:], initial=1))

    def _taps(self, device) -> torch.Tensor:
        if self.h.device != device:
            self.h = self.h.to(device)
        return self.h

    def _conv(self, x: torch.Tensor, adjoint: bool, deriv: int):
        x = x.reshape(self.batch, self.d, self.m)
        y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        kernels.conv1d(y, x, self._taps(x.device), adjoint, self.offset,
                       deriv)
        return y

    def matvec(self, x):
        return self._conv(x, False, self._deriv).view(-1)

    def rmatvec(self, x):
        return self._conv(x, True, self._deriv).view(-1)


class PoststackLinearModellingLocal(Convolve1DLocal):
    """Post-stack seismic modelling d = W D m (pylops
    PoststackLinearModelling, its implicit ``explicit=False`` branch):
    first derivative in time of the log acoustic impedance ``m`` followed
    by convolution with the wavelet ``wav`` centred at len(wav) // 2 —
        Convolve1D(wav, offset=len(wav)//2)
            * FirstDerivative(kind, sampling=1, edge=False)
    as ONE launch per apply: the reflectivity D m (adjoint: W^T d) is
    never written to memory.  ``fused=False`` runs the two-launch
    composition instead, which gives the same bits.

    The documented model carries a factor 1/2, d(t) = 1/2 w(t) * dm/dt;
    with kind="centered" the 3-point stencil 0.5 (m[t+1] - m[t-1])
    supplies it and no further factor is applied, with kind="forward"
    (m[t+1] - m[t]) there is none at all.  pylops could not be run against
    this operator; if a port differs from pylops by a factor of two, this
    is where to look.

    dims: pylops takes (nt0, *spatdims), time first — that is ``axis=0``
    (the default) and dims = (nt0, *spatdims).  ``axis`` is an extension
    for blocks stored with time elsewhere, e.g. contiguous traces:
    ``spatdims`` are then the remaining dims in storage order and
    dims = spatdims[:axis] + (nt0,) + spatdims[axis:]; this replaces the
    Transpose sandwich and its two extra passes over the volume.
    ``spatdims`` may be None (one trace), an int or a tuple."""

    def __init__(self, wav, nt0: int, spatdims=None, kind: str = "centered",
                 axis: int = 0, dtype="float64", fused: bool = True,
                 explicit: bool = False):
        if explicit:
            raise NotImplementedError(
                "explicit=True (a dense modelling matrix) is not built "
                "here: form the matrix on the host and wrap it in "
                "DenseLocal")
        if (wav.ndim if hasattr(wav, "ndim") else np.ndim(wav)) != 1:
            raise NotImplementedError(
                "a 2-D (non-stationary) wav is not supported: build the "
                "dense operator on the host and wrap it in DenseLocal")
        if kind not in _DERIV:
            raise NotImplementedError("'kind' must be 'centered' or "
                                      "'forward'")
        if spatdims is None:
            spat = ()
        elif isinstance(spatdims, (int, np.integer)):
            spat = (int(spatdims),)
        else:
            spat = tuple(int(v) for v in spatdims)
        ax = axis if axis >= 0 else len(spat) + 1 + axis
        if not 0 <= ax <= len(spat):
            raise ValueError(f"axis {axis} out of range for "
                             f"{len(spat) + 1} dims")
        dims = spat[:ax] + (int(nt0),) + spat[ax:]
        super().__init__(dims, wav, offset=len(wav) // 2, axis=ax,
                         dtype=dtype)
        self.kind = kind
        self.fused = bool(fused)
        self._deriv = _DERIV[kind]

    def _fd(self, x: torch.Tensor, op: int) -> torch.Tensor:
        y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        kernels.fd_serial(y, x, op, False, 1.0)
        return y

    def matvec(self, x):
        if self.fused:
            return super().matvec(x)
        v = self._fd(x.reshape(self.batch, self.d, self.m),
                     _FD_OPS[self._deriv][0])
        return self._conv(v, False, 0).view(-1)

    def rmatvec(self, x):
        if self.fused:
            return super().rmatvec(x)
        return self._fd(self._conv(x, True, 0),
                        _FD_OPS[self._deriv][1]).view(-1)

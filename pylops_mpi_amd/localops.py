"""Local (per-rank, serial) operators used inside MPIBlockDiag and the
serial-operator wrap of MPILinearOperator.

The reference uses pylops.LinearOperator here (ref BlockDiag.py:128-143
duck-types .shape/.matvec/.rmatvec on the rank-local array); our local
operators follow the same protocol on torch device tensors, with the
compute in hand-written HIP kernels (no torch math on the product path).
"""
from typing import Callable, Optional, Tuple

import numpy as np
import torch

from . import kernels


class LocalOperator:
    """Protocol: shape (n, m); matvec/rmatvec on 1-D device tensors."""

    shape: Tuple[int, int]
    dtype: np.dtype

    def matvec(self, x: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    def rmatvec(self, x: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError


class DenseLocal(LocalOperator):
    """Dense matrix operator (the serial pylops.MatrixMult analog used by
    the reference's BlockDiag examples, ref examples/plot_cgls.py:30-33):
    matvec = A @ x, rmatvec = A^T @ x via pam_gemv (HBM-bound HIP
    kernels; real dtypes — A^H == A^T).

    ``saveAt`` (default True) materializes A^T on the first rmatvec so
    the adjoint runs the row-parallel n-path GEMV (6.4 TB/s) instead of
    the two-stage transpose path (4.7 TB/s, fixed partial-combine
    overhead — r01 measured table).  Costs one extra copy of A in HBM
    (trivial against 288 GB); set saveAt=False to keep single-copy."""

    def __init__(self, A: torch.Tensor, saveAt: bool = True):
        if A.ndim != 2:
            raise ValueError("DenseLocal expects a 2-D matrix")
        self.A = A.contiguous()
        self.shape = (int(A.shape[0]), int(A.shape[1]))
        self.saveAt = bool(saveAt)
        self._At = None
        self.dtype = np.dtype(
            {torch.float64: np.float64, torch.float32: np.float32}[A.dtype])

    def _gemv(self, A: torch.Tensor, x: torch.Tensor, trans: bool,
              nout: int) -> torch.Tensor:
        out = torch.empty(nout, dtype=A.dtype, device=A.device)
        kernels.gemv(out, A, x, trans)
        return out

    def matvec(self, x: torch.Tensor) -> torch.Tensor:
        return self._gemv(self.A, x, False, self.shape[0])

    def rmatvec(self, x: torch.Tensor) -> torch.Tensor:
        if self.saveAt:
            if self._At is None:
                At = torch.empty((self.shape[1], self.shape[0]),
                                 dtype=self.A.dtype, device=self.A.device)
                kernels.transpose(At, self.A)
                self._At = At
            return self._gemv(self._At, x, False, self.shape[1])
        return self._gemv(self.A, x, True, self.shape[1])


class AdjointLocal(LocalOperator):
    """Adjoint view of a local operator (swap matvec/rmatvec)."""

    def __init__(self, op: LocalOperator):
        self.op = op
        self.shape = (op.shape[1], op.shape[0])
        self.dtype = op.dtype

    def matvec(self, x):
        return self.op.rmatvec(x)

    def rmatvec(self, x):
        return self.op.matvec(x)


class CallableLocal(LocalOperator):
    """Adapter for tests/composition: wrap a (matvec, rmatvec) pair."""

    def __init__(self, shape: Tuple[int, int],
                 matvec: Callable[[torch.Tensor], torch.Tensor],
                 rmatvec: Optional[Callable[[torch.Tensor],
                                            torch.Tensor]] = None,
                 dtype=np.float64):
        self.shape = shape
        self.dtype = np.dtype(dtype)
        self._mv = matvec
        self._rmv = rmatvec

    def matvec(self, x):
        return self._mv(x)

    def rmatvec(self, x):
        if self._rmv is None:
            raise NotImplementedError
        return self._rmv(x)

"""The launch layer's argument checks, exercised with CPU tensors: every
check runs before anything is launched, the device check last, so each
rejection is observable without a GPU — and no output may change."""
import pytest
import torch

from pylops_mpi_amd import kernels


def _operands(dtype=torch.float64):
    a = torch.arange(24, dtype=dtype).reshape(6, 4)
    return a, a + 100.0


def test_noncontiguous_output_rejected():
    a, b = (t.t() for t in _operands(torch.float32))
    out = torch.empty(6, 4).t()
    out.fill_(-1.0)
    with pytest.raises(ValueError, match="pam_add.*contiguous"):
        kernels.add(out, a, b)
    assert torch.all(out == -1.0)
    # in-place operand: same rule
    with pytest.raises(ValueError, match="pam_axpy.*contiguous"):
        kernels.axpy(out, a, 2.0)
    assert torch.all(out == -1.0)


def test_mismatched_element_counts_rejected():
    a, b = _operands()
    out = torch.full((6, 4), -1.0, dtype=torch.float64)
    with pytest.raises(ValueError, match="pam_add"):
        kernels.add(out, a, b[:5])
    with pytest.raises(ValueError, match="pam_dot"):
        kernels.dot(a, b[:5], out.view(-1)[:1])
    C = torch.full((6, 3), -1.0, dtype=torch.float64)
    with pytest.raises(ValueError, match="pam_gemm"):
        kernels.gemm(C, a, b)                 # (6,4) @ (6,4)
    assert torch.all(out == -1.0) and torch.all(C == -1.0)


def test_mixed_dtypes_rejected():
    a, b = _operands()
    out = torch.full((6, 4), -1.0, dtype=torch.float64)
    with pytest.raises(TypeError, match="pam_add"):
        kernels.add(out, a, b.to(torch.float32))
    with pytest.raises(TypeError, match="pam_axpy_d"):
        kernels.axpy_d(out, a, torch.ones(1, dtype=torch.float32))
    with pytest.raises(TypeError, match="pam_unzip"):
        kernels.unzip(out, a.to(torch.complex64))   # wants float32 out
    assert torch.all(out == -1.0)


def test_valid_cpu_tensors_hit_the_device_error_last():
    a, b = _operands()
    out = torch.full((6, 4), -1.0, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU compute path"):
        kernels.add(out, a, b)
    with pytest.raises(RuntimeError, match="no CPU compute path"):
        kernels.add(out, a.t().reshape(6, 4), b)    # inputs may be strided
    with pytest.raises(RuntimeError, match="no CPU compute path"):
        kernels.dot(a, b)
    C = torch.full((6, 6), -1.0, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU compute path"):
        kernels.gemm(C, a, b.t())
    assert torch.all(out == -1.0) and torch.all(C == -1.0)


# shortest axis of the stencils with edge: ops 4, 5 need 2 samples, ops 6, 7,
# 12, 13 need 3 (include/pam.h); nothing shorter is ever launched
FD_SHORT = [(op, n) for op in (4, 5) for n in (1,)] + \
           [(op, n) for op in (6, 7, 12, 13) for n in (1, 2)]


def test_fd_min_rows_table():
    for op in range(14):
        assert kernels.fd_min_rows(op, False) == 1
        assert kernels.fd_min_rows(op, True) == (
            2 if op in (4, 5) else 3 if op in (6, 7, 12, 13) else 1)


@pytest.mark.parametrize("dtype", [torch.float64, torch.complex64])
def test_fd_apply_rejects_short_axis_with_edge(dtype):
    for op, n in FD_SHORT:
        x = torch.ones((n, 5), dtype=dtype)
        y = torch.full((n, 5), -1.0, dtype=dtype)
        with pytest.raises(ValueError, match="pam_fd_apply.*at least"):
            kernels.fd_apply(y, x, None, None, op, True, 0, n, 0, n, 1.0)
        # a one-row block of a short GLOBAL axis: nglob decides, not nloc
        g = torch.ones((1 if op < 6 else 2, 5), dtype=dtype)
        with pytest.raises(ValueError, match="pam_fd_apply.*at least"):
            kernels.fd_apply(y[:1], x[:1], g if n > 1 else None, None, op,
                             True, n - 1, n, 0, 1, 1.0)
        assert torch.all(y == -1.0)


def _at_the_minimum():
    for op in range(14):
        for edge, n in ((True, kernels.fd_min_rows(op, True)), (False, 1)):
            yield (op, edge, n, torch.ones((n, 5), dtype=torch.float64),
                   torch.full((n, 5), -1.0, dtype=torch.float64))


def test_fd_serial_accepts_the_minimum_and_edge_false():
    """At the minimum length, and at any length without edge, the checks
    pass and the call ends at the device check."""
    for op, edge, n, x, y in _at_the_minimum():
        with pytest.raises(RuntimeError, match="no CPU compute path"):
            kernels.fd_serial(y.view(1, n, 5), x.view(1, n, 5), op, edge, 1.0)
        assert torch.all(y == -1.0)


def test_fd_apply_accepts_the_minimum_and_edge_false():
    """The same for fd_apply, which asks the library for the op's halo
    width on the way: the one test of this file that needs libpam.so."""
    from pylops_mpi_amd import _ffi
    if not _ffi.available():
        pytest.skip("libpam.so not built (run __graft_entry__.build())")
    for op, edge, n, x, y in _at_the_minimum():
        with pytest.raises(RuntimeError, match="no CPU compute path"):
            kernels.fd_apply(y, x, None, None, op, edge, 0, n, 0, n, 1.0)
        assert torch.all(y == -1.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.complex128])
def test_fd_serial_rejects_short_axis_with_edge(dtype):
    for op, n in FD_SHORT:
        x = torch.ones((3, n, 4), dtype=dtype)
        y = torch.full((3, n, 4), -1.0, dtype=dtype)
        with pytest.raises(ValueError, match="pam_fd_serial.*at least"):
            kernels.fd_serial(y, x, op, True, 1.0)
        assert torch.all(y == -1.0)


def test_local_derivatives_on_a_short_axis_raise_value_error():
    """FirstDerivativeLocal / SecondDerivativeLocal along an axis of one
    sample with edge, and the component of MPIGradient that holds one: a
    ValueError from the argument checks, not a device error."""
    import pylops_mpi_amd as pm
    from pylops_mpi_amd.fdlocal import (FirstDerivativeLocal,
                                        SecondDerivativeLocal)
    for op in (FirstDerivativeLocal((4, 1), axis=1, edge=True),
               FirstDerivativeLocal((4, 2), axis=1, edge=True, order=5),
               SecondDerivativeLocal((4, 1), axis=1, edge=True),
               SecondDerivativeLocal((2, 2), axis=1, edge=True)):
        v = torch.ones(op.shape[1], dtype=torch.float64)
        for fn in (op.matvec, op.rmatvec):
            with pytest.raises(ValueError, match="pam_fd_serial.*at least"):
                fn(v)
    grad = pm.MPIGradient(dims=(12, 7, 1), edge=True)
    along7, along1 = (blockdiag.ops[0] for blockdiag in grad.Op.ops[1:])
    assert (along7.d, along1.d) == (7, 1)
    x = torch.ones(84, dtype=torch.float64)
    for fn in (along1.matvec, along1.rmatvec):
        with pytest.raises(ValueError, match="pam_fd_serial.*at least"):
            fn(x)                       # the axis of one sample
    with pytest.raises(RuntimeError, match="no CPU compute path"):
        along7.matvec(x)                # the axis of 7 is a valid input

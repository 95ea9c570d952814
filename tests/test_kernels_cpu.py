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

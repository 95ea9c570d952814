"""GPU checks of the tensor-level launch layer (pylops_mpi_amd.kernels):
the hazards are in the host layer, not the kernels, so the shapes are
tiny — a non-contiguous local block, a strided GEMM input, and the
complex-as-real-view path on an odd length (vector tail)."""
import numpy as np
import pytest
import torch
from numpy.testing import assert_allclose

import pylops_mpi_amd as pm
from pylops_mpi_amd import kernels, sparsity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _init():
    from pylops_mpi_amd.comm import init_default_comm
    init_default_comm(torch.device(DEV))


@pytest.fixture(scope="module")
def strided_pair():
    """Two DistributedArrays over transposed (non-contiguous) (8, 6)
    blocks, with the values they hold."""
    g = torch.Generator(device=DEV).manual_seed(11)
    ta, tb = (torch.randn(6, 8, device=DEV, dtype=torch.float64,
                          generator=g).t() for _ in range(2))
    assert not ta.is_contiguous()
    a = pm.DistributedArray((8, 6), local_array=ta)
    b = pm.DistributedArray((8, 6), local_array=tb)
    return a, b, ta.clone(), tb.clone()


def test_inplace_on_noncontiguous_block_raises(strided_pair):
    a, b, ta, _ = strided_pair
    with pytest.raises(ValueError, match="contiguous"):
        a += b
    with pytest.raises(ValueError, match="contiguous"):
        a -= b
    with pytest.raises(ValueError, match="contiguous"):
        a.iaxpy_(0.5, b)
    with pytest.raises(ValueError, match="contiguous"):
        a.xpby_(b, 0.5)
    with pytest.raises(ValueError, match="contiguous"):
        sparsity._apply_thresh(a, 0, 0.1)
    assert torch.equal(a.local_array, ta)      # nothing was written


def test_out_of_place_on_noncontiguous_block(strided_pair):
    # tolerances of tests/test_gpu_parity.py for the same ops
    a, b, ta, tb = strided_pair
    host = lambda t: t.cpu().numpy()                         # noqa: E731
    assert_allclose(host((a + b).local_array), host(ta + tb), rtol=1e-14)
    assert_allclose(host((a * 2.0).local_array), host(ta * 2.0), rtol=1e-14)
    assert_allclose(a.dot(b), host((ta * tb).sum()), rtol=1e-13)
    assert_allclose(a.norm(), host(torch.linalg.vector_norm(ta)), rtol=1e-13)


def test_gemm_transposed_view_input():
    rng = np.random.default_rng(5)
    buf = rng.standard_normal((12, 16))
    B = rng.standard_normal((12, 20)) + np.arange(20)[None, :] * 1e-3
    A = torch.as_tensor(buf, device=DEV).t()            # 16 x 12 view
    assert not A.is_contiguous()
    C = torch.empty((16, 20), dtype=torch.float64, device=DEV)
    kernels.gemm(C, A, torch.as_tensor(B, device=DEV))
    # tolerance of tests/test_gpu_matmult.py::test_gemm_f64
    assert_allclose(C.cpu().numpy(), buf.T @ B, rtol=1e-12, atol=1e-10)


def test_complex_real_view_bitwise():
    g = torch.Generator(device=DEV).manual_seed(3)
    a, b = (torch.randn(33, device=DEV, dtype=torch.complex64, generator=g)
            for _ in range(2))
    y = torch.empty_like(a)
    kernels.add(y, a, b)
    assert torch.equal(y, a + b)
    # real-alpha axpy: mul-round then add-round on each (re, im) component
    y0 = y.clone()
    kernels.axpy(y, b, 0.7)
    ref = torch.view_as_real(y0) + 0.7 * torch.view_as_real(b)
    assert torch.equal(torch.view_as_real(y), ref)

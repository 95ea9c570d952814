"""Rolling-window stencil kernel (csrc/pam.hip fd_roll_kernel) against the
row-parallel kernel, bit for bit.

No knob is involved: rows over 4 MiB in 16-B aligned tensors dispatch to
the rolling kernel, and the same data read from a copy offset by one
element is misaligned and dispatches to the row-parallel kernel at one
element per lane.  Both facts are ASSERTED through kernels.fd_variant
before the outputs are compared with torch.equal.

Shapes: m just over 4 MiB of row, so that the last column block is partly
empty and holds one chain with no valid column — fp64 m = 2^19 + 4 (32-B
lanes) and 2^19 + 6 (16-B lanes), fp32 m = 2^20 + 8; row counts 1, 2, 5, 17
and 33 (the rolling kernel walks chunks of at least 16 rows, so 17 and 33
give more than one chunk).  Every count runs as a whole global array, as a
middle block with ghost planes (the clamped preloads then read them) and,
from 5 rows, as a sub-range of a middle block, whose other rows must keep
their fill value.  edge=True on a whole array of fewer than 3 rows is not a
defined input (tests/test_gpu_fd_band.py) and runs only as a middle block."""
import pytest
import torch

from pylops_mpi_amd import kernels

pytestmark = pytest.mark.gpu

OPS = range(14)
ROWS = (1, 2, 5, 17, 33)
COLS = {torch.float64: ((1 << 19) + 4, (1 << 19) + 6),
        torch.float32: ((1 << 20) + 8,)}
FILL = 7.0   # rows a launch must not store keep this


@pytest.fixture(scope="module", autouse=True)
def _init():
    from pylops_mpi_amd.comm import init_default_comm
    init_default_comm(torch.device("cuda:0"))


def _apply(want_variant, X, lo, nloc, w, ghosts, op, edge, row0, nglob, rb,
           re):
    """One fd_apply on rows [lo, lo + nloc) of X, after asserting the
    kernel the launch will use; rows outside [rb, re) must stay FILL."""
    x = X[lo:lo + nloc]
    gf = X[lo - w:lo] if ghosts else None
    gb = X[lo + nloc:lo + nloc + w] if ghosts else None
    y = torch.full((nloc, X.shape[1]), FILL, dtype=X.dtype, device=X.device)
    assert kernels.fd_variant(y, x, gf, gb, rb, re) == want_variant
    kernels.fd_apply(y, x, gf, gb, op, edge, row0, nglob, rb, re, 0.75)
    assert bool((y[:rb] == FILL).all() and (y[re:] == FILL).all())
    return y


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("edge", [False, True])
def test_roll_equals_row_kernel(monkeypatch, dtype, edge):
    for name in ("PAM_FD_BAND", "PAM_FD_ROLL", "PAM_FD_LONGROW"):
        monkeypatch.delenv(name, raising=False)
    for m in COLS[dtype]:
        assert m * dtype.itemsize > 4 << 20 and (m * dtype.itemsize) % 16 == 0
        nmax = max(ROWS) + 4
        g = torch.Generator(device="cuda:0").manual_seed(21)
        X = torch.randn((nmax, m), generator=g, dtype=dtype, device="cuda:0")
        # the same values one element off 16-B alignment
        base = torch.empty(nmax * m + 1, dtype=dtype, device="cuda:0")
        Xo = base[1:].view(nmax, m)
        Xo.copy_(X)
        assert X.data_ptr() % 16 == 0 and Xo.data_ptr() % 16 != 0
        for nloc in ROWS:
            for op in OPS:
                w = kernels.fd_halo_width(op)
                runs = [(2, True, 2, nloc + 4, 0, nloc)]
                if not (edge and nloc < 3):
                    runs.append((0, False, 0, nloc, 0, nloc))
                if nloc >= 5:
                    runs.append((2, True, 2, nloc + 4, 1, nloc - 2))
                for lo, ghosts, row0, nglob, rb, re in runs:
                    args = (lo, nloc, w, ghosts, op, edge, row0, nglob, rb,
                            re)
                    yr = _apply(kernels.FD_ROLL, X, *args)
                    yp = _apply(kernels.FD_ROW, Xo, *args)
                    assert torch.equal(yr, yp), (m, nloc, op, edge, args)

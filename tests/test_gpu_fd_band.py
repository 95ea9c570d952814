"""Row-band stencil kernel (csrc/pam.hip fd_band_kernel) against the
row-parallel kernel, bit for bit, and against the oracle.

Every comparison forces the band kernel with PAM_FD_BAND=1 and ASSERTS
through kernels.fd_variant that it is what runs; the reference is the
row-parallel kernel forced with PAM_FD_BAND=-1 in the same process on the
same tensors (torch.equal).  The shapes are the smallest at which the band
kernel can go wrong: row counts around one, two and three bands (single
band holding both global edges, partial last band), one partial column
block, several blocks with a column tail, sub-ranges with ghost planes.

edge=True on a whole global array of fewer than 3 rows is not a defined
input (the edge formulas read up to 2 rows away, so BOTH kernels would read
outside the array): those row counts run edge=True as a middle block of a
larger array with ghost planes instead, which every row count also does."""
import numpy as np
import pytest
import torch
from numpy.testing import assert_allclose

import oracle
import pylops_mpi_amd as pm
from pylops_mpi_amd import kernels

pytestmark = pytest.mark.gpu

OPS = range(14)
COLS = [2, 6, 2 * (256 + 3), 4 * (256 + 1)]
FILL = 7.0   # rows a launch must not store keep this


@pytest.fixture(scope="module", autouse=True)
def _init():
    from pylops_mpi_amd.comm import init_default_comm
    init_default_comm(torch.device("cuda:0"))


@pytest.fixture(scope="module")
def RT():
    return kernels.fd_band_rows()


def row_counts(RT):
    return sorted({1, 2, 3, RT - 1, RT, RT + 1, 2 * RT - 1, 2 * RT,
                   2 * RT + 1, 3 * RT + 2})


def randn(shape, dtype, seed):
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=dtype, device="cuda:0")


def apply(mp, mode, want_variant, x, gf, gb, op, edge, row0, nglob, rb, re,
          y=None):
    """One fd_apply under PAM_FD_BAND=mode, after asserting the kernel the
    launch will use."""
    mp.setenv("PAM_FD_BAND", mode)
    if y is None:
        y = torch.full_like(x, FILL)
    got = kernels.fd_variant(y, x, gf, gb, rb, re)
    assert got == want_variant, (mode, got, tuple(x.shape), rb, re)
    kernels.fd_apply(y, x, gf, gb, op, edge, row0, nglob, rb, re, 0.75)
    return y


def band_equals_row(mp, x, gf, gb, op, edge, row0, nglob, rb, re):
    # the band kernel needs 16-B lanes: m a multiple of 2 (fp64) / 4 (fp32)
    # on 16-B aligned rows; a row count never rules it out when forced
    lanes = 16 // x.element_size()
    assert all(t.data_ptr() % 16 == 0 or x.shape[1] % lanes
               for t in (x, gf, gb) if t is not None)
    forced = kernels.FD_ROW if x.shape[1] % lanes else kernels.FD_BAND
    yb = apply(mp, "1", forced, x, gf, gb, op, edge, row0, nglob,
               rb, re)
    yr = apply(mp, "-1", kernels.FD_ROW, x, gf, gb, op, edge, row0, nglob,
               rb, re)
    assert torch.equal(yb, yr), (op, edge, tuple(x.shape), row0, nglob, rb,
                                 re)
    return yb


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("edge", [False, True])
def test_band_equals_row_kernel(monkeypatch, RT, dtype, edge):
    """All 14 ops x row counts x column counts, as a whole global array
    and as a middle block (row0 = 2 of nloc + 4 rows) with ghost planes."""
    for m in COLS:
        X = randn((3 * RT + 2 + 4, m), dtype, 5)
        for nloc in row_counts(RT):
            for op in OPS:
                w = kernels.fd_halo_width(op)
                if not (edge and nloc < 3):
                    band_equals_row(monkeypatch, X[:nloc], None, None, op,
                                    edge, 0, nloc, 0, nloc)
                band_equals_row(monkeypatch, X[2:2 + nloc], X[2 - w:2],
                                X[2 + nloc:2 + nloc + w], op, edge, 2,
                                nloc + 4, 0, nloc)


def test_unstored_rows_and_subranges(monkeypatch, RT):
    """A launch of rows [rb, re) stores nothing else, whichever band the
    range starts or ends in."""
    nloc, m = 3 * RT + 2, 518
    x = randn((nloc, m), torch.float64, 6)
    for op in (4, 5, 7, 12):
        for rb, re in ((0, 1), (1, nloc - 1), (RT - 1, 2 * RT + 1),
                       (nloc - 1, nloc), (2, 2 + RT)):
            y = band_equals_row(monkeypatch, x, None, None, op, True, 0,
                                nloc, rb, re)
            assert bool((y[:rb] == FILL).all() and (y[re:] == FILL).all())


def _blocks(N, sizes):
    assert sum(sizes) == N
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    return [(int(s), int(n)) for s, n in zip(starts, sizes)]


@pytest.mark.parametrize("op", [4, 5, 7, 13])   # W=1 and W=2
@pytest.mark.parametrize("P", [2, 3])
def test_rank_blocks_with_ghosts(monkeypatch, RT, op, P):
    """The multi-GPU paths emulated on one GPU: the global [N, m] array is
    cut into P row blocks, each launched with its neighbours' planes as
    gf/gb — (a) whole block, (b) the overlap path's three launches
    [w, nloc-w) without ghosts, then [0, w) and [nloc-w, nloc) with them.
    One block has nloc = 2w+1, the smallest the overlap path accepts."""
    N, m = 3 * RT + 5, 518
    w = kernels.fd_halo_width(op)
    X = randn((N, m), torch.float64, 7)
    whole = apply(monkeypatch, "-1", kernels.FD_ROW, X, None, None, op, True,
                  0, N, 0, N)
    small = 2 * w + 1
    sizes = [small, N - small] if P == 2 else \
        [RT + 1, small, N - small - RT - 1]
    for split in (False, True):
        outs = []
        for r, (s, nloc) in enumerate(_blocks(N, sizes)):
            x = X[s:s + nloc]
            gf = X[s - w:s] if r > 0 else None
            gb = X[s + nloc:s + nloc + w] if r < P - 1 else None
            args = (op, True, s, N)
            if split:
                y = apply(monkeypatch, "1", kernels.FD_BAND, x, None, None,
                          *args, w, nloc - w)
                apply(monkeypatch, "1", kernels.FD_BAND, x, gf, gb, *args, 0,
                      w, y=y)
                apply(monkeypatch, "1", kernels.FD_BAND, x, gf, gb, *args,
                      nloc - w, nloc, y=y)
            else:
                y = apply(monkeypatch, "1", kernels.FD_BAND, x, gf, gb,
                          *args, 0, nloc)
            outs.append(y)
        assert torch.equal(torch.cat(outs), whole), (op, P, split)


def test_odd_columns_and_misaligned_use_row_kernel(monkeypatch, RT):
    """No 16-B lanes, no band kernel — even when forced."""
    nloc = 2 * RT + 1
    x = randn((nloc, 7), torch.float64, 8)
    yb = apply(monkeypatch, "1", kernels.FD_ROW, x, None, None, 5, True, 0,
               nloc, 0, nloc)
    yr = apply(monkeypatch, "-1", kernels.FD_ROW, x, None, None, 5, True, 0,
               nloc, 0, nloc)
    assert torch.equal(yb, yr)
    # x offset by one element: 8-B but not 16-B aligned
    m = 518
    base = randn((nloc * m + 1,), torch.float64, 9)
    xo = base[1:].view(nloc, m)
    assert xo.data_ptr() % 16 == 8 and xo.is_contiguous()
    yo = apply(monkeypatch, "1", kernels.FD_ROW, xo, None, None, 4, True, 0,
               nloc, 0, nloc)
    ya = band_equals_row(monkeypatch, xo.clone(), None, None, 4, True, 0,
                         nloc, 0, nloc)
    assert torch.equal(yo, ya)


def _operator_variant(dims, dtype):
    """The kernel the operator's single whole-block launch uses."""
    t = torch.empty((dims[0], int(np.prod(dims[1:]))), dtype=dtype,
                    device="cuda:0")
    return kernels.fd_variant(t, t, None, None, 0, dims[0])


def _check_vs_oracle(dims, dtype=np.float64):
    n = int(np.prod(dims))
    rng = np.random.default_rng(12)
    xg = rng.standard_normal(n)
    if np.dtype(dtype).kind == "c":
        xg = xg + 1j * rng.standard_normal(n)
    x = pm.DistributedArray.to_dist(torch.as_tensor(xg, device="cuda:0"))
    sx = oracle.to_dist(xg, 1)
    pairs = []
    for edge in (False, True):
        for kind, order in (("centered", 3), ("centered", 5),
                            ("forward", 3), ("backward", 3)):
            pairs.append((
                pm.MPIFirstDerivative(dims, 1.5, kind, edge, order,
                                      dtype=dtype),
                oracle.SimFirstDerivative(dims, 1.5, kind, edge, order,
                                          dtype=dtype)))
        for kind in ("forward", "backward", "centered"):
            pairs.append((
                pm.MPISecondDerivative(dims, 1.5, kind, edge, dtype=dtype),
                oracle.SimSecondDerivative(dims, 1.5, kind, edge,
                                           dtype=dtype)))
    for op, sop in pairs:
        assert_allclose(op.matvec(x).asarray().cpu().numpy(),
                        sop.matvec(sx).asarray(), rtol=1e-13, atol=1e-14)
        assert_allclose(op.rmatvec(x).asarray().cpu().numpy(),
                        sop.rmatvec(sx).asarray(), rtol=1e-13, atol=1e-14)


@pytest.mark.parametrize("dims,variant", [
    ((20, 7), kernels.FD_ROW),             # no 16-B lanes
    ((20, 518), kernels.FD_ROW),           # short rows
    ((8, 1280, 256), kernels.FD_ROLL),     # 2.5 MiB ragged, under the floor
    ((16, 1280, 256), kernels.FD_BAND),    # 2.5 MiB ragged, 4 bands of rows
    ((6, 2048, 512), kernels.FD_ROLL),     # rows over 4 MiB
])
def test_auto_rule_branches(monkeypatch, RT, dims, variant):
    """Each branch of the automatic dispatch at the smallest shape that
    reaches it: the kernel the query reports, and the result against the
    oracle (first derivative, both centered orders)."""
    monkeypatch.delenv("PAM_FD_BAND", raising=False)
    assert RT == 4, "the (16, 1280, 256) case assumes a floor of 4*RT = 16"
    assert _operator_variant(dims, torch.float64) == variant
    n = int(np.prod(dims))
    xg = np.random.default_rng(13).standard_normal(n)
    x = pm.DistributedArray.to_dist(torch.as_tensor(xg, device="cuda:0"))
    sx = oracle.to_dist(xg, 1)
    for order in (3, 5):
        op = pm.MPIFirstDerivative(dims, 1.5, "centered", True, order)
        sop = oracle.SimFirstDerivative(dims, 1.5, "centered", True, order)
        assert_allclose(op.matvec(x).asarray().cpu().numpy(),
                        sop.matvec(sx).asarray(), rtol=1e-13, atol=1e-14)
        assert_allclose(op.rmatvec(x).asarray().cpu().numpy(),
                        sop.rmatvec(sx).asarray(), rtol=1e-13, atol=1e-14)


def test_unrolled_row_kernel_equals_band(monkeypatch):
    """The row-parallel kernel runs its 4x-unrolled interior path once a
    block has >= 4 column iterations, which the launch grid only reaches
    at about 2^28 column vectors per launch: one launch of that size, with
    a remainder after the unrolled trips, against the band kernel.  One op
    per (term count, halo width) class: NT = 2, 3, 4 and W = 1, 2."""
    nloc, m = 2048, 2 * (131072 + 300)
    x = randn((nloc, m), torch.float64, 14)
    for op in (4, 5, 7, 12):
        band_equals_row(monkeypatch, x, None, None, op, False, 0, nloc, 0,
                        nloc)


def test_band_vs_oracle(monkeypatch, RT):
    """All operator kinds, edge False and True, through the operator
    classes with the band kernel forced (fp64, the oracle's tolerance)."""
    monkeypatch.setenv("PAM_FD_BAND", "1")
    # the oracle's 5-point operators want a few rows more than the stencil
    for nloc in sorted({max(n, 6) for n in (RT - 1, RT, 2 * RT + 1,
                                            3 * RT + 2)}):
        for m in (6, 518):
            assert _operator_variant((nloc, m), torch.float64) == \
                kernels.FD_BAND
            _check_vs_oracle((nloc, m))


def test_band_complex_vs_oracle(monkeypatch, RT):
    """complex128 runs as its real view with doubled columns."""
    monkeypatch.setenv("PAM_FD_BAND", "1")
    dims = (2 * RT + 1, 259)
    assert _operator_variant(dims, torch.complex128) == kernels.FD_BAND
    _check_vs_oracle(dims, np.complex128)

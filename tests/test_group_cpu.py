"""L2,1 group kernels, MPIL21 and PrimalDual — everything that can be
checked without a GPU: the C-ABI's argument checks (they run before any
HIP call), header / binding / export agreement, the launch layer's check
order on CPU tensors, and MPIL21's validation at world size 1.

Every ctypes call below passes n <= 0, so even a missing check could not
reach a launch with these placeholder pointers."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pylops_mpi_amd as pm
from pylops_mpi_amd import _ffi, kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pam.h")
EARG, EDTYPE, EOP = -1, -2, -3
F64, C64 = 0, 3


@pytest.fixture(scope="module")
def lib():
    return _ffi.lib()


@pytest.fixture(scope="module")
def buf():
    """One live host buffer; its address stands in for every pointer."""
    return ctypes.create_string_buffer(64)


def _shrink(lib, p, mode=0, ncomp=3, y=None, a=None, b=None, n=0,
            thresh=1.5, dtype=F64):
    y = [p, p, p, None] if y is None else y
    a = [p, p, p, None] if a is None else a
    b = [None] * 4 if b is None else b
    return lib.pam_group_shrink(None, mode, ncomp, *y, *a, *b, 0.5, n,
                                thresh, dtype)


def test_group_shrink_argument_errors(lib, buf):
    p = ctypes.addressof(buf)
    assert _shrink(lib, p) == 0                       # n == 0: no launch
    assert _shrink(lib, p, b=[p, p, p, None]) == 0
    assert _shrink(lib, p, ncomp=0) == EARG
    assert _shrink(lib, p, ncomp=5, y=[p] * 4, a=[p] * 4) == EARG
    assert _shrink(lib, p, y=[p, None, p, None]) == EARG
    assert _shrink(lib, p, a=[p, p, None, None]) == EARG
    assert _shrink(lib, p, ncomp=4) == EARG           # 4th slot is NULL
    assert _shrink(lib, p, b=[p, None, p, None]) == EARG   # partly NULL
    assert _shrink(lib, p, b=[None, p, p, None]) == EARG
    assert _shrink(lib, p, n=-1) == EARG
    assert _shrink(lib, p, thresh=-0.5) == EARG
    assert _shrink(lib, p, mode=2) == EOP
    assert _shrink(lib, p, mode=-1) == EOP
    assert _shrink(lib, p, dtype=4) == EDTYPE
    assert _shrink(lib, p, dtype=-1) == EDTYPE
    # slots past ncomp are ignored
    assert _shrink(lib, p, ncomp=1, y=[p, None, None, None],
                   a=[p, None, None, None]) == 0
    assert _shrink(lib, p, ncomp=2, dtype=C64, mode=1, thresh=0.0) == 0


def test_group_norm_argument_errors(lib, buf):
    p = ctypes.addressof(buf)

    def norm(ncomp=2, x=(p, p, None, None), n=-1, ws=p, out=p, dtype=F64):
        return lib.pam_group_norm(None, ncomp, *x, n, ws, out, dtype)

    assert norm() == EARG                             # n < 0
    assert norm(ncomp=0, n=0) == EARG
    assert norm(ncomp=5, x=(p, p, p, p), n=0) == EARG
    assert norm(ncomp=3, n=0) == EARG                 # third slot is NULL
    assert norm(x=(None, p, None, None), n=0) == EARG
    assert norm(ws=None, n=0) == EARG
    assert norm(out=None, n=0) == EARG
    assert norm(dtype=7, n=0) == EDTYPE


def test_header_binding_and_exports_agree(lib):
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+PAM_GROUP_MAX\s+4\b", src)
    P, L, I, D = (ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                  ctypes.c_double)
    want = {"pam_group_shrink": [P, I, L] + [P] * 12 + [D, L, D, I],
            "pam_group_norm": [P, L] + [P] * 4 + [L, P, P, I]}
    kinds = {"void*": P, "const void*": P, "int64_t": L, "int": I,
             "double": D}
    for name, argtypes in want.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, f"{name} not declared in pam.h"
        declared = [kinds[" ".join(a.split()).replace("*", "* ")
                          .rsplit(None, 1)[0].replace(" *", "*")]
                    for a in m.group(1).split(",")]
        assert declared == argtypes
        assert _ffi._SIGS[name] == (argtypes, I)
        assert hasattr(lib, name)
    assert lib.pam_version() == 1
    assert kernels._GROUP_MAX == 4


def _comps(k, n=12, dtype=torch.float64):
    return [torch.arange(n, dtype=dtype) + c for c in range(k)]


def test_launch_layer_checks_in_order():
    xs, ys = _comps(3), [torch.full((12,), -1.0, dtype=torch.float64)
                         for _ in range(3)]
    mixed = [xs[0], xs[1].to(torch.float32), xs[2]]
    with pytest.raises(TypeError, match="pam_group_shrink"):
        kernels.group_shrink(ys, mixed, 0, 1.5)
    with pytest.raises(TypeError, match="pam_group_shrink"):
        kernels.group_shrink(ys, xs, 0, 1.5, shift=mixed, beta=2.0)
    with pytest.raises(TypeError, match="pam_group_norm"):
        kernels.group_norm(mixed)
    with pytest.raises(TypeError, match="unsupported dtype"):
        kernels.group_norm(_comps(2, dtype=torch.int32))
    for k in (0, 5):
        with pytest.raises(ValueError, match="pam_group_shrink.*components"):
            kernels.group_shrink(_comps(k), _comps(k), 0, 1.5)
        with pytest.raises(ValueError, match="pam_group_norm.*components"):
            kernels.group_norm(_comps(k))
    with pytest.raises(ValueError, match="components"):
        kernels.group_shrink(ys, xs[:2], 0, 1.5)
    with pytest.raises(ValueError, match="components"):
        kernels.group_shrink(ys, xs, 0, 1.5, shift=xs[:2])
    short = [xs[0], xs[1][:11], xs[2]]
    with pytest.raises(ValueError, match="pam_group_shrink.*12 elements"):
        kernels.group_shrink(ys, short, 0, 1.5)
    with pytest.raises(ValueError, match="pam_group_norm.*12 elements"):
        kernels.group_norm(short)
    strided = torch.full((12, 2), -1.0, dtype=torch.float64)[:, 0]
    with pytest.raises(ValueError, match="pam_group_shrink.*contiguous"):
        kernels.group_shrink([ys[0], strided, ys[2]], xs, 0, 1.5)
    # valid CPU operands (inputs may be strided): the device check is last
    xin = [torch.stack([t, t], dim=1)[:, 0] for t in xs]
    with pytest.raises(RuntimeError, match="no CPU compute path"):
        kernels.group_shrink(ys, xin, 0, 1.5)
    with pytest.raises(RuntimeError, match="no CPU compute path"):
        kernels.group_shrink(xs, xs, 1, 1.5, shift=ys, beta=0.5)
    with pytest.raises(RuntimeError, match="no CPU compute path"):
        kernels.group_norm(xin)
    assert all(torch.all(y == -1.0) for y in ys) and \
        torch.all(strided == -1.0)


def test_public_names_importable():
    from pylops_mpi_amd.proximal import MPIL21, MPIProxOperator
    from pylops_mpi_amd.proximal.optimization import PrimalDual
    import pylops_mpi_amd.proximal as prox
    import pylops_mpi_amd.proximal.optimization as po
    assert "MPIL21" in prox.__all__ and "PrimalDual" in po.__all__
    assert callable(PrimalDual)
    op = MPIL21(sigma=0.3)
    assert isinstance(op, MPIProxOperator)
    assert op.accepts_shift is True and op.sigma == 0.3
    assert repr(op) == "<MPIL21>"


def test_mpil21_validation_world1():
    from pylops_mpi_amd.proximal import MPIL21
    from pylops_mpi_amd.comm import PamComm
    op = MPIL21()
    # a CPU communicator of its own: the process-wide default may already
    # sit on a GPU when the whole suite runs there
    comm = PamComm(0, 1, torch.device("cpu"), use_dist=False)

    def arr(n, dtype=np.float64, partition=pm.Partition.SCATTER):
        d = pm.DistributedArray((n,), comm, dtype=dtype,
                                partition=partition)
        d[:] = 1.0
        return d

    for call in (op, lambda v: op.prox(v, 0.5),
                 lambda v: op.proxdual(v, 0.5)):
        with pytest.raises(TypeError, match="StackedDistributedArray"):
            call(arr(6))
        with pytest.raises(ValueError, match="local shapes"):
            call(pm.StackedDistributedArray([arr(6), arr(5)]))
        with pytest.raises(ValueError, match="dtype"):
            call(pm.StackedDistributedArray([arr(6),
                                             arr(6, np.float32)]))
        with pytest.raises(ValueError, match="partition"):
            call(pm.StackedDistributedArray(
                [arr(6), arr(6, partition=pm.Partition.BROADCAST)]))
        with pytest.raises(ValueError, match="1 to 4"):
            call(pm.StackedDistributedArray([arr(6) for _ in range(5)]))
    good = pm.StackedDistributedArray([arr(6), arr(6)])
    with pytest.raises(ValueError, match="components"):
        op.prox(good, 0.5, shift=pm.StackedDistributedArray([arr(6)]))
    with pytest.raises(ValueError, match="local shapes"):
        op.proxdual(good, 0.5, beta=2.0,
                    shift=pm.StackedDistributedArray([arr(5), arr(5)]))
    # a valid stack passes validation and stops at the device check
    with pytest.raises(RuntimeError, match="no CPU compute path"):
        op.prox(good, 0.5)
    with pytest.raises(RuntimeError, match="no CPU compute path"):
        op(good)


def test_primal_dual_show_evaluates_on_every_rank(capsys):
    """The functionals logged by show=True are collectives on distributed
    arrays: every rank has to evaluate them, rank 0 alone prints.  Checked
    with NumPy stand-ins that count the calls."""
    from pylops_mpi_amd.proximal.optimization import PrimalDual

    class Vec:
        def __init__(self, a, rank):
            self.a, self.rank = np.asarray(a, dtype=float), rank

        def copy(self):
            return Vec(self.a.copy(), self.rank)

        def zeros_like(self):
            return Vec(np.zeros_like(self.a), self.rank)

        def __add__(self, o):
            return Vec(self.a + o.a, self.rank)

        def __sub__(self, o):
            return Vec(self.a - o.a, self.rank)

        def __rmul__(self, c):
            return Vec(c * self.a, self.rank)

        def dot(self, o):
            self.ndot = getattr(self, "ndot", 0) + 1
            return float(self.a @ o.a)

    class Eye:
        napply = 0

        def __matmul__(self, v):
            self.napply += 1
            return v.copy()

        H = property(lambda self: self)

    class Prox:
        def __init__(self):
            self.ncall = 0

        def __call__(self, v):
            self.ncall += 1
            return 0.5

        def prox(self, v, tau):
            return v.copy()

        proxdual = prox

    counts = {}
    for rank in (0, 1):
        f, g, A = Prox(), Prox(), Eye()
        z = Vec([0.1, 0.2, 0.3], rank)
        PrimalDual(f, g, A, Vec([1.0, 2.0, 3.0], rank), tau=0.5, mu=0.5,
                   z=z, niter=3, show=True)
        counts[rank] = (f.ncall, g.ncall, A.napply, z.ndot)
        out = capsys.readouterr().out
        if rank == 0:
            assert "Primal-dual" in out
            assert len([ln for ln in out.splitlines()
                        if ln.strip()[:1].isdigit()]) == 3
        else:
            assert out == ""
    assert counts[0] == counts[1] and counts[0][:2] == (3, 3)
    assert counts[0][3] == 3

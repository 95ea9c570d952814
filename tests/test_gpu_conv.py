"""pam_conv1d kernel by kernel: the plain, trace and column kernels, each
forced through PAM_CONV_VARIANT where it is valid, against the NumPy loop
of tests/convref.py (itself checked in tests/test_convref_cpu.py).

Every operand sits in a larger, sentinel-filled device buffer
(primref.Placed), 16-byte aligned or one element off it.  After a launch
the output must equal the reference bit for bit (primref.same: +-0 equal),
its guards must hold the sentinel and the inputs their uploaded bits.
Shapes sit on the kernels' tile edges, read from the tile queries:
d in {1, 2, nh-1, nh, T-1, T, T+1, 2T+3}, m in {1, 3, M-1, M, M+1} and the m
on either side of every change of the automatic dispatch.  Calls go
through pylops_mpi_amd.kernels; a complex128 operand one real off
alignment, which torch cannot express, goes to the C entry point."""
import itertools
import os
from functools import lru_cache

import numpy as np
import pytest
import torch
from numpy.testing import assert_allclose

import convref as cr
import primref as pr
from primref import Placed
import pylops_mpi_amd as pm
from pylops_mpi_amd import _ffi, kernels

pytestmark = pytest.mark.gpu

DT = pr.DTYPES
TORCH = {"f64": torch.float64, "f32": torch.float32,
         "c128": torch.complex128, "c64": torch.complex64}
NHS = (1, 2, 3, 8, 41)
VARIANTS = (0, 1, 2)
MAX_ELEMS = 1 << 20


@pytest.fixture(scope="module", autouse=True)
def _init():
    from pylops_mpi_amd.comm import init_default_comm
    init_default_comm(torch.device("cuda:0"))


@pytest.fixture
def force():
    """force(v) selects a kernel for the calls that follow (None: the
    automatic choice); the environment is restored afterwards."""
    old = os.environ.pop("PAM_CONV_VARIANT", None)

    def set_(v):
        if v is None:
            os.environ.pop("PAM_CONV_VARIANT", None)
        else:
            os.environ["PAM_CONV_VARIANT"] = str(v)
    yield set_
    os.environ.pop("PAM_CONV_VARIANT", None)
    if old is not None:
        os.environ["PAM_CONV_VARIANT"] = old


def offsets(nh):
    return sorted({0, nh // 2, nh - 1})


def real_name(dname):
    return {"c128": "f64", "c64": "f32"}.get(dname, dname)


@lru_cache(maxsize=None)
def crossover_ms(dname, d, nh):
    """Every m below 4096 next to a change of the automatic dispatch for
    [., d, m] blocks, both sides (none while one kernel serves all m)."""
    code = _ffi.dtype_code(TORCH[real_name(dname)])
    k = 2 if pr.is_complex(DT[dname]) else 1
    old = os.environ.pop("PAM_CONV_VARIANT", None)
    try:
        v = [_ffi.lib().pam_conv1d_variant(code, d, k * m, nh)
             for m in range(1, 4097)]
    finally:
        if old is not None:
            os.environ["PAM_CONV_VARIANT"] = old
    out = set()
    for i in range(len(v) - 1):
        if v[i] != v[i + 1]:
            out |= {i + 1, i + 2}
    return sorted(out)


def shapes(variant, dname, nh):
    """(d, m) pairs on the tile edges of ``variant``; for complex blocks
    the edges are those of the doubled real columns."""
    td, tm = kernels.conv1d_tile(variant or 2, TORCH[dname], nh)
    k = 2 if pr.is_complex(DT[dname]) else 1
    ds = sorted({1, 2, nh - 1, nh, td - 1, td, td + 1, 2 * td + 3} - {0})
    ms = {1, 3} | {max(1, (tm + e) // k) for e in (-1, 0, 1)} \
        | {max(1, -(-(tm + 1) // k))}
    out = []
    for d in ds:
        for m in sorted(ms | set(crossover_ms(dname, d, nh))):
            if 3 * d * m * k <= MAX_ELEMS:
                out.append((d, m))
    return out


@lru_cache(maxsize=None)
def data(dname, n, seed):
    """Standard normals with a few exact zeros of either sign; shared and
    read-only."""
    dt = DT[dname]
    rng = np.random.default_rng([seed, n, list(DT).index(dname)])
    x = rng.standard_normal(n)
    if pr.is_complex(dt):
        x = x + 1j * rng.standard_normal(n)
    x = x.astype(dt)
    r = pr.rview(x)
    if r.size >= 16:
        r[(np.arange(4) * 37 + seed) % r.size] = [0.0, -0.0, 0.0, -0.0]
    x.setflags(write=False)
    return x


def reference(x, h, shape, off, adj, deriv):
    """conv1d_ref on the interleaved real view, as the launch layer runs a
    complex block."""
    b, d, m = shape
    k = 2 if pr.is_complex(x.dtype) else 1
    want = cr.conv1d_ref(pr.rview(x).reshape(b, d, k * m), h, off, adj,
                         deriv)
    return want.reshape(-1).view(x.dtype)


def launch(y, x, h, shape, adj, off, deriv):
    b, d, m = shape
    if y.tensor is not None and x.tensor is not None:
        kernels.conv1d(y.tensor.view(b, d, m), x.tensor.view(b, d, m),
                       h.tensor, adj, off, deriv)
        return
    assert y.dtype == np.complex128     # one real off: raw pointers
    rc = _ffi.lib().pam_conv1d(
        torch.cuda.current_stream().cuda_stream, 1 if adj else 0, x.ptr,
        y.ptr, h.ptr, b, d, 2 * m, h.n, off, deriv, _ffi.F64)
    assert rc == 0, rc


def run_case(dname, shape, nh, off, adj, deriv, align, seed=0):
    """One guarded launch -> (output value, message); asserts guards and
    inputs."""
    b, d, m = shape
    x = data(dname, b * d * m, seed)
    h = data(real_name(dname), nh, seed + 1)
    px = Placed(x, align[1])
    ph = Placed(h, align[2])
    py = Placed(np.full(x.size, pr.SENTINEL, dtype=x.dtype), align[0])
    launch(py, px, ph, shape, adj, off, deriv)
    msg = (f"{dname} shape={shape} nh={nh} off={off} adj={adj} "
           f"deriv={deriv} align={align}")
    full = py.fetch()
    assert py.guards_intact(full), f"guard overwritten: {msg}"
    assert px.untouched() and ph.untouched(), f"input changed: {msg}"
    return py.value(full), x, h, msg


def diff(got, want):
    g, w = pr.rview(got), pr.rview(want)
    bad = np.flatnonzero(~((g == w) | (np.isnan(g) & np.isnan(w))))
    return (f"{bad.size} of {g.size} reals differ, first at {bad[:4]}: "
            f"got {g[bad[:4]]}, want {w[bad[:4]]}")


ALIGNS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1))  # y, x, h


def settings(nh):
    """Every (adjoint, deriv, offset, batch), shuffled once per nh."""
    s = list(itertools.product((False, True), (0, 1, 2), offsets(nh),
                               (1, 3)))
    np.random.default_rng(nh).shuffle(s)
    return s


@pytest.mark.parametrize("dname", list(DT))
@pytest.mark.parametrize("variant", VARIANTS)
def test_kernel_matches_reference_bit_for_bit(force, variant, dname):
    """Each (d, m) on a tile edge runs two (or as many as it takes to use
    them all) of the (direction, deriv, offset, batch) settings, taken in
    turn from the shuffled list, so every
    setting meets many shapes and every shape both a short and a long
    filter; the alignments rotate with them."""
    force(variant)
    ran = 0
    for nh in NHS:
        todo = settings(nh)
        valid = [(d, m) for d, m in shapes(variant, dname, nh)
                 if kernels.conv1d_variant(
                     torch.empty((1, d, m), dtype=TORCH[dname],
                                 device="meta"), nh) == variant]
        # (a halo that does not fit makes a shape invalid for a variant)
        reps = max(2, -(-len(todo) // len(valid)))
        i = 0
        for d, m in valid:
            for _ in range(reps):
                adj, deriv, off, b = todo[i % len(todo)]
                align = ALIGNS[i % len(ALIGNS)]
                i += 1
                got, x, h, msg = run_case(dname, (b, d, m), nh, off, adj,
                                          deriv, align, seed=i % 3)
                want = reference(x, h, (b, d, m), off, adj, deriv)
                assert pr.same(got, want), f"{msg}: {diff(got, want)}"
                ran += 1
        assert i >= len(todo), (variant, dname, nh, i)
    assert ran >= 5 * 36, ran


@pytest.mark.parametrize("dname", ("f64", "f32"))
def test_variants_agree_bit_for_bit(force, dname):
    """The three kernels on the same operands, compared with each other
    directly, on shapes that cut the tiles of both tiled kernels."""
    for nh, (d, m) in itertools.product(
            (3, 41), ((131, 67), (300, 5), (2051, 1), (40, 130))):
        for adj, deriv in itertools.product((False, True), (0, 1, 2)):
            outs = []
            for v in VARIANTS:
                force(v)
                blk = torch.empty((2, d, m), dtype=TORCH[dname],
                                  device="meta")
                assert kernels.conv1d_variant(blk, nh) == v
                outs.append(run_case(dname, (2, d, m), nh, nh // 2, adj,
                                     deriv, (0, 0, 0))[0])
            for v in (1, 2):
                assert pr.same(outs[v], outs[0]), \
                    (v, nh, d, m, adj, deriv, diff(outs[v], outs[0]))


@pytest.mark.parametrize("dname", list(DT))
def test_automatic_dispatch_on_both_sides_of_a_crossover(force, dname):
    """With nothing forced: the m on either side of every change of kernel
    (and m = 1, 64, 200 where there is none) gives the reference's bits."""
    force(None)
    nh, d = 41, 96
    for m in sorted({1, 64, 200} | set(crossover_ms(dname, d, nh))):
        for adj, deriv in ((False, 1), (True, 1), (False, 0), (True, 2)):
            got, x, h, msg = run_case(dname, (2, d, m), nh, 20, adj, deriv,
                                      (0, 0, 0))
            want = reference(x, h, (2, d, m), 20, adj, deriv)
            assert pr.same(got, want), f"{msg}: {diff(got, want)}"


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dname", ("f64", "f32", "c64"))
def test_fused_equals_composed(force, variant, dname):
    """forward: fused == conv1d(fd_serial(x)); adjoint: fused ==
    fd_serial(conv1d(x)) — bit for bit, both stencil kinds."""
    force(variant)
    tdt = TORCH[dname]
    fd_ops = {1: (4, 5), 2: (0, 1)}
    for (b, d, m), nh in itertools.product(
            ((1, 1, 1), (2, 2, 3), (3, 131, 67), (1, 2051, 2), (2, 40, 129)),
            (2, 41)):
        x = torch.from_numpy(data(dname, b * d * m, 5).copy()).to(
            "cuda:0").view(b, d, m)
        h = torch.from_numpy(data(real_name(dname), nh, 6).copy()).to(
            "cuda:0")
        assert kernels.conv1d_variant(x, nh) == variant
        for deriv, adj in itertools.product((1, 2), (False, True)):
            fused, t1, t2 = (torch.empty_like(x) for _ in range(3))
            kernels.conv1d(fused, x, h, adj, nh // 2, deriv)
            if adj:
                kernels.conv1d(t1, x, h, True, nh // 2, 0)
                kernels.fd_serial(t2, t1, fd_ops[deriv][1], False, 1.0)
            else:
                kernels.fd_serial(t1, x, fd_ops[deriv][0], False, 1.0)
                kernels.conv1d(t2, t1, h, False, nh // 2, 0)
            got, want = fused.cpu().numpy(), t2.cpu().numpy()
            assert pr.same(got, want), \
                (b, d, m, nh, deriv, adj, diff(got, want))


@pytest.mark.parametrize("variant,dname,shape,nh", (
    (1, "f32", (2, 20, 2000), 41),      # 84000 halo samples
    (1, "f64", (1, 300, 3), 3000),      # 9003 halo samples of 8 bytes
    (2, "f64", (2, 24, 70), 130),       # 131 halo rows of 512 bytes
))
def test_lds_fallback_gives_the_same_bits(force, variant, dname, shape, nh):
    """A forced tiled kernel whose halo outgrows the LDS budget: the query
    reports the plain kernel and the launch produces the reference."""
    force(variant)
    blk = torch.empty(shape, dtype=TORCH[dname], device="meta")
    assert kernels.conv1d_variant(blk, nh) == kernels.CONV_PLAIN
    for adj, deriv in ((False, 0), (True, 1), (False, 2)):
        got, x, h, msg = run_case(dname, shape, nh, nh // 2, adj, deriv,
                                  (0, 0, 0))
        want = reference(x, h, shape, nh // 2, adj, deriv)
        assert pr.same(got, want), f"{msg}: {diff(got, want)}"


# --------------------------------------------------------------- operators
def dev(a):
    return torch.as_tensor(a, device="cuda:0")


def local_ops(dtype="float64"):
    rng = np.random.default_rng(11)
    wav = pm.ricker(np.arange(6) * 0.004, f0=30)[0]
    return [
        pm.Convolve1DLocal((3, 16, 24), rng.standard_normal(8), offset=2,
                           axis=1, dtype=dtype),
        pm.Convolve1DLocal((48, 24), rng.standard_normal(5), offset=4,
                           axis=-1, dtype=dtype),
        pm.PoststackLinearModellingLocal(wav, 16, spatdims=(3, 24), axis=1,
                                         dtype=dtype),
        pm.PoststackLinearModellingLocal(wav, 48, spatdims=24, dtype=dtype,
                                         kind="forward"),
        pm.PoststackLinearModellingLocal(wav, 24, spatdims=48, axis=-1,
                                         dtype=dtype, fused=False),
    ]


@pytest.mark.parametrize("variant", (None, 0, 1, 2))
def test_dottest_through_blockdiag(force, variant):
    force(variant)
    rng = np.random.default_rng(12)
    for op in local_ops():
        Op = pm.MPIBlockDiag([op])
        n = op.shape[0]
        u = pm.DistributedArray.to_dist(dev(rng.standard_normal(n)))
        v = pm.DistributedArray.to_dist(dev(rng.standard_normal(n)))
        assert pm.dottest(Op, u, v, rtol=1e-10)
    for op in local_ops("complex128")[:3]:
        Op = pm.MPIBlockDiag([op])
        n = op.shape[0]
        u, v = (pm.DistributedArray.to_dist(dev(
            rng.standard_normal(n) + 1j * rng.standard_normal(n)))
            for _ in range(2))
        assert pm.dottest(Op, u, v, rtol=1e-10)


def test_blockdiag_applies_the_local_operator():
    """MPIBlockDiag([op]) x is op on the local block, and that is the
    reference; a NumPy filter moves to the device on first use."""
    rng = np.random.default_rng(13)
    for op in local_ops():
        Op = pm.MPIBlockDiag([op])
        xg = rng.standard_normal(op.shape[1])
        x = pm.DistributedArray.to_dist(dev(xg))
        for name, adj in (("matvec", False), ("rmatvec", True)):
            y = getattr(Op, name)(x)
            local = getattr(op, name)(x.local_array)
            assert torch.equal(y.local_array, local)
            want = cr.conv1d_ref(
                xg.reshape(op.batch, op.d, op.m), op.h.cpu().numpy(),
                op.offset, adj, op._deriv)
            assert pr.same(local.cpu().numpy(), want.ravel()), (op.dims, name)
        assert op.h.is_cuda


def test_cgls_cost_trace_matches_dense_recurrence():
    """5 CGLS iterations on a 3 x 16 x 24 post-stack problem: the cost
    trace against the same recurrence in NumPy on the dense matrix built
    from conv1d_ref; rtol as the CGLS trace check of smoke()."""
    dims, niter, damp = (3, 16, 24), 5, 0.1
    n = int(np.prod(dims))
    wav = pm.ricker(np.arange(6) * 0.004, f0=30)[0]
    op = pm.PoststackLinearModellingLocal(wav, 16, spatdims=(3, 24), axis=1)
    Op = pm.MPIBlockDiag([op])
    rng = np.random.default_rng(14)
    yg = rng.standard_normal(n)
    # dense matrix: identity columns as batches of one reference call
    eye = np.eye(n).reshape(n * dims[0], dims[1], dims[2])
    A = cr.conv1d_ref(eye, wav, len(wav) // 2, False, 1).reshape(n, n).T

    x = np.zeros(n)
    s = yg - A @ x
    r = A.T @ s - damp * x
    c = r.copy()
    q = A @ c
    kold = r @ r
    want = [np.linalg.norm(s)]
    for _ in range(niter):
        a = kold / (q @ q + damp ** 2 * (c @ c))
        x = x + a * c
        s = s - a * q
        r = A.T @ s - damp ** 2 * x
        k = r @ r
        c = r + (k / kold) * c
        q = A @ c
        kold = k
        want.append(np.linalg.norm(s))

    yd = pm.DistributedArray.to_dist(dev(yg))
    x0 = pm.DistributedArray((n,), dtype=np.float64)
    x0[:] = 0.0
    xs, _, _, _, _, cost = pm.cgls(Op, yd, x0, niter=niter, damp=damp,
                                   tol=0.0)
    assert_allclose(np.asarray(cost), np.asarray(want), rtol=1e-10)
    assert_allclose(xs.asarray().cpu().numpy(), x, rtol=1e-8, atol=1e-10)

"""GPU parity for the L2,1 group kernels (pam_group_shrink /
pam_group_norm), MPIL21 and PrimalDual at world size 1.

Expected values are NumPy closed forms restated here, evaluated in the
array's own dtype and in the kernel's documented order (components
ascending, |z|^2 = re^2 + im^2), so the tolerances only have to cover a
handful of correctly rounded operations:
  rho = sqrt(sum_c |v_c|^2)
  mode 0: s = (rho - t) / rho if rho > t else 0      (prox of t*||.||_2,1)
  mode 1: s = t / rho         if rho > t else 1      (L2-ball projection)
and a dozen-line Chambolle-Pock on dense per-axis difference matrices.

Branch coverage is asserted on the reference: for every case with
n >= 255, between 10% and 90% of the groups lie on each side of
rho > thresh (with n = 1 or 3 a share cannot be bounded that way: the one
zero group alone is 100% or 33% of them)."""
from functools import lru_cache

import numpy as np
import pytest
import torch
from numpy.testing import assert_allclose

import oracle
import pylops_mpi_amd as pm
from pylops_mpi_amd import kernels
from pylops_mpi_amd.proximal import L1, MPIL2, MPIL21, MPIProxOperator
from pylops_mpi_amd.proximal.optimization import PrimalDual

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 255, 256, 257, 1031)     # vector-tail and block-edge sizes
BIG = 262144 + 513                      # > NPARTIAL * BLK: stage 1 strides
THRESH = 1.5
DTYPES = {"f64": np.float64, "f32": np.float32,
          "c128": np.complex128, "c64": np.complex64}
TOL = {"f64": dict(rtol=1e-13, atol=1e-15), "c128": dict(rtol=1e-13,
                                                         atol=1e-15),
       "f32": dict(rtol=1e-6, atol=1e-7), "c64": dict(rtol=1e-6, atol=1e-7)}


@pytest.fixture(scope="module", autouse=True)
def _init():
    from pylops_mpi_amd.comm import init_default_comm
    init_default_comm(torch.device("cuda:0"))


def host(t):
    return t.cpu().numpy()


def dev(a):
    return torch.as_tensor(np.array(a), device="cuda:0")


def place(arrs, offset=0):
    """Device copies of ``arrs``; ``offset=1`` makes each a view starting
    one element into a larger buffer (8 / 4 / 8 bytes off 16-byte
    alignment for f64 / f32 / c64: the scalar kernels; a complex128
    element is 16 bytes, so that dtype stays on the vector path)."""
    out = []
    for a in arrs:
        src = torch.from_numpy(np.array(a))
        buf = torch.empty(a.size + 1, dtype=src.dtype, device="cuda:0")
        t = buf[offset:offset + a.size]
        t.copy_(src)
        out.append(t)
    return out


def draw(rng, dt, ncomp, n):
    comps = []
    for _ in range(ncomp):
        v = rng.standard_normal(n)
        if np.issubdtype(dt, np.complexfloating):
            # the complex standard normal: E|z|^2 = 1, parts of variance 1/2
            v = (v + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
        v = v.astype(dt)
        v[n // 2] = 0
        v.setflags(write=False)
        comps.append(v)
    return tuple(comps)


@lru_cache(maxsize=None)
def data(dname, ncomp, n, seed=0):
    """ncomp standard-normal components of n elements, one group all
    zeros.  Shared and never modified.  With THRESH = 1.5 the expected
    share of groups at or below the threshold runs from 0.87 (one real
    component) and 0.89 (one complex) down to 0.19 (four complex), so a
    few hundred draws can land outside the 10%..90% band the tests
    require of the reference: such a draw is rejected and redrawn —
    deterministically, and judged on the NumPy reference alone."""
    rng = np.random.default_rng([seed, ncomp, n, list(DTYPES).index(dname)])
    for _ in range(200):
        comps = draw(rng, DTYPES[dname], ncomp, n)
        if n < 255 or 0.1 <= (np_rho(comps) > THRESH).mean() <= 0.9:
            return comps
    raise AssertionError("no draw covers both branches")


def np_rho(vs):
    acc = np.zeros(vs[0].shape, dtype=vs[0].real.dtype)
    for v in vs:
        if np.iscomplexobj(v):
            acc = acc + (v.real * v.real + v.imag * v.imag)
        else:
            acc = acc + v * v
    return np.sqrt(acc)


def np_shrink(vs, mode, thresh):
    rho = np_rho(vs)
    thresh = rho.dtype.type(thresh)
    above = rho > thresh
    safe = np.where(above, rho, rho.dtype.type(1))
    if mode == 0:
        s = np.where(above, (safe - thresh) / safe, rho.dtype.type(0))
    else:
        s = np.where(above, thresh / safe, rho.dtype.type(1))
    return [v * s for v in vs], above


def np_norm21(vs):
    q = sum(np.abs(v.astype(np.complex128)) ** 2 for v in vs)
    return float(np.sum(np.sqrt(q)))


# ------------------------------------------------------------ group_shrink
@pytest.mark.parametrize("ncomp", [1, 2, 3, 4])
@pytest.mark.parametrize("dname", list(DTYPES))
def test_group_shrink_vs_numpy(dname, ncomp):
    for n in SIZES:
        vs = data(dname, ncomp, n)
        for mode in (0, 1):
            want, above = np_shrink(vs, mode, THRESH)
            if n >= 255:
                assert 0.1 <= above.mean() <= 0.9, (n, above.mean())
            for offset in (0, 1):
                xs = place(vs, offset)
                ys = place([np.full_like(v, 7) for v in vs], offset)
                kernels.group_shrink(ys, xs, mode, THRESH)
                for c in range(ncomp):
                    got = host(ys[c])
                    assert_allclose(got, want[c], **TOL[dname],
                                    err_msg=f"n={n} mode={mode} c={c} "
                                            f"offset={offset}")
                    assert got[n // 2] == 0 and not np.isnan(got).any()
                    assert torch.equal(xs[c], dev(vs[c]))  # inputs intact
                # in place: bitwise the out-of-place result
                kernels.group_shrink(xs, xs, mode, THRESH)
                for c in range(ncomp):
                    assert torch.equal(xs[c], ys[c]), (n, mode, c, offset)


@pytest.mark.parametrize("dname", list(DTYPES))
def test_group_shrink_fused_shift_is_scale_add_shrink(dname):
    beta = 0.37
    for ncomp in (1, 2, 3, 4):
        for n in SIZES:
            vs, ws = data(dname, ncomp, n), data(dname, ncomp, n, seed=1)
            for mode, offset in ((0, 0), (1, 1), (0, 1), (1, 0)):
                xs, sh = place(vs, offset), place(ws, offset)
                fused = [torch.empty_like(t) for t in xs]
                kernels.group_shrink(fused, xs, mode, THRESH, shift=sh,
                                     beta=beta)
                plain = []
                for x, w in zip(xs, sh):
                    t = torch.empty_like(x)
                    kernels.scale(t, w, beta)
                    kernels.add(t, x, t)
                    plain.append(t)
                kernels.group_shrink(plain, plain, mode, THRESH)
                for c in range(ncomp):
                    assert torch.equal(fused[c], plain[c]), \
                        (ncomp, n, mode, offset, c)


@pytest.mark.parametrize("ncomp", [1, 2, 3, 4])
def test_group_shrink_complex128_scalar_path(ncomp):
    """A complex128 tensor is always 16-byte aligned (torch refuses a
    complex view at an odd real offset), so the scalar complex128 kernels
    are reached through the C-ABI: float64 buffers read as complex128
    from one real (8 bytes) in."""
    from pylops_mpi_amd import _ffi
    for n in SIZES:
        vs, ws = data("c128", ncomp, n), data("c128", ncomp, n, seed=1)

        def bufs(arrs):     # 2n reals starting at real 1 of 2n + 1
            out = []
            for a in arrs:
                b = torch.full((2 * n + 1,), 7.0, dtype=torch.float64,
                               device="cuda:0")
                b[1:].copy_(torch.from_numpy(np.array(a).view(np.float64)))
                assert b[1:].data_ptr() % 16 == 8
                out.append(b)
            return out

        def slots(bs):
            return [b[1:].data_ptr() for b in bs] + [None] * (4 - ncomp)

        stream = torch.cuda.current_stream().cuda_stream
        for mode in (0, 1):
            for shift, beta in ((None, 1.0), (ws, 0.37)):
                xs, ys = bufs(vs), bufs(vs)
                sh = bufs(shift) if shift else []
                rc = _ffi.lib().pam_group_shrink(
                    stream, mode, ncomp, *slots(ys), *slots(xs),
                    *(slots(sh) if sh else [None] * 4), beta, n, THRESH,
                    _ffi.C128)
                assert rc == 0
                v = vs if shift is None else [
                    a + np.float64(beta) * b for a, b in zip(vs, shift)]
                want, _ = np_shrink(v, mode, THRESH)
                for c in range(ncomp):
                    got = host(ys[c])
                    assert got[0] == 7.0            # nothing before the view
                    assert_allclose(got[1:].view(np.complex128), want[c],
                                    **TOL["c128"])


def test_one_real_component_is_soft_threshold():
    for n in SIZES:
        (v,) = data("f64", 1, n)
        (x,) = place([v])
        y, z = torch.empty_like(x), torch.empty_like(x)
        kernels.group_shrink([y], [x], 0, THRESH)
        kernels.thresh(z, x, 0, THRESH)
        assert_allclose(host(y), host(z), **TOL["f64"])


def test_zero_elements_is_a_no_op():
    e = torch.empty(0, dtype=torch.float64, device="cuda:0")
    kernels.group_shrink([e, e], [e, e], 0, THRESH)


# -------------------------------------------------------------- group_norm
@pytest.mark.parametrize("dname", list(DTYPES))
def test_group_norm_vs_numpy(dname):
    for ncomp in (1, 2, 3, 4):
        for n in SIZES + ((BIG,) if ncomp == 3 else ()):
            vs = data(dname, ncomp, n)
            for offset in (0, 1):
                xs = place(vs, offset)
                first = kernels.group_norm(xs).clone()
                again = kernels.group_norm(xs)
                assert torch.equal(first, again)      # deterministic tree
                assert_allclose(first.item(), np_norm21(vs), rtol=1e-12,
                                err_msg=f"ncomp={ncomp} n={n}")
                out = torch.full((1,), -1.0, dtype=torch.float64,
                                 device="cuda:0")
                assert kernels.group_norm(xs, out=out) is out
                assert torch.equal(out, first)


# ------------------------------------------------------------------ MPIL21
def stack(arrs, partition=pm.Partition.SCATTER):
    return pm.StackedDistributedArray(
        [pm.DistributedArray.to_dist(dev(a), partition=partition)
         for a in arrs])


def check_layout(y, x):
    assert isinstance(y, pm.StackedDistributedArray)
    assert y.narrays == x.narrays
    for a, b in zip(y.distarrays, x.distarrays):
        assert a.partition == b.partition and a.dtype == b.dtype
        assert a.local_shapes == b.local_shapes
        assert a.global_shape == b.global_shape


def check_l21(op, x, sigma, tau):
    vs = [host(d.asarray()).ravel() for d in x.distarrays]
    f = op(x)
    assert isinstance(f, float)
    assert_allclose(f, sigma * np_norm21(vs), rtol=1e-12)
    y = op.prox(x, tau)
    check_layout(y, x)
    want, above = np_shrink(vs, 0, sigma * tau)
    assert 0.1 <= above.mean() <= 0.9
    for c in range(x.narrays):
        assert_allclose(host(y[c].asarray()).ravel(), want[c], **TOL["f64"])
    y = op.proxdual(x, tau)
    check_layout(y, x)
    want, above = np_shrink(vs, 1, sigma)
    assert 0.1 <= above.mean() <= 0.9
    for c in range(x.narrays):
        assert_allclose(host(y[c].asarray()).ravel(), want[c], **TOL["f64"])


def test_mpil21_on_gradient_output():
    dims = (9, 8, 7)
    rng = np.random.default_rng(11)
    x = pm.DistributedArray.to_dist(dev(rng.standard_normal(
        int(np.prod(dims)))))
    g = pm.MPIGradient(dims) @ x
    assert g.narrays == 3
    check_l21(MPIL21(sigma=0.8), g, 0.8, 0.9)


def test_mpil21_on_broadcast_stack():
    rng = np.random.default_rng(12)
    x = stack([rng.standard_normal(301) for _ in range(2)],
              partition=pm.Partition.BROADCAST)
    assert x[0].partition == pm.Partition.BROADCAST
    check_l21(MPIL21(sigma=1.2), x, 1.2, 0.7)


def test_mpil21_moreau_identity_and_shift():
    sigma, tau = 1.3, 0.7
    op = MPIL21(sigma=sigma)
    vs = data("f64", 3, 1031)
    x = stack(vs)
    got = op.prox(x, tau) + tau * op.proxdual((1.0 / tau) * x, 1.0 / tau)
    for c in range(3):
        assert_allclose(host(got[c].asarray()), vs[c], **TOL["f64"])
    # shift=v, beta=b evaluates at x + b * v in the same pass
    v = stack(data("f64", 3, 1031, seed=1))
    for fn in (op.prox, op.proxdual):
        fused, plain = fn(x, tau, shift=v, beta=0.4), fn(x + 0.4 * v, tau)
        check_layout(fused, x)
        for c in range(3):
            assert torch.equal(fused[c].local_array, plain[c].local_array)


# -------------------------------------------------------------- PrimalDual
DIMS = (16, 12)
SIGMA = 0.3
STEP = 0.99 / 8.0 ** 0.5


@lru_cache(maxsize=None)
def tv_problem():
    n = int(np.prod(DIMS))
    img = np.zeros(DIMS)
    img[4:11, 3:9] = 1.0                               # two-level image
    noisy = (img + 0.2 * np.random.default_rng(5).standard_normal(DIMS)
             ).ravel()

    def axis_fd(v, axis):
        vg = np.moveaxis(v.reshape(DIMS), axis, 0)
        y = oracle.serial_fd1_matvec(vg, 1.0, "forward", False, 3)
        return np.moveaxis(y, 0, axis).ravel()

    D = [oracle.dense_matrix_from_matvec(lambda v, ax=ax: axis_fd(v, ax), n)
         for ax in range(2)]
    return noisy, D


def np_primal_dual(b, D, dualprox, niter, gfirst, tau=STEP, mu=STEP,
                   theta=1.0, z=0.0, y0=None):
    """Chambolle-Pock for 0.5 ||x - b||^2 + z.x + g(D x), x0 = b."""
    x, xhat = b.copy(), b.copy()
    y = np.zeros((len(D), b.size)) if y0 is None else y0.copy()

    def dual(y, xhat):
        return dualprox(y + mu * np.stack([Dk @ xhat for Dk in D]))

    def primal(x, y):
        ATy = sum(Dk.T @ yk for Dk, yk in zip(D, y)) + z
        xn = (1.0 / (1.0 + tau)) * ((x - tau * ATy) + tau * b)
        return xn, xn + theta * (xn - x)

    for _ in range(niter):
        if gfirst:
            y = dual(y, xhat)
            x, xhat = primal(x, y)
        else:
            x, xhat = primal(x, y)
            y = dual(y, xhat)
    return x, y


def tv_objective(x, b, D):
    return 0.5 * np.sum((x - b) ** 2) + SIGMA * np_norm21(
        [Dk @ x for Dk in D])


@pytest.mark.parametrize("gfirst", [True, False])
def test_primal_dual_tv_vs_numpy(gfirst):
    noisy, D = tv_problem()
    bd = pm.DistributedArray.to_dist(dev(noisy))
    A = pm.MPIGradient(DIMS, kind="forward")
    proxg = MPIL21(sigma=SIGMA)
    seen = []
    x, y = PrimalDual(MPIL2(b=bd), proxg, A, bd, tau=STEP, mu=STEP,
                      niter=30, gfirst=gfirst, returny=True,
                      callback=seen.append)
    want_x, want_y = np_primal_dual(
        noisy, D, lambda v: np.stack(np_shrink(list(v), 1, SIGMA)[0]),
        30, gfirst)
    assert isinstance(x, pm.DistributedArray) and len(seen) == 30
    assert isinstance(y, pm.StackedDistributedArray) and y.narrays == 2
    assert_allclose(host(x.asarray()), want_x, rtol=1e-10, atol=1e-12)
    for c in range(2):
        assert_allclose(host(y[c].asarray()), want_y[c], rtol=1e-10,
                        atol=1e-12)
    assert tv_objective(host(x.asarray()), noisy, D) < \
        tv_objective(noisy, noisy, D)
    # without returny: x alone, the same iterate
    x2 = PrimalDual(MPIL2(b=bd), proxg, A, bd, tau=STEP, mu=STEP, niter=30,
                    gfirst=gfirst)
    assert torch.equal(x2.local_array, x.local_array)


def test_primal_dual_separable_prox_takes_plain_path():
    noisy, D = tv_problem()
    bd = pm.DistributedArray.to_dist(dev(noisy))
    proxg = MPIProxOperator(L1(SIGMA))
    assert not getattr(proxg, "accepts_shift", False)
    x, y = PrimalDual(MPIL2(b=bd), proxg, pm.MPIGradient(DIMS,
                                                         kind="forward"),
                      bd, tau=STEP, mu=STEP, niter=30, returny=True)

    def l1_dual(v):     # Moreau: v - mu * soft(v / mu, sigma / mu)
        return v - STEP * oracle.soft_threshold(v / STEP, SIGMA / STEP)

    want_x, want_y = np_primal_dual(noisy, D, l1_dual, 30, True)
    assert_allclose(host(x.asarray()), want_x, rtol=1e-10, atol=1e-12)
    for c in range(2):
        assert_allclose(host(y[c].asarray()), want_y[c], rtol=1e-10,
                        atol=1e-12)


def test_primal_dual_linear_term_start_and_show(capsys):
    noisy, D = tv_problem()
    rng = np.random.default_rng(6)
    z = 0.1 * rng.standard_normal(noisy.size)
    y0 = 0.1 * rng.standard_normal((2, noisy.size))
    bd = pm.DistributedArray.to_dist(dev(noisy))
    x = PrimalDual(MPIL2(b=bd), MPIL21(sigma=SIGMA),
                   pm.MPIGradient(DIMS, kind="forward"), bd, tau=STEP,
                   mu=0.5 * STEP, theta=0.8, niter=4, show=True,
                   z=pm.DistributedArray.to_dist(dev(z)), y0=stack(y0))
    want, _ = np_primal_dual(
        noisy, D, lambda v: np.stack(np_shrink(list(v), 1, SIGMA)[0]), 4,
        True, mu=0.5 * STEP, theta=0.8, z=z, y0=y0)
    assert_allclose(host(x.asarray()), want, rtol=1e-10, atol=1e-12)
    out = capsys.readouterr().out
    assert "Proximal operator (g): <MPIL21>" in out
    assert len([ln for ln in out.splitlines()
                if ln.strip()[:1].isdigit()]) == 4    # one line per iterate

"""The references of tests/primref.py checked on their own, without a GPU:
against higher precision, against oracle.soft_threshold / hard_threshold /
half_threshold, and — for the bit-exact family — against the fused
evaluation they must be able to tell apart from the unfused one."""
import math

import numpy as np
import pytest
import torch
from numpy.testing import assert_allclose

import oracle
import primref as pr

N = 4099
ALPHA = 0.7             # not representable in float32


def draw(dname, n=N, seed=0):
    rng = np.random.default_rng([seed, list(pr.DTYPES).index(dname)])
    x = rng.standard_normal(n)
    if pr.is_complex(pr.DTYPES[dname]):
        x = x + 1j * rng.standard_normal(n)
    return x.astype(pr.DTYPES[dname])


@pytest.mark.parametrize("dname", list(pr.DTYPES))
def test_realview_refs_vs_float64(dname):
    dt = pr.DTYPES[dname]
    x, y = draw(dname), draw(dname, seed=1)
    wide = np.complex128 if pr.is_complex(dt) else np.float64
    xw, yw = x.astype(wide), y.astype(wide)
    a = float(pr.real_type(dt)(ALPHA))
    tol = dict(rtol=0, atol=4 * pr.eps(dt) * 8.0)     # |x|, |y| < 8
    assert pr.same(pr.add(x, y), x + y) and pr.same(pr.sub(x, y), x - y)
    assert pr.same(pr.neg(x), -x)
    assert_allclose(pr.scale(x, ALPHA), a * xw, **tol)
    assert_allclose(pr.axpy(y, x, ALPHA), yw + a * xw, **tol)
    assert_allclose(pr.xpby(y, x, ALPHA), xw + a * yw, **tol)
    assert pr.same(pr.axpy_d(y, x, ALPHA, -1.0), pr.axpy(y, x, -ALPHA))
    assert pr.same(pr.xpby_d(y, x, ALPHA, 1.0), pr.xpby(y, x, ALPHA))
    for r in (pr.add(x, y), pr.scale(x, ALPHA), pr.axpy(y, x, ALPHA)):
        assert r.dtype == dt and r.shape == x.shape
    f = pr.fill(5, ALPHA, dt)
    assert f.dtype == dt and np.all(pr.rview(f) == pr.real_type(dt)(ALPHA))


@pytest.mark.parametrize("dname", ["f64", "f32"])
def test_axpy_ref_rounds_the_product(dname):
    """The unfused y + fl(a*x) and a fused multiply-add differ on random
    data: a kernel that contracts cannot match the reference bit for bit.
    The fused value is formed exactly in longdouble / float64 and rounded
    once."""
    dt = pr.DTYPES[dname]
    x, y = draw(dname), draw(dname, seed=1)
    wide = np.longdouble if dt is np.float64 else np.float64
    fused = (y.astype(wide) + wide(dt(ALPHA)) * x.astype(wide)).astype(dt)
    unfused = pr.axpy(y, x, ALPHA)
    differ = np.count_nonzero(fused != unfused)
    assert 0 < differ < N // 2
    # and never by more than one unit in the last place of the larger term
    assert np.all(np.abs(fused - unfused)
                  <= pr.eps(dt) * (np.abs(y) + np.abs(x)))


@pytest.mark.parametrize("dname", ["c128", "c64"])
def test_complex_refs(dname):
    dt = pr.DTYPES[dname]
    a, b = draw(dname), draw(dname, seed=1)
    aw, bw = a.astype(np.complex128), b.astype(np.complex128)
    tol = dict(rtol=0, atol=4 * pr.eps(dt) * 32.0)
    assert_allclose(pr.cmul(a, b), aw * bw, **tol)
    assert pr.same(pr.mul(a, b), pr.cmul(a, b))
    alpha = complex(ALPHA, -1.3)
    R = pr.real_type(dt)
    assert_allclose(pr.cscale(a, alpha),
                    aw * complex(R(alpha.real), R(alpha.imag)), **tol)
    assert pr.same(pr.conj(a), np.conj(a))
    # the parts are not interchangeable: a swapped (ar, ai) is far off
    assert not np.allclose(pr.cscale(a, alpha),
                           pr.cscale(a, complex(alpha.imag, alpha.real)))
    assert pr.cmul(a, b).dtype == dt and pr.cscale(a, alpha).dtype == dt


def test_scalar_refs():
    assert pr.scalar_alpha(-3.0, 2.0, 4.0, 0.5) == 0.75
    assert pr.scalar_alpha(3.0, -2.0, 9.0, 0.0) == 1.5
    assert pr.scalar_div(-1.0, 3.0) == abs(-1.0 / 3.0)


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("dname", list(pr.DTYPES))
def test_threshold_refs_vs_oracle(dname, kind):
    dt, t = pr.DTYPES[dname], 0.7
    rng = np.random.default_rng([3, kind, list(pr.DTYPES).index(dname)])
    for n in (1, 257, 1025):
        x = pr.thresh_data(rng, dt, n, kind, t)
        assert x.dtype == dt and x.size == n
        te = pr.cast_thresh(t, dt)
        assert pr.thresh_margin(x, kind, te) >= 1e-3
        wide = x.astype(np.complex128 if pr.is_complex(dt) else np.float64)
        want = (oracle.soft_threshold, oracle.hard_threshold,
                oracle.half_threshold)[kind](wide, te)
        got = pr.THRESH_REF[kind](x, t)
        # float32 references evaluate in float32: a few roundings from the
        # float64 oracle; everything else is the oracle's own arithmetic
        tol = (4 * pr.eps(dt) if dname == "f32" and kind == 0 else 1e-15)
        assert_allclose(got, want, rtol=tol, atol=tol)
        if n >= 257:    # both branches are present
            assert 0.02 < np.mean(want == 0) < 0.98, np.mean(want == 0)
            assert x[n // 2] == 0 and got[n // 2] == 0


def test_real_soft_ref_propagates_nan():
    for dt in (np.float64, np.float32):
        x = np.array([1.0, np.nan, -2.0], dtype=dt)
        got = pr.soft(x, 0.5)
        assert np.isnan(got[1]) and got[0] == dt(0.5) and got[2] == dt(-1.5)
        assert np.isnan(oracle.soft_threshold(x, 0.5)[1])


def test_decision_points():
    assert pr.decision_point(0, 0.7) == 0.7
    assert pr.decision_point(1, 0.7) == math.sqrt(1.4)
    assert_allclose(pr.decision_point(2, 0.7), 0.9449407874211548
                    * 0.7 ** (2.0 / 3.0), rtol=1e-15)


def test_reduction_terms_and_sums():
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal(N), rng.standard_normal(N)
    s, bound = pr.lsum(pr.dot_terms(x, y))
    exact = math.fsum(pr.dot_terms(x, y))
    assert abs(float(s) - exact) <= 2.0 ** -60 * abs(exact) + 1e-300
    assert_allclose(float(bound), N * 2.0 ** -53 * math.fsum(
        np.abs(pr.dot_terms(x, y))), rtol=1e-14)
    # integer data: every reference is the integer result
    xi = rng.integers(-4, 5, N).astype(np.float32)
    yi = rng.integers(-4, 5, N).astype(np.float32)
    assert pr.lsum(pr.dot_terms(xi, yi))[0] == int(
        np.dot(xi.astype(np.int64), yi.astype(np.int64)))
    z = (xi + 1j * yi).astype(np.complex64)
    w = (yi - 1j * xi).astype(np.complex64)
    for conjx in (0, 1):
        re, im = pr.cdot_terms(z, w, conjx)
        want = np.sum((np.conj(z) if conjx else z).astype(np.complex128)
                      * w.astype(np.complex128))
        assert (pr.lsum(re)[0], pr.lsum(im)[0]) == (want.real, want.imag)
    assert pr.lsum(pr.powsum_terms(z, 2))[0] == np.sum(
        xi.astype(np.int64) ** 2 + yi.astype(np.int64) ** 2)
    assert pr.lsum(pr.powsum_terms(xi, 1))[0] == np.sum(np.abs(xi))
    # general terms against float_power
    zc = (x + 1j * y)
    for p in (1, 2, 3, 0.5):
        assert_allclose(pr.powsum_terms(zc, p).astype(np.float64),
                        np.abs(np.float_power(zc, p)), rtol=1e-14)
        with np.errstate(invalid="ignore"):     # x < 0, p = 0.5: NaN
            want = np.abs(np.float_power(x, p))
        assert np.isnan(want).any() == (p == 0.5)
        assert_allclose(pr.powsum_terms(x, p).astype(np.float64), want,
                        rtol=1e-14)
        assert_allclose(pr.powsum_terms(np.abs(x), p).astype(np.float64),
                        np.abs(x) ** p, rtol=1e-14)
    assert_allclose(pr.abs_terms(zc).astype(np.float64), np.abs(zc),
                    rtol=1e-15)
    assert pr.count_nonzero(np.array([0.0, np.nan, -0.0, 2.0])) == 2.0


def test_gemv_ref():
    rng = np.random.default_rng(6)
    A = rng.integers(-4, 5, (65, 255)).astype(np.float32)
    for trans in (0, 1):
        x = rng.integers(-4, 5, A.shape[0] if trans else A.shape[1]
                         ).astype(np.float32)
        ref, bound = pr.gemv(A, x, trans)
        Ai = A.astype(np.int64)
        want = (Ai.T if trans else Ai) @ x.astype(np.int64)
        assert np.array_equal(ref.astype(np.int64), want)
        assert ref.shape == bound.shape and np.all(bound >= 0)
    Ar = rng.standard_normal((7, 5))
    xr = rng.standard_normal(7)
    ref, bound = pr.gemv(Ar, xr, 1)
    assert_allclose(ref.astype(np.float64), Ar.T @ xr, rtol=1e-13)
    assert np.all(bound < 1e-13)


def test_same_compares_slot_by_slot():
    a = np.array([0.0, np.nan, 1.0])
    assert pr.same(a, np.array([-0.0, np.nan, 1.0]))
    assert not pr.same(a, np.array([0.0, 1.0, 1.0]))
    assert not pr.same(a, a.astype(np.float32))
    assert not pr.same(np.array([complex(np.nan, 1.0)]),
                       np.array([complex(np.nan, 2.0)]))
    assert not pr.same(np.array([complex(np.nan, 1.0)]),
                       np.array([complex(1.0, np.nan)]))


@pytest.mark.parametrize("dname", list(pr.DTYPES))
def test_placement_on_host(dname):
    """Placed on the CPU device: offsets, views, guards."""
    dt = pr.DTYPES[dname]
    itemsize = np.dtype(pr.real_type(dt)).itemsize
    for n in (0, 1, 5):
        x = draw(dname, n)
        for off in (0, 1):
            p = pr.Placed(x, off, device="cpu")
            assert pr.GUARD * itemsize >= 32 and p.lo >= pr.GUARD
            assert p.ptr % 16 == (0 if off == 0 else 4 if dname == "f32"
                                  else 8)
            assert p.untouched() and p.guards_intact()
            assert pr.same(p.value(), x)
            if dname == "c128" and off:
                assert p.tensor is None
                continue
            assert p.tensor.shape == (n,)
            assert pr.same(p.tensor.numpy(), x)
            if n:
                assert p.tensor.data_ptr() == p.ptr
                p.tensor[0] = 3.0           # the view writes the buffer
                assert p.guards_intact() and not p.untouched()
                assert p.value()[0] == 3.0
            p.buf[p.hi] = 1.0               # one past the end
            assert not p.guards_intact()
            q = pr.Placed(x, off, device="cpu")
            q.buf[q.lo - 1] = -pr.SENTINEL  # one before the start
            assert not q.guards_intact()
    assert torch.tensor(pr.SENTINEL, dtype=torch.float32).item() \
        == pr.SENTINEL

"""The NumPy loops of tests/kirchref.py, on their own: a hand-worked pair,
the dense matrix, the dot test, chunking and the skip rules."""
import numpy as np
import pytest

import kirchref as kr

DTYPES = (np.float64, np.float32)


def tables(rng, ns, nr, ni, nt, dtype):
    """Random tables in samples whose sums spread over [-2, nt + 2)."""
    qs = rng.uniform(-1.0, (nt + 2) / 2.0, (ns, ni))
    qr = rng.uniform(-1.0, (nt + 2) / 2.0, (nr, ni))
    return qs.astype(dtype), qr.astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_hand_worked_pair(dtype):
    """One point, one co-located source / receiver pair 1.625 samples away
    each way: q = 3.25."""
    qs = np.array([[1.625]], dtype=dtype)
    d = kr.spread_ref(np.array([1.0], dtype=dtype), qs, qs, 8)
    assert d.shape == (1, 1, 8) and d.dtype == dtype
    assert d.ravel().tolist() == [0, 0, 0, 0.75, 0.25, 0, 0, 0]
    assert kr.spread_count(qs, qs, 8).ravel().tolist() == \
        [0, 0, 0, 1, 1, 0, 0, 0]
    data = np.arange(8, dtype=dtype).reshape(1, 1, 8)
    assert kr.gather_ref(data, qs, qs).tolist() == [0.75 * 3 + 0.25 * 4]


def test_equals_the_dense_matrix_and_its_transpose():
    rng = np.random.default_rng(0)
    ns, nr, ni, nt = 2, 3, 7, 9
    qs, qr = tables(rng, ns, nr, ni, nt, np.float64)
    A = kr.dense(qs, qr, nt)
    assert A.shape == (ns * nr * nt, ni)
    # weights of a contributing pair sum to one, others to nothing
    sums = A.reshape(ns * nr, nt, ni).sum(axis=1)
    assert np.all((np.abs(sums - 1) < 1e-15) | (sums == 0))
    assert 0 < np.count_nonzero(sums) < sums.size
    m = rng.standard_normal(ni)
    d = rng.standard_normal((ns, nr, nt))
    np.testing.assert_allclose(kr.spread_ref(m, qs, qr, nt).ravel(), A @ m,
                               rtol=0, atol=1e-14)
    np.testing.assert_allclose(kr.gather_ref(d, qs, qr), A.T @ d.ravel(),
                               rtol=0, atol=1e-14)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dot_test(dtype):
    rng = np.random.default_rng(1)
    ns, nr, ni, nt = 3, 2, 40, 33
    qs, qr = tables(rng, ns, nr, ni, nt, dtype)
    m = rng.standard_normal(ni).astype(dtype)
    d = rng.standard_normal((ns, nr, nt)).astype(dtype)
    lhs = np.dot(kr.spread_ref(m, qs, qr, nt).ravel().astype(np.float64),
                 d.ravel().astype(np.float64))
    rhs = np.dot(m.astype(np.float64),
                 kr.gather_ref(d, qs, qr).astype(np.float64))
    assert abs(lhs - rhs) <= 50 * np.finfo(dtype).eps * (abs(lhs) + 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_chunking(dtype):
    rng = np.random.default_rng(2)
    ns, nr, ni, nt = 3, 4, 50, 21
    qs, qr = tables(rng, ns, nr, ni, nt, dtype)
    d = rng.standard_normal((ns, nr, nt)).astype(dtype)
    whole = kr.gather_ref(d, qs, qr)
    for chunk in (12, 13, 1000):
        assert np.array_equal(kr.gather_ref(d, qs, qr, chunk), whole)
    # a real split is the sum of the chunks' own gathers, in order; the
    # traces as 12 sources of one receiver with the rounded sums as table
    qsum = np.repeat(qs, nr, axis=0) + np.tile(qr, (ns, 1))
    zero = np.zeros((1, ni), dtype=dtype)
    flat = d.reshape(12, 1, nt)
    parts = [kr.gather_ref(flat[k0:k0 + 5], qsum[k0:k0 + 5], zero)
             for k0 in (0, 5, 10)]
    want = parts[0] + parts[1] + parts[2]
    assert np.array_equal(kr.gather_ref(flat, qsum, zero, 5), want)
    assert np.array_equal(kr.gather_ref(d, qs, qr, 5), want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_skip_rules(dtype):
    """q = -0.5, nt - 1 exactly, one ulp below nt - 1, an exact integer,
    NaN and +inf, one image point each."""
    nt = 6
    T = dtype
    below = np.nextafter(T(nt - 1), T(0))
    q = np.array([-0.5, nt - 1, below, 2.0, np.nan, np.inf], dtype=dtype)
    qs = (q / 2).reshape(1, -1)             # halves are exact; inf, nan stay
    assert np.array_equal(qs[0] + qs[0], q, equal_nan=True)
    keep, it, w = kr.pairs(qs[0], qs[0], nt)
    assert keep.tolist() == [False, False, True, True, False, False]
    assert it.tolist() == [0, 0, nt - 2, 2, 0, 0]
    assert w[3] == 0 and w[2] == below - T(nt - 2) and 0 < w[2] < 1
    m = np.array([1, 10, 100, 1000, 1e4, 1e5], dtype=dtype)
    d = kr.spread_ref(m, qs, qs, nt)[0, 0]
    want = np.zeros(nt, dtype=dtype)
    want[2] = 1000
    want[nt - 2] = T(100) * (T(1) - w[2])
    want[nt - 1] = T(100) * w[2]
    assert np.array_equal(d, want)
    assert kr.spread_count(qs, qs, nt)[0, 0].tolist() == [0, 0, 1, 1, 1, 1]
    data = np.arange(1, nt + 1, dtype=dtype).reshape(1, 1, nt)
    mig = kr.gather_ref(data, qs, qs)
    assert mig[[0, 1, 4, 5]].tolist() == [0, 0, 0, 0]
    assert mig[3] == 3
    assert mig[2] == (T(1) - w[2]) * T(nt - 1) + w[2] * T(nt)
    # non-finite data next to a skipped pair never reaches the image
    data[0, 0, :2] = np.nan
    assert kr.gather_ref(data, qs, qs)[[0, 1, 4, 5]].tolist() == [0, 0, 0, 0]

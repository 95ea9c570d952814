"""The NumPy reference of pam_conv1d (tests/convref.py) checked on its own,
without a GPU: against the pad-and-convolve "same" recipe pylops'
Convolve1D is built on, against its own transpose, and against explicit
first-derivative matrices."""
import numpy as np
import pytest

import convref as cr

NHS = (1, 2, 3, 4, 7, 8, 41)
DS = (1, 2, 5, 17, 40)


def offsets(nh):
    return sorted({0, nh // 2, nh - 1})


@pytest.mark.parametrize("nh", NHS)
def test_equals_same_recipe(nh):
    """Odd and even nh, offsets {0, nh//2, nh-1}, both directions: the
    closed form is the padded np.convolve / np.correlate "same" result.
    The two sum the same products in a different order, hence a few ulp
    of the largest partial sum instead of equality."""
    rng = np.random.default_rng(nh)
    for d in DS:
        for off in offsets(nh):
            x = rng.standard_normal(d)
            h = rng.standard_normal(nh)
            for adj in (False, True):
                got = cr.conv1d_ref(x.reshape(1, d, 1), h, off, adj).ravel()
                want = cr.same_recipe(x, h, off, adj)
                tol = 4 * np.finfo(np.float64).eps * nh * \
                    np.abs(h).max() * np.abs(x).max()
                np.testing.assert_allclose(got, want, rtol=0, atol=tol)


@pytest.mark.parametrize("deriv", (0, 1, 2))
@pytest.mark.parametrize("nh", (1, 2, 3, 8, 41))
def test_adjoint_is_exact_transpose(nh, deriv):
    """Each matrix entry is one tap, or for deriv a sum of the same
    products in the same order, so the transpose holds exactly — with
    integer taps, whose sums no order can round differently."""
    rng = np.random.default_rng(100 + nh)
    h = rng.integers(-4, 5, nh).astype(np.float64)
    for d in (1, 2, 5, 17):
        for off in offsets(nh):
            F = cr.dense(lambda v: cr.conv1d_ref(v, h, off, False, deriv), d)
            A = cr.dense(lambda v: cr.conv1d_ref(v, h, off, True, deriv), d)
            assert np.array_equal(A, F.T), (d, nh, off, deriv)


@pytest.mark.parametrize("deriv", (1, 2))
def test_deriv_equals_explicit_matrix(deriv):
    """forward = C D and adjoint = D^T C^T with the explicit D of either
    kind; batches and columns do not mix."""
    rng = np.random.default_rng(7 + deriv)
    for d, nh in ((1, 3), (2, 3), (5, 2), (17, 8), (17, 41)):
        h = rng.standard_normal(nh)
        D = cr.fd_matrix(d, deriv)
        for off in offsets(nh):
            C = cr.dense(lambda v: cr.conv_ref(v, h, off, False), d)
            x = rng.standard_normal((2, d, 3))
            fwd = cr.conv1d_ref(x, h, off, False, deriv)
            adj = cr.conv1d_ref(x, h, off, True, deriv)
            want_f = np.einsum("ng,bgj->bnj", C @ D, x)
            want_a = np.einsum("ng,bgj->bnj", D.T @ C.T, x)
            np.testing.assert_allclose(fwd, want_f, rtol=0, atol=1e-13 * nh)
            np.testing.assert_allclose(adj, want_a, rtol=0, atol=1e-13 * nh)
            # the stencil alone is the matrix exactly
            Dm = cr.dense(lambda v: cr.fd_ref(v, deriv, False), d)
            Dt = cr.dense(lambda v: cr.fd_ref(v, deriv, True), d)
            assert np.array_equal(Dm, D) and np.array_equal(Dt, D.T)


def test_dtype_is_kept_and_rounded_per_tap():
    """float32 in, float32 out, each tap rounded on its own."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((1, 9, 2)).astype(np.float32)
    h = rng.standard_normal(4).astype(np.float32)
    got = cr.conv1d_ref(x, h, 1, False)
    assert got.dtype == np.float32
    n, j = 5, 1
    acc = np.float32(0)
    for k in range(4):
        g = n - k + 1
        if 0 <= g < 9:
            acc = np.float32(acc + np.float32(h[k] * x[0, g, j]))
    assert got[0, n, j] == acc

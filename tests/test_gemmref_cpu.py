"""The references, integer data and placement of tests/gemmref.py checked
on their own, without a GPU."""
import numpy as np
import pytest
import torch
from numpy.testing import assert_allclose

import gemmref as gr
import primref as pr

DT = pr.DTYPES


def normals(rng, shape, dt):
    x = rng.standard_normal(shape)
    if pr.is_complex(dt):
        x = x + 1j * rng.standard_normal(shape)
    return x.astype(dt)


@pytest.mark.parametrize("opa", [False, True])
@pytest.mark.parametrize("dname", list(DT))
def test_refs_vs_matmul(dname, opa):
    """Against np.matmul in float64 / complex128 of the stored values, to
    the reference's own bound at u = 2^-53 (float64 matmul is one more
    summation order) — and the float32 bound is 2^29 times that."""
    dt = DT[dname]
    wide = np.complex128 if pr.is_complex(dt) else np.float64
    rng = np.random.default_rng([1, list(DT).index(dname), opa])
    for batch, M, K, N in ((1, 5, 7, 3), (3, 33, 65, 17), (2, 4, 0, 6)):
        A = normals(rng, (batch, K, M) if opa else (batch, M, K), dt)
        B = normals(rng, (batch, K, N), dt)
        C0 = normals(rng, (batch, M, N), dt)
        for c0 in (None, C0):
            ref, bound = gr.bgemm(A, B, c0, opa)
            assert ref.shape == bound.shape == (batch, M, N)
            assert ref.dtype == (np.clongdouble if pr.is_complex(dt)
                                 else np.longdouble)
            want = np.matmul(gr.op(A, opa).astype(wide), B.astype(wide))
            if c0 is not None:
                want = want + c0.astype(wide)
            b64 = bound * (gr.unit(np.float64) / gr.unit(dt))
            assert gr.err_ratio(want, ref, b64) <= 1.0
            assert np.all(bound >= 0)
            if K == 0:
                assert np.all(ref == (0 if c0 is None else c0))
    assert gr.unit(np.float32) == 2.0 ** -24
    assert gr.unit(np.complex64) == 2.0 ** -24
    assert gr.unit(np.float64) == gr.unit(np.complex128) == 2.0 ** -53


def test_gemm_is_the_unbatched_bgemm_and_broadcasts():
    rng = np.random.default_rng(2)
    A, B = normals(rng, (6, 4), np.float64), normals(rng, (3, 4, 5),
                                                     np.float64)
    ref, bound = gr.gemm(A, B[0])
    assert_allclose(ref.astype(np.float64), A @ B[0], rtol=0, atol=1e-14)
    refb, _ = gr.bgemm(A, B)            # one A for every batch
    assert refb.shape == (3, 6, 5)
    assert np.array_equal(refb[0], ref)
    assert_allclose(refb[2].astype(np.float64), A @ B[2], rtol=0,
                    atol=1e-14)


def test_err_ratio():
    ref = np.array([1.0, 2.0], dtype=np.longdouble)
    bound = np.array([0.5, 0.0], dtype=np.longdouble)
    assert gr.err_ratio(np.array([1.25, 2.0]), ref, bound) == 0.5
    assert gr.err_ratio(np.array([1.0, 2.5]), ref, bound) == np.inf
    assert np.isnan(gr.err_ratio(np.array([np.nan, 2.0]), ref, bound))
    cref = np.array([1 + 1j], dtype=np.clongdouble)
    assert gr.err_ratio(np.array([1 + 3j]), cref, bound[:1]) == 4.0


def all_shapes():
    """Every (batch, M, K, N) the GPU suite runs."""
    return ([(1,) + s for s in gr.GEMM_SHAPES + gr.KT_SHAPES]
            + gr.BATCHED_SHAPES + gr.VARIANT_SHAPES)


@pytest.mark.parametrize("dname", list(DT))
def test_integer_data_stay_exact(dname):
    """Parts in [-4, 4]; every result and every sum of magnitudes below
    2^24 (int_gemm asserts the latter) for every shape of the GPU suite."""
    dt = DT[dname]
    shapes = all_shapes()
    assert len(shapes) > 40
    for i, (batch, M, K, N) in enumerate(shapes):
        assert max(M, K, N) <= 520
        rng = np.random.default_rng([3, i])
        for opa in (False, True):
            A = gr.int_operand(rng, (batch, K, M) if opa else (batch, M, K),
                               dt)
            B = gr.int_operand(rng, (batch, K, N), dt)
            C0 = gr.int_operand(rng, (batch, M, N), dt)
            assert A.dtype == dt
            want = gr.int_gemm(A, B, C0, opa)
            assert want.dtype == dt and want.shape == (batch, M, N)
            assert np.max(np.abs(pr.rview(want.reshape(-1))),
                          initial=0) < gr.INT_LIMIT
            if i % 7 == 0:
                ref, _ = gr.bgemm(A, B, C0, opa)
                assert np.array_equal(ref, want.astype(ref.dtype))
    with pytest.raises(AssertionError):     # not integers
        gr.int_gemm(np.full((2, 2), 0.5, dt), np.ones((2, 2), dt))
    with pytest.raises(AssertionError):     # partial sums past 2^24
        gr.int_gemm(np.full((1, 2 ** 12), 2.0 ** 6, dt),
                    np.full((2 ** 12, 1), 2.0 ** 6, dt))


@pytest.mark.parametrize("dname", list(DT))
def test_trends_tell_reads_apart(dname):
    """A @ B, A^T @ B, A^H @ B and a one-column shift of either operand
    differ pairwise, in most entries."""
    dt = DT[dname]
    rng = np.random.default_rng(4)
    n = 33
    A, B = gr.int_operand(rng, (n, n), dt), gr.int_operand(rng, (n, n), dt)
    forms = {"AB": gr.int_gemm(A, B),
             "AtB": gr.int_gemm(np.ascontiguousarray(A.T), B),
             "ABt": gr.int_gemm(A, np.ascontiguousarray(B.T)),
             "shiftA": gr.int_gemm(np.roll(A, 1, axis=1), B),
             "shiftB": gr.int_gemm(A, np.roll(B, 1, axis=1)),
             "rowA": gr.int_gemm(np.roll(A, 1, axis=0), B)}
    if pr.is_complex(dt):
        forms["AhB"] = gr.int_gemm(A, B, opa=True)
        forms["conjA"] = gr.int_gemm(np.conj(A), B)
    names = list(forms)
    for i, p in enumerate(names):
        for q in names[i + 1:]:
            assert np.mean(forms[p] != forms[q]) > 0.5, (p, q)
    # the trends alone (no random part) already do it for the transpose
    t = gr._trend((n, n)).astype(np.int64)
    assert np.mean(t @ t != t.T @ t) > 0.5


@pytest.mark.parametrize("dname", list(DT))
def test_placement_on_host(dname):
    """Placed2D on the CPU device: index round trip, padding, guards."""
    dt = DT[dname]
    rng = np.random.default_rng(5)
    w = 2 if pr.is_complex(dt) else 1
    for shape, ld, bs in (((3, 5), None, None), ((3, 5), 8, None),
                          ((2, 3, 5), 6, 23), ((2, 3, 5), None, None),
                          ((1, 1), 4, None), ((4, 0), 3, None),
                          ((4, 0), None, None), ((1, 257), 258, None)):
        x = normals(rng, shape, dt)
        for off in (0, 1):
            for fill in (pr.SENTINEL, np.nan):
                p = gr.Placed2D(x, ld, bs, off, fill, device="cpu")
                rows, cols = shape[-2:]
                assert p.ld == (ld or cols) and p.bstride == (bs or
                                                              rows * p.ld)
                assert p.ptr % 16 == (0 if off == 0 else
                                      4 if dname == "f32" else 8)
                assert p.untouched() and p.guards_intact()
                assert pr.same(p.value(), x) and p.value().shape == shape
                assert p.mask.sum() == x.size * w
                outside = p.image[~p.mask]
                assert outside.size >= 2 * pr.GUARD
                assert (np.all(np.isnan(outside)) if fill != fill
                        else np.all(outside == fill))
                if not x.size:
                    continue
                # element (b, r, c) sits where the C-ABI looks for it
                b = (shape[0] if len(shape) == 3 else 1) - 1
                r, c = rows - 1, cols - 1
                at = p.lo + (b * p.bstride + r * p.ld + c) * w
                assert p.image[at] == pr.rview(x.reshape(-1))[-w]
                assert at + w == p.hi
                p.buf[p.index[0]] = 3.0     # a write to the operand
                assert p.guards_intact() and not p.untouched()
                assert pr.rview(p.value().reshape(-1))[0] == 3.0
                for spot in (p.lo - 1, p.hi):       # just outside
                    q = gr.Placed2D(x, ld, bs, off, fill, device="cpu")
                    q.buf[spot] = 1.0
                    assert not q.guards_intact()
                if p.ld > cols and rows > 1:        # a padding column
                    q = gr.Placed2D(x, ld, bs, off, fill, device="cpu")
                    q.buf[q.lo + cols * w] = 1.0
                    assert not q.guards_intact()
                if len(shape) == 3 and p.bstride > rows * p.ld:
                    q = gr.Placed2D(x, ld, bs, off, fill, device="cpu")
                    q.buf[q.lo + (p.bstride - 1) * w] = 1.0     # the gap
                    assert not q.guards_intact()
    assert torch.tensor(pr.SENTINEL, dtype=torch.float32).item() \
        == pr.SENTINEL

"""tests/stencilref.py checked on a CPU: the bit-exact restatement
(fd_rows, nsconv_ref) against the dense definitions (fd_dense,
nsconv_dense) and against the oracle, the transpose structure of the ops,
and the rank cuts.

Tolerance of fd_rows against fd_dense @ x, in units of u = eps / 2.  An
output is a sum of k products T(c_t) * x_t scaled by T(coeff).  Each product
carries the rounding of its coefficient and its own (2 u) and passes through
at most k sums (k u); the scaling adds the rounding of coeff and of the last
product (2 u): to first order (k + 4) u sum_t |c_t x_t| |coeff|.  k is at
most NT, the op's term count, except for op 13 with edge, whose fix-ups add
x[0] to row 2 and x[N-1] to row N-3 on top of all three terms: NT + 1 = 4
samples from N = 4 on and NT + 2 = 5 at N = 5, where both land on row 2.
The fix-ups of the matvec ops replace the terms, the other additive ones
fall on rows where as many terms are masked out.  Since k + 4 <= 4 NT + 4
either way, the error is within (2 NT + 2) eps |coeff| sum_t |c_t x_t| —
the bound asserted, with eps of the array's type and
sum_t |c_t x_t| = |D| |x| (no row of any op holds two contributions of
opposite sign to one entry)."""
import numpy as np
import pytest
from numpy.testing import assert_allclose

import oracle
import stencilref as sr

LD = np.longdouble
KINDS = {0: ("forward", 3), 2: ("backward", 3), 4: ("centered", 3),
         6: ("centered", 5)}
KINDS2 = {8: "forward", 10: "backward", 12: "centered"}
SAMPLING = 1.5
NS = range(1, 10)


def coeff_of(op):
    return 1.0 / SAMPLING if op < 8 else 1.0 / SAMPLING ** 2


def defined(op, edge):
    return [N for N in NS if N >= sr.fd_min_rows(op, edge)]


def data(N, m, dtype, seed=0):
    return np.random.default_rng(seed + 131 * N + m).standard_normal(
        (N, m)).astype(dtype)


def test_min_rows_table():
    for op in sr.OPS:
        assert sr.fd_min_rows(op, False) == 1
        assert sr.fd_min_rows(op, True) == (
            2 if op in (4, 5) else 3 if op in (6, 7, 12, 13) else 1)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("op", sr.OPS)
def test_fd_rows_against_dense(op, edge, dtype):
    eps = float(np.finfo(dtype).eps)
    n = len(sr.TERMS[op])                       # NT
    for N in defined(op, edge):
        x = data(N, 5, dtype)
        c = 0.75
        D = sr.fd_dense(op, edge, N)
        assert np.count_nonzero(D, axis=1).max() <= n + 2 * (op == 13 and edge)
        want = LD(c) * (D @ x.astype(LD))
        bound = (2 * n + 2) * eps * abs(c) * (np.abs(D) @ np.abs(x.astype(LD)))
        got = sr.fd_rows(x, op, edge, c, 0, N)
        assert got.dtype == dtype and got.shape == x.shape
        err = np.abs(got.astype(LD) - want)
        assert np.all(err <= bound), (op, edge, N, float(np.max(err - bound)))
        # below the minimum the reference refuses, as the library does
    for N in range(1, sr.fd_min_rows(op, edge)):
        with pytest.raises(IndexError):
            sr.fd_rows(data(N, 2, dtype), op, edge, 1.0, 0, N)
        with pytest.raises(IndexError):
            sr.fd_dense(op, edge, N)


@pytest.mark.parametrize("edge", [False, True])
def test_odd_ops_are_transposes_with_one_exception(edge):
    for op, even in sr.PARTNER.items():
        for N in defined(op, edge):
            R, M = sr.fd_dense(op, edge, N), sr.fd_dense(even, edge, N)
            if (op, edge, N) == (7, True, 3):
                diff = np.argwhere(R != M.T).tolist()
                assert diff == [[0, 1], [2, 1]]
                assert R[0, 1] == -1 and M.T[0, 1] == -0.5
                assert R[2, 1] == 1 and M.T[2, 1] == 0.5
            else:
                assert np.array_equal(R, M.T), (op, edge, N)


@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("op", [1, 3, 5, 7, 9, 11, 13])
def test_rmatvec_arithmetic_is_the_stated_matrix(op, edge):
    """fd_rows of an odd op on the identity gives fd_dense exactly where
    the coefficients are exact (all but 1/12 and 2/3), and to one rounding
    otherwise — the N = 3 exception included, so the exception is what the
    arithmetic does and not an artefact of the dense table."""
    for N in defined(op, edge):
        got = sr.fd_rows(np.eye(N), op, edge, 1.0, 0, N).astype(LD)
        D = sr.fd_dense(op, edge, N)
        assert np.all(np.abs(got - D) <= np.finfo(np.float64).eps * np.abs(D))
        assert np.array_equal(got != 0, D != 0)


@pytest.mark.parametrize("edge", [False, True])
def test_against_serial_oracle(edge):
    """The matvec ops against oracle.serial_fd1_matvec / serial_fd2_matvec
    wherever those are defined — which must be exactly where fd_min_rows
    says."""
    ran = 0
    for op in (0, 2, 4, 6, 8, 10, 12):
        for N in NS:
            x = data(N, 4, np.float64)
            try:
                if op < 8:
                    kind, order = KINDS[op]
                    want = oracle.serial_fd1_matvec(x, SAMPLING, kind, edge,
                                                    order)
                else:
                    want = oracle.serial_fd2_matvec(x, SAMPLING, KINDS2[op],
                                                    edge)
            except IndexError:
                assert N < sr.fd_min_rows(op, edge), (op, edge, N)
                continue
            assert N >= sr.fd_min_rows(op, edge), (op, edge, N)
            got = sr.fd_rows(x, op, edge, coeff_of(op), 0, N)
            assert_allclose(got, want, rtol=1e-12, atol=1e-13)
            ran += 1
    assert ran >= 7 * 7


def _sim(op, dims, edge):
    even = op - op % 2
    if op < 8:
        kind, order = KINDS[even]
        return oracle.SimFirstDerivative(dims, SAMPLING, kind, edge, order)
    return oracle.SimSecondDerivative(dims, SAMPLING, KINDS2[even], edge)


# Where the rank simulation itself refuses a shape.  On one rank: only the
# 5-point operators without edge at N = 1 (both) and N = 2 (rmatvec), whose
# zero padding gets a negative length.  On several ranks the smallest block
# holds N // P rows, and the slice algebra raises when that is fewer than
# the ghost rows an rmatvec asks of a neighbour (2 w: ops 5 and 7) or than
# the rows the edge formulas name on the first / last rank alone.
SIM_P1_REFUSES = {(6, 1), (7, 1), (7, 2)}


def sim_rows_needed(op, edge):
    need = 2 * sr.HALO[op] if op in (5, 7) else sr.HALO[op]
    return max(need, sr.fd_min_rows(op, edge))


@pytest.mark.parametrize("P", [1, 2, 3])
@pytest.mark.parametrize("edge", [False, True])
def test_against_rank_simulated_oracle(P, edge):
    """All 14 ops against oracle.SimFirstDerivative / SimSecondDerivative
    (matvec and rmatvec) on P simulated ranks, at every accepted N <= 9
    but the shapes listed above, which the simulation must refuse — no
    other shape may drop out.  On several ranks every rank must hold the
    op's halo width of rows (what MPIFirstDerivative itself demands; with
    fewer the slice algebra takes rows from the wrong rank without
    noticing), so those shapes are not compared."""
    for op in sr.OPS:
        for N in defined(op, edge):
            if P > 1 and N // P < sr.HALO[op]:
                continue
            refuses = (op, N) in SIM_P1_REFUSES if P == 1 else \
                N // P < sim_rows_needed(op, edge)
            x = data(N, 3, np.float64, seed=5)
            sim = _sim(op, (N, 3), edge)
            fn = sim.rmatvec if op % 2 else sim.matvec
            if refuses:
                with pytest.raises((ValueError, IndexError)):
                    fn(oracle.to_dist(x.ravel(), P))
                continue
            want = fn(oracle.to_dist(x.ravel(), P)).asarray()
            got = sr.fd_rows(x, op, edge, coeff_of(op), 0, N)
            assert_allclose(got.ravel(), want, rtol=1e-12, atol=1e-13)


def test_n3_exception_is_the_oracles():
    """centered5 with edge at N = 3: the rank-simulated reference algebra
    gives OP7_EDGE_N3, not the transpose of its own matvec."""
    sim = oracle.SimFirstDerivative((3,), 1.0, "centered", True, 5)

    def mat(fn):
        return np.stack([fn(oracle.to_dist(np.eye(3)[:, j].copy(), 1))
                         .asarray() for j in range(3)], axis=1)

    R, M = mat(sim.rmatvec), mat(sim.matvec)
    assert np.array_equal(R, sr.OP7_EDGE_N3.astype(np.float64))
    assert np.array_equal(M, sr.fd_dense(6, True, 3).astype(np.float64))
    assert not np.array_equal(R, M.T)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("op", sr.OPS)
def test_rank_cuts_reproduce_the_whole_array(op, edge, dtype):
    """The global array cut into P blocks, each evaluated from its own rows
    and its neighbours' planes, concatenates to the whole-array result bit
    for bit; so does the overlap split [w, nloc-w) without planes plus the
    two boundary ranges with them."""
    w = sr.HALO[op]
    N = 4 * w + 5
    x = data(N, 3, dtype, seed=9)
    whole = sr.fd_rows(x, op, edge, 0.75, 0, N)
    cuts = [[w, N - w], [N - w, w], [2 * w + 1, N - 2 * w - 1],
            [w, 2 * w + 1, N - 3 * w - 1], [2 * w + 1, w, N - 3 * w - 1],
            [N - 3 * w - 1, 2 * w + 1, w]]
    for sizes in cuts:
        assert sum(sizes) == N and min(sizes) >= w
        outs, s = [], 0
        for r, nloc in enumerate(sizes):
            gf = x[s - w:s] if r > 0 else None
            gb = x[s + nloc:s + nloc + w] if r < len(sizes) - 1 else None
            assert gb is None or gb.shape[0] == w
            y = sr.fd_rows(x[s:s + nloc], op, edge, 0.75, s, N, gf, gb)
            if nloc > 2 * w:
                parts = [sr.fd_rows(x[s:s + nloc], op, edge, 0.75, s, N,
                                    gf, gb, 0, w),
                         sr.fd_rows(x[s:s + nloc], op, edge, 0.75, s, N,
                                    None, None, w, nloc - w),
                         sr.fd_rows(x[s:s + nloc], op, edge, 0.75, s, N,
                                    gf, gb, nloc - w, nloc)]
                assert np.array_equal(np.concatenate(parts), y)
            outs.append(y)
            s += nloc
        assert np.array_equal(np.concatenate(outs), whole), (op, sizes)


def test_fd_serial_ref_is_fd_rows_per_batch():
    x = np.random.default_rng(3).standard_normal((3, 7, 4))
    for op in sr.OPS:
        y = sr.fd_serial_ref(x, op, True, 0.5)
        for b in range(3):
            assert np.array_equal(y[b], sr.fd_rows(x[b], op, True, 0.5, 0, 7))


# ------------------------------------------------------------------ nsconv
def _nsc_case(dtype, nf, hsize, seed=0):
    rng = np.random.default_rng(seed)
    hs = rng.standard_normal((nf, hsize)).astype(dtype)
    return hs, 3.0, 5.5        # anchors at 3, 8.5, 14, ...: 3 and 14 on samples


def _dense_of(fn, d, dtype):
    return np.stack([fn(np.eye(d, dtype=dtype)[:, j].reshape(1, d, 1)).ravel()
                     for j in range(d)], axis=1)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nf", [1, 2, 4])
@pytest.mark.parametrize("hsize", [1, 3, 7])
def test_nsconv_adjoint_is_the_transpose_bit_for_bit(dtype, nf, hsize):
    hs, oh, dh = _nsc_case(dtype, nf, hsize)
    for d in (1, 2, max(hsize - 1, 1), 24):
        F = _dense_of(lambda v: sr.nsconv_ref(v, hs, oh, dh, True), d, dtype)
        A = _dense_of(lambda v: sr.nsconv_ref(v, hs, oh, dh, False), d, dtype)
        assert np.array_equal(F.T, A)
        FD = sr.nsconv_dense(hs, d, oh, dh, True)
        assert np.array_equal(FD.T, sr.nsconv_dense(hs, d, oh, dh, False))
        # an interpolated tap is two rounded products and a rounded sum
        eps = float(np.finfo(dtype).eps)
        amax = np.abs(hs.astype(LD)).max()
        assert np.all(np.abs(F.astype(LD) - FD) <= 3 * eps * amax)
        # clamped and on-anchor taps are the stored filters themselves
        hh = hsize // 2
        for ix in (0, 3):
            if ix < d:
                assert F[ix, ix] == hs[0][hh]


@pytest.mark.parametrize("nf", [2, 4])
def test_nsconv_against_oracle(nf):
    hs, oh, dh = _nsc_case(np.float64, nf, 7)
    ih = oh + dh * np.arange(nf)
    rng = np.random.default_rng(4)
    for dims in ((1, 24, 1), (2, 24, 3), (3, 6, 1)):
        x = rng.standard_normal(dims)
        xt = np.ascontiguousarray(np.moveaxis(x, 1, -1))   # oracle: last axis
        tdims = xt.shape
        for forward, fn in ((True, oracle.serial_nsconv_mv),
                            (False, oracle.serial_nsconv_rmv)):
            want = np.moveaxis(fn(xt.ravel(), tdims, hs, ih).reshape(tdims),
                               -1, 1)
            got = sr.nsconv_ref(x, hs, oh, dh, forward)
            assert_allclose(got, want, rtol=1e-12, atol=1e-13)

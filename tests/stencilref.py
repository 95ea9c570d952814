"""NumPy references of the finite-difference stencils (pam_fd_apply,
pam_fd_serial) and of pam_nsconv (include/pam.h) for the kernel tests of
tests/test_gpu_stencil.py; checked on their own, on a CPU, by
tests/test_stencilref_cpu.py.  No GPU, no torch.

Two independent statements of every stencil:

``fd_dense`` is the DEFINITION, an N x N np.longdouble matrix.  The matvec
ops (even codes) are written row by row from the published formulas, with
sampling 1:
  forward    y[g] = x[g+1] - x[g]                              g <= N-2
  backward   y[g] = x[g] - x[g-1]                              g >= 1
  centered3  y[g] = (x[g+1] - x[g-1]) / 2                      1 <= g <= N-2
  centered5  y[g] = x[g-2]/12 - 2 x[g-1]/3 + 2 x[g+1]/3 - x[g+2]/12
                                                               2 <= g <= N-3
  second derivative forward / backward / centered:
             x[g+2] - 2 x[g+1] + x[g] (g <= N-3), x[g] - 2 x[g-1] + x[g-2]
             (g >= 2), x[g+1] - 2 x[g] + x[g-1] (1 <= g <= N-2)
every other row is zero, and with edge
  centered3  y[0] = x[1] - x[0], y[N-1] = x[N-1] - x[N-2]
  centered5  the same two rows, y[1] = (x[2] - x[0]) / 2 and
             y[N-2] = (x[N-1] - x[N-3]) / 2
  second centered  y[0] = x[0] - 2 x[1] + x[2],
             y[N-1] = x[N-3] - 2 x[N-2] + x[N-1]
(forward and backward have no edge rows).  An rmatvec op (odd code) is the
transpose of its partner, with ONE exception, stated explicitly in
``OP7_EDGE_N3``: centered5 with edge at N = 3.  There the matvec writes
row 1 twice (y[1] and y[-2] are the same row, both (x[2] - x[0]) / 2) while
the rmatvec adds the fix-ups of both ends, so x[1] is counted twice.  The
reference's slice algebra does exactly that; the kernels keep it.

``fd_rows`` is the ARITHMETIC the kernels promise (include/pam.h): per
output acc = 0, then for every term (offset, coefficient, lo, hi) of the op,
in the op's order, active iff lo <= g <= N-1-hi: acc += T(c) * x[g+off] with
the product rounded and then the sum, c rounded from float64 to T once; then
the edge fix-up of the row, operation by operation as listed in ``_edge``;
last acc *= T(coeff).  The library is built without contraction, so NumPy
in the array's own dtype gives the same bits.  The terms are the formulas
above read off per output row (matvec) or per input column (rmatvec: entry
[g, g+off] of the transpose is entry [g+off, g] of the matvec, active where
row g+off is); their ORDER is the one thing fixed by the library and not by
the mathematics, and for the ops of three and four terms it is part of what
the bit-for-bit tests pin.

``nsconv_ref`` / ``nsconv_dense`` do the same for pam_nsconv."""
import numpy as np

LD = np.longdouble
OPS = tuple(range(14))
PARTNER = {1: 0, 3: 2, 5: 4, 7: 6, 9: 8, 11: 10, 13: 12}
HALO = {op: (1 if op < 6 else 2) for op in OPS}    # pam_fd_halo_width
_EDGE_MIN = {4: 2, 5: 2, 6: 3, 7: 3, 12: 3, 13: 3}


def fd_min_rows(op, edge):
    """Shortest axis on which the op is defined: the edge rows of the
    centered ops name x[1] / x[N-2] (3-point) or x[2] / x[N-3] (5-point and
    second derivative), which must exist."""
    return _EDGE_MIN.get(op, 1) if edge else 1


# ------------------------------------------------------------- definition
# matvec ops: (row range as (lo, hi): rows lo .. N-1-hi, {offset: coeff})
_L = LD(1)
_STENCIL = {
    0: ((0, 1), {0: -_L, 1: _L}),
    2: ((1, 0), {0: _L, -1: -_L}),
    4: ((1, 1), {1: _L / 2, -1: -_L / 2}),
    6: ((2, 2), {-2: _L / 12, -1: -2 * _L / 3, 1: 2 * _L / 3, 2: -_L / 12}),
    8: ((0, 2), {0: _L, 1: -2 * _L, 2: _L}),
    10: ((2, 0), {0: _L, -1: -2 * _L, -2: _L}),
    12: ((1, 1), {-1: _L, 0: -2 * _L, 1: _L}),
}
# centered5 rmatvec with edge at N = 3: NOT the transpose of the matvec,
# which is [[-1, 1, 0], [-.5, 0, .5], [0, -1, 1]]
OP7_EDGE_N3 = np.array([[-1, -1, 0], [1, 0, -1], [0, 1, 1]], dtype=LD)


def _set_row(D, g, entries):
    D[g, :] = 0
    for col, v in entries.items():
        if not 0 <= col < D.shape[0]:
            raise IndexError(f"row {g} names x[{col}] of {D.shape[0]}")
        D[g, col] = v


def fd_dense(op, edge, N):
    """The N x N matrix of the op in np.longdouble, sampling 1."""
    if N < fd_min_rows(op, edge):
        raise IndexError(f"op {op} with edge is not defined for N = {N}")
    if op in PARTNER:
        if op == 7 and edge and N == 3:
            return OP7_EDGE_N3.copy()
        return fd_dense(PARTNER[op], edge, N).T.copy()
    (lo, hi), sten = _STENCIL[op]
    D = np.zeros((N, N), dtype=LD)
    for g in range(lo, N - hi):
        _set_row(D, g, {g + off: v for off, v in sten.items()})
    if edge and op in (4, 6):
        _set_row(D, 0, {1: _L, 0: -_L})
        if op == 6:
            _set_row(D, 1, {2: _L / 2, 0: -_L / 2})
        _set_row(D, N - 1, {N - 1: _L, N - 2: -_L})
        if op == 6:
            _set_row(D, N - 2, {N - 1: _L / 2, N - 3: -_L / 2})
    if edge and op == 12:
        _set_row(D, 0, {0: _L, 1: -2 * _L, 2: _L})
        _set_row(D, N - 1, {N - 3: _L, N - 2: -2 * _L, N - 1: _L})
    return D


# -------------------------------------------------------------- arithmetic
# (offset, coefficient in float64, lo, hi) in the library's order
TERMS = {
    0: ((1, 1.0, 0, 1), (0, -1.0, 0, 1)),
    1: ((0, -1.0, 0, 1), (-1, 1.0, 1, 0)),
    2: ((0, 1.0, 1, 0), (-1, -1.0, 1, 0)),
    3: ((1, -1.0, 0, 1), (0, 1.0, 1, 0)),
    4: ((1, 0.5, 1, 1), (-1, -0.5, 1, 1)),
    5: ((1, -0.5, 0, 2), (-1, 0.5, 2, 0)),
    6: ((-2, 1.0 / 12, 2, 2), (-1, -2.0 / 3, 2, 2), (1, 2.0 / 3, 2, 2),
        (2, -1.0 / 12, 2, 2)),
    7: ((2, 1.0 / 12, 0, 4), (1, -2.0 / 3, 1, 3), (-1, 2.0 / 3, 3, 1),
        (-2, -1.0 / 12, 4, 0)),
    8: ((2, 1.0, 0, 2), (1, -2.0, 0, 2), (0, 1.0, 0, 2)),
    9: ((0, 1.0, 0, 2), (-1, -2.0, 1, 1), (-2, 1.0, 2, 0)),
    10: ((0, 1.0, 2, 0), (-1, -2.0, 2, 0), (-2, 1.0, 2, 0)),
    11: ((2, 1.0, 0, 2), (1, -2.0, 1, 1), (0, 1.0, 2, 0)),
    12: ((1, 1.0, 1, 1), (0, -2.0, 1, 1), (-1, 1.0, 1, 1)),
    13: ((1, 1.0, 0, 2), (0, -2.0, 1, 1), (-1, 1.0, 2, 0)),
}


def _edge(op, g, N, X, acc, T):
    """The edge fix-up of global row g; X(off) is row g + off.  The matvec
    ops overwrite acc, the rmatvec ops add to it: first the fix-up that
    belongs to the head of the axis, then the one of the tail (a short axis
    gets both)."""
    h, two = T(0.5), T(2)
    if op == 4:
        if g == 0:
            return X(1) - X(0)
        if g == N - 1:
            return X(0) - X(-1)
    elif op == 5:
        if g == 0:
            acc = acc - X(0)
        elif g == 1:
            acc = acc + X(-1)
        if g == N - 2:
            acc = acc - X(1)
        elif g == N - 1:
            acc = acc + X(0)
    elif op == 6:
        if g == 0:
            return X(1) - X(0)
        if g == N - 1:
            return X(0) - X(-1)
        if g == 1 or g == N - 2:
            return h * (X(1) - X(-1))
    elif op == 7:
        if g == 0:
            acc = acc - (X(0) + h * X(1))
        elif g == 1:
            acc = acc + X(-1)
        elif g == 2:
            acc = acc + h * X(-1)
        if g == N - 3:
            acc = acc - h * X(1)
        elif g == N - 2:
            acc = acc - X(1)
        elif g == N - 1:
            acc = acc + (h * X(-1) + X(0))
    elif op == 12:
        if g == 0:
            return (X(0) - two * X(1)) + X(2)
        if g == N - 1:
            return (X(-2) - two * X(-1)) + X(0)
    elif op == 13:
        if g == 0:
            acc = acc + X(0)
        elif g == 1:
            acc = acc - two * X(-1)
        elif g == 2:
            acc = acc + X(-2)
        if g == N - 3:
            acc = acc + X(2)
        elif g == N - 2:
            acc = acc - two * X(1)
        elif g == N - 1:
            acc = acc + X(0)
    return acc


def fd_rows(x, op, edge, coeff, row0, nglob, gf=None, gb=None, rbegin=0,
            rend=None):
    """Rows [rbegin, rend) of pam_fd_apply on the [nloc, m] block ``x``
    whose first row is global row ``row0`` of ``nglob``; gf / gb are the
    [w, m] planes before and after the block.  A row that no operand holds
    raises IndexError."""
    x = np.asarray(x)
    assert x.ndim == 2 and x.dtype in (np.float32, np.float64)
    T = x.dtype.type
    nloc, m = x.shape
    N = int(nglob)
    rend = nloc if rend is None else rend
    if N < fd_min_rows(op, edge):
        raise IndexError(f"op {op} with edge is not defined for N = {N}")
    w = HALO[op]

    def row(i):
        if 0 <= i < nloc:
            return x[i]
        src, k = (gf, i + w) if i < 0 else (gb, i - nloc)
        if src is None or not 0 <= k < w:
            raise IndexError(f"local row {i} of a {nloc}-row block")
        return src[k]

    out = np.empty((rend - rbegin, m), dtype=x.dtype)
    c = T(coeff)
    with np.errstate(all="ignore"):
        for i in range(rbegin, rend):
            g = row0 + i
            acc = np.zeros(m, dtype=x.dtype)
            for off, ct, lo, hi in TERMS[op]:
                if lo <= g <= N - 1 - hi:
                    acc = acc + T(ct) * row(i + off)
            if edge:
                acc = _edge(op, g, N, lambda off: row(i + off), acc, T)
            out[i - rbegin] = acc * c
    return out


def fd_serial_ref(x, op, edge, coeff):
    """pam_fd_serial on [batch, d, m]: the stencil along axis 1, per batch
    and column."""
    x = np.asarray(x)
    batch, d, m = x.shape
    flat = np.ascontiguousarray(x.transpose(1, 0, 2)).reshape(d, batch * m)
    y = fd_rows(flat, op, edge, coeff, 0, d)
    return np.ascontiguousarray(y.reshape(d, batch, m).transpose(1, 0, 2))


# ------------------------------------------------------------------ nsconv
def _tap(hs, ix, oh, dh, exact):
    """The hsize taps of the filter at sample ix: clamped to the first /
    last anchor filter outside the anchors, linearly interpolated between
    two anchors inside; the position in float64."""
    nf = hs.shape[0]
    q = (np.float64(ix) - np.float64(oh)) / np.float64(dh)
    ic = int(np.floor(q))
    if ic < 0:
        return hs[0].astype(LD) if exact else hs[0]
    if ic >= nf - 1:
        return hs[nf - 1].astype(LD) if exact else hs[nf - 1]
    if exact:
        w = LD(q - ic)
        return (1 - w) * hs[ic].astype(LD) + w * hs[ic + 1].astype(LD)
    T = hs.dtype.type
    w = T(q - np.float64(ic))
    return (T(1) - w) * hs[ic] + w * hs[ic + 1]


def nsconv_ref(x, hs, oh, dh, forward):
    """pam_nsconv on [batch, d, m] in the array's dtype T, hh = hsize // 2:
      forward  y[n] = sum_t x[n + hh - t] * h_{n + hh - t}[t]
      adjoint  y[n] = sum_t x[n - hh + t] * h_n[t]
    acc = 0, t ascending, acc += x * h with the product rounded and then
    the sum; samples outside [0, d) are skipped."""
    x, hs = np.asarray(x), np.asarray(hs)
    assert x.ndim == 3 and hs.ndim == 2 and x.dtype == hs.dtype
    d = x.shape[1]
    hsize = hs.shape[1]
    hh = hsize // 2
    with np.errstate(all="ignore"):
        taps = [_tap(hs, ix, oh, dh, False) for ix in range(d)]
        y = np.zeros_like(x)
        for n in range(d):
            acc = np.zeros_like(x[:, 0, :])
            for t in range(hsize):
                ix = n + hh - t if forward else n - hh + t
                if 0 <= ix < d:
                    acc = acc + x[:, ix, :] * taps[ix if forward else n][t]
            y[:, n, :] = acc
    return y


def nsconv_dense(hs, d, oh, dh, forward):
    """The d x d matrix of pam_nsconv along the axis in np.longdouble, from
    the definition: forward [n, ix] = h_ix[n - ix + hh], adjoint
    [n, ix] = h_n[ix - n + hh], where the tap exists.  The interpolation
    weight is the exact q - floor(q) of the float64 position."""
    hs = np.asarray(hs)
    hsize = hs.shape[1]
    hh = hsize // 2
    A = np.zeros((d, d), dtype=LD)
    for n in range(d):
        for ix in range(d):
            t = n - ix + hh if forward else ix - n + hh
            if 0 <= t < hsize:
                A[n, ix] = _tap(hs, ix if forward else n, oh, dh, True)[t]
    return A

"""NumPy reference of pam_conv1d (include/pam.h) for the kernel tests of
tests/test_gpu_conv.py; checked on its own, on a CPU, by
tests/test_convref_cpu.py.

``conv1d_ref`` restates the entry point on a [batch, d, m] array in the
array's own dtype: acc = 0, taps in ascending k, one rounded multiply and
one rounded add per tap, terms whose sample leaves [0, d) skipped — so the
kernels can be compared bit for bit.  The derivative stages restate
pam_fd_serial with edge = 0 and coeff = 1: the terms of csrc/fd_defs.h
(ops 4/5 centered, 0/1 forward) in their order."""
import numpy as np

# (row offset, coefficient, lo, hi): active iff lo <= g <= d - 1 - hi
FD_TERMS = {
    (1, False): ((1, 0.5, 1, 1), (-1, -0.5, 1, 1)),      # op 4
    (1, True): ((1, -0.5, 0, 2), (-1, 0.5, 2, 0)),       # op 5
    (2, False): ((1, 1.0, 0, 1), (0, -1.0, 0, 1)),       # op 0
    (2, True): ((0, -1.0, 0, 1), (-1, 1.0, 1, 0)),       # op 1
}
FD_OP = {(1, False): 4, (1, True): 5, (2, False): 0, (2, True): 1}


def _shifted_add(acc, coef, x, shift, lo, hi):
    """acc[:, g] += coef * x[:, g + shift] for g in [lo, hi) where the
    sample exists; the product is rounded, then the sum."""
    d = x.shape[1]
    lo, hi = max(lo, -shift, 0), min(hi, d - shift, d)
    if lo < hi:
        with np.errstate(all="ignore"):
            acc[:, lo:hi] += coef * x[:, lo + shift:hi + shift]


def fd_ref(x, deriv, adjoint):
    """pam_fd_serial(op, edge=0, coeff=1) along axis 1 of [batch, d, m]."""
    T = x.dtype.type
    d = x.shape[1]
    acc = np.zeros_like(x)
    for off, coef, lo, hi in FD_TERMS[(deriv, bool(adjoint))]:
        _shifted_add(acc, T(coef), x, off, lo, d - hi)
    return acc * T(1)


def conv_ref(x, h, offset, adjoint):
    """The taps alone (deriv = 0)."""
    assert x.ndim == 3 and h.ndim == 1 and h.dtype == x.dtype
    assert 0 <= offset < h.size
    acc = np.zeros_like(x)
    for k in range(h.size):
        _shifted_add(acc, h[k], x, (k - offset) if adjoint else (offset - k),
                     0, x.shape[1])
    return acc


def conv1d_ref(x, h, offset, adjoint, deriv=0):
    """pam_conv1d: forward C(Dx), adjoint D^T(C^T x); deriv 0 none, 1
    centered, 2 forward."""
    x = np.ascontiguousarray(x)
    if not deriv:
        return conv_ref(x, h, offset, adjoint)
    if adjoint:
        return fd_ref(conv_ref(x, h, offset, True), deriv, True)
    return conv_ref(fd_ref(x, deriv, False), h, offset, False)


def dense(fn, d, dtype=np.float64):
    """The d x d matrix of a linear map on [1, d, 1] arrays, column by
    column from the identity."""
    cols = [fn(np.eye(d, dtype=dtype)[:, i].reshape(1, d, 1)).ravel()
            for i in range(d)]
    return np.stack(cols, axis=1)


def fd_matrix(d, deriv, dtype=np.float64):
    """The explicit first-derivative matrix D (edge False, sampling 1):
    centered (deriv 1) rows 1..d-2 hold (-0.5, 0, 0.5); forward (deriv 2)
    rows 0..d-2 hold (-1, 1)."""
    D = np.zeros((d, d), dtype=dtype)
    if deriv == 1:
        for g in range(1, d - 1):
            D[g, g - 1], D[g, g + 1] = -0.5, 0.5
    else:
        for g in range(d - 1):
            D[g, g], D[g, g + 1] = -1.0, 1.0
    return D


def same_recipe(x, h, offset, adjoint):
    """pylops' Convolve1D recipe on one trace: pad h so that ``offset``
    becomes the centre, convolve (forward) or correlate (adjoint) in mode
    "same"."""
    nh = h.size
    pad = max(offset, nh - 1 - offset)      # new centre, length 2 pad + 1
    hp = np.zeros(2 * pad + 1, dtype=h.dtype)
    hp[pad - offset:pad - offset + nh] = h
    d = x.size
    if adjoint:
        full = np.correlate(x, hp, mode="full")
    else:
        full = np.convolve(x, hp, mode="full")
    return full[pad:pad + d]

"""NumPy reference of pam_kirch (include/pam.h) for the kernel tests of
tests/test_gpu_kirch.py; checked on its own, on a CPU, by
tests/test_kirchref_cpu.py.

Tables are in samples and trace-major, qs (ns, ni) and qr (nr, ni); the
data is (ns, nr, nt), trace k = is * nr + ir.  Per pair, in the tables'
dtype: q = qs[is, i] + qr[ir, i], it = floor(q), w = q - it; the pair
contributes iff 0 <= it < nt - 1 (NaN, +-inf and negative q do not).
Each function loops over the traces and is vectorised over the image
points, which keeps the per-point order of the C loop (np.add.at adds
unbuffered, in index order).

``gather_ref`` is the pinned arithmetic of the adjoint: acc = 0, traces
ascending inside a chunk, term = ((1 - w) * d0) + (w * d1), acc += term,
the chunks' partial sums added in ascending order — bit for bit what the
kernel gives when ``chunk`` is what pam_kirch_chunk reports.
``spread_ref`` is the forward loop, image points ascending; the kernel's
order differs, so it is compared within ``spread_bound``."""
import numpy as np


def pairs(qs_row, qr_row, nt):
    """(keep, it, w) of one trace for every image point; it is 0 where the
    pair is skipped."""
    T = qs_row.dtype.type
    with np.errstate(invalid="ignore"):
        q = qs_row + qr_row
        keep = (q >= T(0)) & (q < T(nt))
        f = np.floor(np.where(keep, q, T(0)))
        it = f.astype(np.int64)
        keep &= it < nt - 1
        w = np.where(keep, q - f, T(0))
    return keep, np.where(keep, it, 0), w


def spread_ref(m, qs, qr, nt, acc=None):
    """d (ns, nr, nt): d[k, it] += m[i] * (1 - w), d[k, it + 1] += m[i] * w
    for i ascending; samples that receive nothing are 0.  The pair's
    geometry is taken in the tables' dtype, products and sums in ``acc``
    (default: m's dtype)."""
    acc = np.dtype(m.dtype if acc is None else acc).type
    ns, nr = qs.shape[0], qr.shape[0]
    d = np.zeros((ns, nr, nt), dtype=acc)
    mv = m.astype(acc)
    for s in range(ns):
        for r in range(nr):
            keep, it, w = pairs(qs[s], qr[r], nt)
            it, w, mk = it[keep], w[keep].astype(acc), mv[keep]
            idx = np.stack([it, it + 1], axis=1).ravel()
            val = np.stack([mk * (acc(1) - w), mk * w], axis=1).ravel()
            np.add.at(d[s, r], idx, val)
    return d


def spread_count(qs, qr, nt):
    """Contributions per sample of spread_ref, (ns, nr, nt) int64: every
    contributing pair counts once at it and once at it + 1."""
    ns, nr = qs.shape[0], qr.shape[0]
    n = np.zeros((ns, nr, nt), dtype=np.int64)
    for s in range(ns):
        for r in range(nr):
            keep, it, _ = pairs(qs[s], qr[r], nt)
            np.add.at(n[s, r], it[keep], 1)
            np.add.at(n[s, r], it[keep] + 1, 1)
    return n


def spread_bound(m, qs, qr, nt):
    """(n + 2) * eps_T * spread_ref(|m|) per sample, the sum in float64:
    the bound of a sum of n products in any order, each product carrying
    the roundings of 1 - w and of the multiply."""
    eps = float(np.finfo(m.dtype).eps)
    mag = spread_ref(np.abs(m), qs, qr, nt, acc=np.float64)
    return (spread_count(qs, qr, nt) + 2) * eps * mag


def gather_ref(d, qs, qr, chunk=None):
    """mig (ni,): per chunk of ``chunk`` traces acc = 0, k ascending,
    acc += ((1 - w) * d[k, it]) + (w * d[k, it + 1]); the chunks' sums are
    added in ascending order.  chunk None (or >= ns * nr): one chunk."""
    T = d.dtype.type
    ns, nr, nt = d.shape
    ntr, ni = ns * nr, qs.shape[1]
    chunk = ntr if chunk is None else max(1, min(int(chunk), ntr))
    total = None
    for k0 in range(0, ntr, chunk):
        part = np.zeros(ni, dtype=d.dtype)
        for k in range(k0, min(k0 + chunk, ntr)):
            s, r = divmod(k, nr)
            keep, it, w = pairs(qs[s], qr[r], nt)
            with np.errstate(all="ignore"):
                term = ((T(1) - w) * d[s, r, it]) + (w * d[s, r, it + 1])
                part[keep] += term[keep]
        with np.errstate(all="ignore"):
            total = part if total is None else total + part
    return total


def dense(qs, qr, nt, dtype=np.float64):
    """The (ns * nr * nt, ni) matrix of the spread, column by column."""
    ni = qs.shape[1]
    cols = [spread_ref(np.eye(ni, dtype=dtype)[i], qs, qr, nt).ravel()
            for i in range(ni)]
    return np.stack(cols, axis=1)

"""NumPy references, exact-integer data and 2-D operand placement for the
kernel-level tests of the GEMM family (tests/test_gpu_gemm.py; checked on
their own, on a CPU, by tests/test_gemmref_cpu.py).  The companion of
tests/primref.py, whose helpers and SENTINEL it shares.

References.  ``gemm`` and ``bgemm`` return (ref, bound): the product of the
STORED values in np.longdouble (complex: np.clongdouble, assembled from real
and imaginary parts) and the forward bound that holds for any summation
order with one rounding per operation,
  real:     (K + 1) u (|A| @ |B| + |C0|)
  complex:  (2K + 2) u ((|Ar| + |Ai|) @ (|Br| + |Bi|) + |C0r| + |C0i|)
            for the real and for the imaginary part,
u = 2^-53 (float64 / complex128) or 2^-24 (float32 / complex64): the kernels
accumulate in the array's real type.

Exact-integer data.  ``int_operand`` draws integers in [-2, 2] and adds a
row trend and a column trend in [-1, 1] each, so real and imaginary parts
lie in [-4, 4] and a transposed or shifted read is far off.  A product is at
most 32 in magnitude (complex: two products of 16 per part), so for K <= 520
every partial sum, in any order, stays below 2^15 and is exact in float32
and float64: the comparison is equality with an int64 matmul (``int_gemm``,
which asserts max |ref| < 2^24).

Placement.  ``Placed2D`` puts a [rows, cols] operand or a [batch, rows, cols]
stack inside a larger device buffer of its real type: leading dimension
ld >= cols, batch stride >= rows * ld, GUARD reals before and after, the
start 0 or 1 element off 16-byte alignment as in primref.Placed.  Padding
and guards hold ``fill``: NaN for an input (a stray load that reaches a
stored result shows up as NaN), SENTINEL for an output."""
import numpy as np

import primref as pr
from primref import GUARD, LD, SENTINEL, is_complex, real_type

INT_LIMIT = 2 ** 24

# The shapes of tests/test_gpu_gemm.py, (M, K, N).  pam_gemm: f64 tile
# 128x64, BK 16, 2-wide loads; f32 tile 128x128, BK 32, 4-wide loads.
GEMM_SHAPES = [
    (1, 1, 1), (1, 0, 1), (130, 0, 70),
    # unguarded kernels: one, two, three and six f64 panels, 1..3 of f32
    (128, 16, 64), (128, 32, 128), (256, 64, 128), (128, 48, 128),
    (128, 96, 256),
    # tile edges -1 / +1, K around one panel of either kernel
    (127, 16, 63), (129, 17, 65), (127, 33, 129), (129, 31, 127),
    (128, 15, 64), (128, 48, 127),
    # K 1..3 past a full panel; N, K not multiples of the vector width, so
    # the last vector straddles the edge and only the vector guard decides
    (130, 19, 62), (65, 34, 130), (64, 35, 66), (256, 18, 131),
    (70, 67, 260), (1, 257, 130), (513, 5, 3)]
GEMM_OFF_SHAPES = [(128, 32, 128), (256, 64, 128), (129, 17, 65),
                   (64, 35, 66), (1, 257, 130)]
GEMM_RANDOM_SHAPES = [(1, 1, 1), (130, 0, 70), (128, 32, 128),
                      (128, 96, 256), (129, 17, 65), (64, 35, 66),
                      (70, 67, 260), (1, 257, 130), (513, 5, 3)]
# batched kernels, (batch, M, K, N): 64x64 tile, BK 16; complex without
# accumulate BK 8 up to K = 64
BATCHED_SHAPES = [
    (1, 1, 0, 1), (3, 65, 0, 63), (1, 1, 1, 1), (3, 64, 1, 65),
    (3, 63, 7, 65), (1, 64, 8, 64), (3, 65, 9, 1), (1, 64, 16, 64),
    (1, 63, 16, 1), (3, 129, 17, 63), (3, 64, 64, 64), (1, 129, 64, 65),
    (3, 63, 65, 64), (1, 65, 65, 129), (3, 1, 80, 129), (1, 129, 80, 129)]
BATCHED_RANDOM_SHAPES = [(3, 65, 0, 63), (3, 63, 7, 65), (3, 129, 17, 63),
                         (1, 129, 64, 65), (1, 65, 65, 129),
                         (3, 1, 80, 129)]
# added for the 128x64 complex tile, which wants M >= 128
VARIANT_SHAPES = [(2, 128, 64, 64), (1, 256, 48, 70)]
KT_SHAPES = [(256, 32, 256), (256, 64, 512), (512, 96, 256),
             (512, 512, 512)]


def unit(dt):
    """Unit roundoff of the array's real type."""
    return LD(2.0) ** (-53 if real_type(dt) is np.float64 else -24)


# --------------------------------------------------------------- references
def op(A, opa):
    """op(A) on the last two axes: A, or its (conjugate) transpose."""
    if not opa:
        return A
    At = np.swapaxes(A, -1, -2)
    return np.conj(At) if np.iscomplexobj(At) else At


def product(A, B, opa=False):
    """(ref, mag) of op(A) @ B without C0: the longdouble product and the
    magnitude sum |A| @ |B| (complex: (|Ar| + |Ai|) @ (|Br| + |Bi|)) that
    its bound is made of.  The expensive half of ``bgemm``, for callers
    that share one product between the plain and the accumulating run."""
    assert A.dtype == B.dtype
    A = op(A, opa)
    if not is_complex(A.dtype):
        Al, Bl = A.astype(LD), B.astype(LD)
        return np.matmul(Al, Bl), np.matmul(np.abs(Al), np.abs(Bl))
    ar, ai = A.real.astype(LD), A.imag.astype(LD)
    br, bi = B.real.astype(LD), B.imag.astype(LD)
    ref = np.empty(np.broadcast_shapes(ar.shape[:-2], br.shape[:-2])
                   + (ar.shape[-2], br.shape[-1]), dtype=np.clongdouble)
    ref.real = np.matmul(ar, br) - np.matmul(ai, bi)
    ref.imag = np.matmul(ar, bi) + np.matmul(ai, br)
    return ref, np.matmul(np.abs(ar) + np.abs(ai), np.abs(br) + np.abs(bi))


def finish(ref, mag, K, dt, C0=None):
    """(ref + C0, bound) from ``product``'s pair."""
    if C0 is not None:
        assert C0.dtype == dt
        if is_complex(dt):
            cr, ci = C0.real.astype(LD), C0.imag.astype(LD)
            ref = ref.copy()
            ref.real, ref.imag = ref.real + cr, ref.imag + ci
            mag = mag + np.abs(cr) + np.abs(ci)
        else:
            ref, mag = ref + C0.astype(LD), mag + np.abs(C0.astype(LD))
    ops = 2 * K + 2 if is_complex(dt) else K + 1
    return ref, ops * unit(dt) * mag


def bgemm(A, B, C0=None, opa=False):
    """(ref, bound) of op(A) @ B (+ C0) on [.., rows, cols] operands of one
    dtype; A broadcasts over the batch of B.  The bound of a complex result
    applies to its real and to its imaginary part."""
    ref, mag = product(A, B, opa)
    return finish(ref, mag, op(A, opa).shape[-1], A.dtype, C0)


def gemm(A, B, C0=None):
    """(ref, bound) of A @ B (+ C0)."""
    return bgemm(A, B, C0, False)


def err_ratio(got, ref, bound):
    """max err / bound over all real and imaginary parts; an entry whose
    bound is 0 (K == 0 without accumulate) must be exact: ratio 0 or inf."""
    if np.iscomplexobj(ref):
        err = np.maximum(np.abs(got.real.astype(LD) - ref.real),
                         np.abs(got.imag.astype(LD) - ref.imag))
    else:
        err = np.abs(got.astype(LD) - ref)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / bound)
    return float(np.max(r))


# ------------------------------------------------------- exact-integer data
def _trend(shape):
    rows, cols = shape[-2:]
    row = (np.arange(rows) % 3 - 1)[:, None]
    col = (np.arange(cols) % 5 % 3 - 1)[None, :]
    return row + col                        # in [-2, 2]


def int_operand(rng, shape, dt):
    """Integers in [-4, 4] (both parts of a complex dtype): uniform draws in
    [-2, 2] plus a row trend and a column trend."""
    t = _trend(shape)
    x = rng.integers(-2, 3, shape) + t
    if is_complex(dt):
        x = x + 1j * (rng.integers(-2, 3, shape) - t)
    x = x.astype(dt)
    assert np.max(np.abs(pr.rview(x)), initial=0) <= 4
    return x


def _ints(x):
    if is_complex(x.dtype):
        return x.real.astype(np.int64), x.imag.astype(np.int64)
    return x.astype(np.int64), None


def int_gemm(A, B, C0=None, opa=False):
    """op(A) @ B (+ C0) of integer-valued operands through int64, returned
    in the operands' dtype; asserts that every entry and every possible
    partial sum (sum |a| |b| + |c0|) is below 2^24."""
    dt = A.dtype
    ar, ai = _ints(op(A, opa))
    br, bi = _ints(B)
    for x in (A, B) + (() if C0 is None else (C0,)):
        r = pr.rview(x.reshape(-1))
        assert x.dtype == dt and np.array_equal(r, np.rint(r))
    if ai is None:
        re, im = np.matmul(ar, br), None
        mag = np.matmul(np.abs(ar), np.abs(br))
    else:
        re = np.matmul(ar, br) - np.matmul(ai, bi)
        im = np.matmul(ar, bi) + np.matmul(ai, br)
        mag = np.matmul(np.abs(ar) + np.abs(ai), np.abs(br) + np.abs(bi))
    if C0 is not None:
        cr, ci = _ints(C0)
        re, mag = re + cr, mag + np.abs(cr)
        if im is not None:
            im, mag = im + ci, mag + np.abs(ci)
    assert np.max(mag, initial=0) < INT_LIMIT
    if im is None:
        return re.astype(dt)
    out = np.empty(re.shape, dtype=dt)
    out.real, out.imag = re, im
    return out


# ---------------------------------------------------------------- placement
class Placed2D:
    """A [rows, cols] operand or a [batch, rows, cols] stack on the device,
    inside a ``fill``-filled buffer of its real type.

    ld: leading dimension in elements (default cols); bstride: batch stride
    in elements (default rows * ld); off: 0, or 1 to start one element
    (complex128: one real) later, as primref.Placed.  The buffer ends GUARD
    (+2) reals after the last element of the last row: the padding of the
    last row is not part of the operand."""

    def __init__(self, arr, ld=None, bstride=None, off=0, fill=SENTINEL,
                 device="cuda:0", guard=GUARD):
        import torch
        arr = np.asarray(arr)
        assert arr.ndim in (2, 3)
        self.shape, self.dtype, self.off = arr.shape, arr.dtype, off
        batch = arr.shape[0] if arr.ndim == 3 else 1
        rows, cols = arr.shape[-2:]
        a3 = arr.reshape(batch, rows, cols)
        self.rtype = real_type(arr.dtype)
        w = self.w = 2 if is_complex(arr.dtype) else 1
        self.ld = cols if ld is None else ld
        self.bstride = rows * self.ld if bstride is None else bstride
        assert self.ld >= cols and self.bstride >= rows * self.ld
        assert guard % 4 == 0
        self.lo = guard + off * (2 if arr.dtype == np.complex64 else 1)
        span = ((batch - 1) * self.bstride + (rows - 1) * self.ld + cols
                if arr.size else 0)
        self.hi = self.lo + span * w
        b, r, c, p = np.ix_(np.arange(batch), np.arange(rows),
                            np.arange(cols), np.arange(w))
        self.index = (self.lo + (b * self.bstride + r * self.ld + c) * w
                      + p).reshape(-1)
        assert self.index.size == 0 or (
            self.index.min() == self.lo and self.index.max() == self.hi - 1)
        img = np.full(self.hi + guard + 2, fill, dtype=self.rtype)
        img[self.index] = pr.rview(a3.reshape(-1))
        self.mask = np.zeros(img.size, dtype=bool)
        self.mask[self.index] = True
        self.image = img                    # what was uploaded
        self.buf = torch.from_numpy(img.copy()).to(device)
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + self.lo * img.itemsize
        assert self.ptr % 16 == (0 if not off else
                                 4 if self.rtype is np.float32 and w == 1
                                 else 8)

    def fetch(self):
        """The whole buffer, padding and guards included, on the host."""
        return self.buf.cpu().numpy()

    def value(self, full=None):
        full = self.fetch() if full is None else full
        return np.ascontiguousarray(full[self.index]).view(
            self.dtype).reshape(self.shape)

    def guards_intact(self, full=None):
        """Guards, padding columns and inter-batch gaps hold the uploaded
        bits."""
        full = self.fetch() if full is None else full
        return np.array_equal(pr.bits(full[~self.mask]),
                              pr.bits(self.image[~self.mask]))

    def untouched(self, full=None):
        """Every real of the buffer holds the uploaded bits."""
        full = self.fetch() if full is None else full
        return np.array_equal(pr.bits(full), pr.bits(self.image))

"""NumPy references and operand placement for the kernel-level tests of the
vector primitives (tests/test_gpu_primitives.py; checked on their own, on a
CPU, by tests/test_primref_cpu.py).

References.  Each restates one entry point of include/pam.h in NumPy, in
the array's own dtype, with one rounding per operation and in the kernel's
order, so that the element-wise family can be compared bit for bit:
  * real-view ops (add, sub, neg, real-alpha scale / axpy / xpby) act on
    the interleaved real view of a complex array, as kernels.py launches
    them;
  * complex products are built from real and imaginary REAL arrays
    (re = ar*br - ai*bi, im = ar*bi + ai*br): every product and sum is then
    its own NumPy loop and is rounded once, which NumPy's complex multiply
    does not promise;
  * the thresholds are oracle/proximal.py's formulas, written out here in
    the array's dtype (real soft and hard: exact) or in float64 /
    complex128 of the stored values (complex soft, half);
  * the reductions return per-element float64 terms; their sum is taken in
    np.longdouble.

Placement.  ``Placed`` puts one operand inside a larger device buffer of
its real type, pre-filled with SENTINEL: GUARD reals of guard on each side
and the operand starting 0 or 1 element later (1: 8 bytes off 16-byte
alignment for float64 / complex64, 4 bytes for float32; for complex128 one
REAL later, which torch cannot view as complex — ``tensor`` is then None
and the caller passes ``ptr`` to the C-ABI)."""
import numpy as np

DTYPES = {"f64": np.float64, "f32": np.float32,
          "c128": np.complex128, "c64": np.complex64}
GUARD = 8               # reals: two float4 / four double2 vector widths
SENTINEL = -8191.5      # exact in float32; no data below is that large
HALF_CUT = 54.0 ** (1.0 / 3.0) / 4.0    # 0.944940787421...


def real_type(dt):
    return np.dtype(dt).type(0).real.dtype.type


def is_complex(dt):
    return np.issubdtype(np.dtype(dt), np.complexfloating)


def eps(dt):
    return float(np.finfo(real_type(dt)).eps)


def rview(a):
    """The interleaved real view of a (possibly complex) 1-D array."""
    a = np.ascontiguousarray(a)
    return a.view(real_type(a.dtype))


def bits(a):
    a = rview(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def same(got, want):
    """Equal values component by component: +-0 are equal (np.array_equal)
    and a NaN equals a NaN — inf - inf and 0 * inf occur in the data — but
    only in the same real or imaginary slot, hence the real views."""
    got, want = np.asarray(got), np.asarray(want)
    return (got.dtype == want.dtype and got.shape == want.shape
            and np.array_equal(rview(got), rview(want), equal_nan=True))


def _quiet(fn):
    def wrapped(*a, **k):
        with np.errstate(all="ignore"):
            return fn(*a, **k)
    wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
    return wrapped


# ------------------------------------------------------------ element-wise
def fill(n, value, dt):
    """pam_fill on the real view: every real (T)value."""
    out = np.empty(n, dtype=dt)
    rview(out)[...] = real_type(dt)(value)
    return out


@_quiet
def neg(x):
    return (-rview(x)).view(x.dtype)


@_quiet
def add(a, b):
    return (rview(a) + rview(b)).view(a.dtype)


@_quiet
def sub(a, b):
    return (rview(a) - rview(b)).view(a.dtype)


@_quiet
def scale(x, alpha):
    """y = T(alpha) * x, REAL alpha, componentwise"""
    return (real_type(x.dtype)(alpha) * rview(x)).view(x.dtype)


@_quiet
def axpy(y, x, alpha):
    """y + T(alpha) * x: the product is rounded, then the sum"""
    return (rview(y) + real_type(y.dtype)(alpha) * rview(x)).view(y.dtype)


@_quiet
def xpby(y, x, beta):
    """x + T(beta) * y"""
    return (rview(x) + real_type(y.dtype)(beta) * rview(y)).view(y.dtype)


def axpy_d(y, x, alpha64, scale_):
    """the device-scalar form: the scalar is T(scale * alpha64), the
    product taken in float64"""
    return axpy(y, x, np.float64(scale_) * np.float64(alpha64))


def xpby_d(y, x, beta64, scale_):
    return xpby(y, x, np.float64(scale_) * np.float64(beta64))


def _parts(z):
    return np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)


def _join(re, im, dt):
    out = np.empty(re.shape, dtype=dt)
    out.real, out.imag = re, im
    return out


@_quiet
def cmul(a, b):
    ar, ai = _parts(a)
    br, bi = _parts(b)
    return _join(ar * br - ai * bi, ar * bi + ai * br, a.dtype)


@_quiet
def mul(a, b):
    return cmul(a, b) if is_complex(a.dtype) else a * b


@_quiet
def cscale(x, alpha):
    """complex alpha, its parts cast to the array's real type"""
    R = real_type(x.dtype)
    ar, ai = R(complex(alpha).real), R(complex(alpha).imag)
    xr, xi = _parts(x)
    return _join(xr * ar - xi * ai, xr * ai + xi * ar, x.dtype)


def conj(x):
    xr, xi = _parts(x)
    return _join(xr, -xi, x.dtype)


def scalar_alpha(num, den0, den1, damp):
    with np.errstate(all="ignore"):
        return np.abs(np.float64(num) / (np.float64(den0)
                                         + np.float64(damp) * np.float64(den1)))


def scalar_div(num, den):
    with np.errstate(all="ignore"):
        return np.abs(np.float64(num) / np.float64(den))


# ---------------------------------------------------------------- threshold
def cast_thresh(t, dt):
    """The threshold as the kernel holds it: (T)t."""
    return float(real_type(dt)(t))


def decision_point(kind, t):
    """|x| at which thresholding switches branch: t (soft), sqrt(2 t)
    (hard), (54^(1/3) / 4) t^(2/3) (half)."""
    return {0: t, 1: np.sqrt(2.0 * t), 2: HALF_CUT * t ** (2.0 / 3.0)}[kind]


def thresh_margin(x, kind, t):
    """Smallest relative distance of any |x| from the decision point."""
    if x.size == 0:
        return np.inf
    pt = decision_point(kind, t)
    wide = np.complex128 if is_complex(x.dtype) else np.float64
    return float(np.min(np.abs(np.abs(x.astype(wide)) - pt)) / pt)


def thresh_data(rng, dt, n, kind, t, margin=1e-3):
    """Normals scaled by 2, one exact zero; every magnitude within a
    relative ``margin`` of the decision point is moved to twice that
    point, so no element sits where one rounding decides the branch."""
    x = 2.0 * rng.standard_normal(n)
    if is_complex(dt):
        x = x + 2.0j * rng.standard_normal(n)
    if n >= 3:
        x[n // 2] = 0.0
    pt = decision_point(kind, t)
    a = np.abs(x)
    near = np.abs(a - pt) <= 2.0 * margin * pt
    x[near] = x[near] * (2.0 * pt / a[near])
    return x.astype(dt)


@_quiet
def soft(x, t):
    """real: sign(x) * max(|x| - T(t), 0) in T — exact.  complex: the
    oracle's z * max(|z| - t, 0) / |z| in complex128 of the stored values,
    t being T(t)."""
    if is_complex(x.dtype):
        z = x.astype(np.complex128)
        a = np.abs(z)
        s = np.where(a > 0, np.maximum(a - cast_thresh(t, x.dtype), 0.0)
                     / np.where(a > 0, a, 1.0), 0.0)
        return z * s
    T = x.dtype.type
    return np.sign(x) * np.maximum(np.abs(x) - T(t), T(0))


@_quiet
def hard(x, t):
    """x where |x| >= sqrt(T(2) * T(t)), else 0; complex by magnitude
    (float64).  The factor is 0 or 1: exact away from the tie."""
    T = real_type(x.dtype)
    if is_complex(x.dtype):
        a = np.abs(x.astype(np.complex128))
        return np.where(a >= np.sqrt(2.0 * cast_thresh(t, x.dtype)), x,
                        x.dtype.type(0))
    return np.where(np.abs(x) >= np.sqrt(T(2) * T(t)), x, T(0))


@_quiet
def half(x, t):
    """The L1/2 prox (Xu et al. 2012) in float64 / complex128 of the
    stored values, t being T(t):
      |x| > (54^(1/3)/4) t^(2/3):
          (2/3) x (1 + cos(2 pi / 3 - (2/3) acos((t/8) (|x|/3)^-1.5)))
      else 0."""
    t = cast_thresh(t, x.dtype)
    z = x.astype(np.complex128 if is_complex(x.dtype) else np.float64)
    a = np.abs(z)
    above = a > HALF_CUT * t ** (2.0 / 3.0)
    safe = np.where(above, a, 3.0)
    phi = np.arccos(np.clip((t / 8.0) * (safe / 3.0) ** -1.5, -1.0, 1.0))
    fac = (2.0 / 3.0) * (1.0 + np.cos(2.0 * np.pi / 3.0 - (2.0 / 3.0) * phi))
    return np.where(above, z * fac, 0.0)


THRESH_REF = {0: soft, 1: hard, 2: half}


# --------------------------------------------------------------- reductions
LD = np.longdouble
U = 2.0 ** -53          # unit roundoff of float64


def _f64_parts(z):
    return z.real.astype(np.float64), z.imag.astype(np.float64)


@_quiet
def dot_terms(x, y):
    """x[i] * y[i] in float64 (exact for float32 inputs)"""
    return x.astype(np.float64) * y.astype(np.float64)


@_quiet
def cdot_terms(x, y, conjx):
    """(re, im) terms of sum x*y or sum conj(x)*y, each part two float64
    products and their sum"""
    xr, xi = _f64_parts(x)
    yr, yi = _f64_parts(y)
    if conjx:
        xi = -xi
    return xr * yr - xi * yi, xr * yi + xi * yr


@_quiet
def powsum_terms(x, p):
    """|x^p| per element, np.float_power semantics: on a real dtype a
    negative x with a fractional p gives NaN (complex: |z|^p).  p == 1 on
    reals and p == 2 are float64 arithmetic as the kernel does it (x*x, or
    zr*zr + zi*zi); every other term — |z| and a general power — is
    evaluated in np.longdouble."""
    if is_complex(x.dtype):
        zr, zi = _f64_parts(x)
        if p == 2:
            return zr * zr + zi * zi
        a = np.hypot(zr.astype(LD), zi.astype(LD))
        return a if p == 1 else a ** LD(p)
    xv = x.astype(np.float64)
    if p == 2:
        return xv * xv
    return (np.abs(xv) if p == 1
            else np.abs(np.float_power(xv.astype(LD), LD(p))))


@_quiet
def abs_terms(x):
    """|x| for the max / min norms: exact on reals, longdouble hypot on
    complex"""
    if is_complex(x.dtype):
        zr, zi = _f64_parts(x)
        return np.hypot(zr.astype(LD), zi.astype(LD))
    return np.abs(x.astype(np.float64))


def count_nonzero(x):
    """NaN counts as nonzero (NaN != 0), as np.count_nonzero has it"""
    return float(np.count_nonzero(x))


@_quiet
def lsum(terms):
    """np.longdouble sum of the terms and the forward bound
    n * 2^-53 * sum|terms| that holds for any float64 summation order"""
    t = np.asarray(terms).astype(LD)
    return t.sum(), t.size * LD(U) * np.abs(t).sum()


def gemv(A, x, trans):
    """(reference, bound) of y = A @ x or A^T @ x: longdouble products of
    the stored values and n * 2^-53 * (|A| @ |x|) per entry, n the length
    of the sums; + eps(float32) * |ref| for the final cast of a float32
    result."""
    Al, xl = A.astype(LD), x.astype(LD)
    if trans:
        Al = Al.T
    ref = Al @ xl
    bound = Al.shape[1] * LD(U) * (np.abs(Al) @ np.abs(xl))
    if A.dtype == np.float32:
        bound = bound + LD(eps(np.float32)) * np.abs(ref)
    return ref, bound


# ---------------------------------------------------------------- placement
class Placed:
    """One 1-D operand on the device, inside a SENTINEL-filled buffer of
    its real type.  ``off``: 0, or 1 to start one element (complex128:
    one real) later."""

    def __init__(self, arr, off=0, device="cuda:0", guard=GUARD):
        import torch
        arr = np.ascontiguousarray(arr).ravel()
        self.dtype, self.n, self.off = arr.dtype, arr.size, off
        self.rtype = real_type(arr.dtype)
        self.nreal = arr.size * (2 if is_complex(arr.dtype) else 1)
        assert guard % 4 == 0
        self.lo = guard + off * (2 if arr.dtype == np.complex64 else 1)
        self.hi = self.lo + self.nreal
        img = np.full(self.hi + guard + 2, SENTINEL, dtype=self.rtype)
        img[self.lo:self.hi] = rview(arr)
        self.image = img                    # what was uploaded
        self.buf = torch.from_numpy(img.copy()).to(device)
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + self.lo * img.itemsize
        assert self.ptr % 16 == (0 if not off else
                                 4 if self.rtype is np.float32
                                 and not is_complex(arr.dtype) else 8)
        v = self.buf[self.lo:self.hi]
        if is_complex(arr.dtype):
            v = None if self.lo % 2 else torch.view_as_complex(
                v.view(self.n, 2))
        self.tensor = v

    def fetch(self):
        """The whole buffer, guards included, on the host."""
        return self.buf.cpu().numpy()

    def value(self, full=None):
        full = self.fetch() if full is None else full
        return full[self.lo:self.hi].copy().view(self.dtype)

    def guards_intact(self, full=None):
        full = self.fetch() if full is None else full
        return (np.array_equal(bits(full[:self.lo]),
                               bits(self.image[:self.lo]))
                and np.array_equal(bits(full[self.hi:]),
                                   bits(self.image[self.hi:])))

    def untouched(self, full=None):
        """Guards and operand hold the uploaded bits."""
        full = self.fetch() if full is None else full
        return np.array_equal(bits(full), bits(self.image))

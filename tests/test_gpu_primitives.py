"""Kernel-by-kernel tests of the vector primitives in csrc/pam.hip: the
element-wise ops, thresholds, scalar kernels, reductions, GEMV and the
(de)interleave kernels, each against the plain NumPy reference of
tests/primref.py (itself checked in tests/test_primref_cpu.py).

Every operand is a view into a larger, sentinel-filled buffer
(primref.Placed): 16-byte aligned or one element off it, which selects the
vector or the scalar (V=1) kernel, and each operand is misaligned on its
own because vec_launch ANDs the alignment of all pointers.  After a
launch the guards of the output must hold the sentinel bit for bit and the
inputs their uploaded bits.  Calls go through pylops_mpi_amd.kernels; only
a complex128 operand one REAL off alignment, which torch cannot express,
goes to the same C entry point by raw pointer (and pam_fill, which the
kernels layer does not wrap).

Element-wise results are compared bit for bit (primref.same: +-0 equal,
NaN equal to NaN in the same slot).  Reductions are exact on integer
data; on random data they are held to n * 2^-53 * sum|terms|, the forward
bound of any float64 summation order, against an np.longdouble sum."""
import os
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest
import torch
from numpy.testing import assert_allclose

import primref as pr
from primref import Placed
from pylops_mpi_amd import _ffi, kernels

pytestmark = pytest.mark.gpu

DT = pr.DTYPES
NAMES = list(DT)
EW_SIZES = (0, 1, 2, 3, 4, 5, 7, 255, 256, 257, 511, 512, 513, 1023, 1024,
            1025, 1027, 4099)
OFFSETS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1))  # y, a, b
ALPHA = 0.7                     # not representable in float32 (or float64)
CALPHA = complex(0.7, -1.3)
A64 = 0.7 / 3.0                 # the device scalar of axpy_d / xpby_d
THRESH = 0.7


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev64(*vals):
    return torch.tensor(vals, dtype=torch.float64, device="cuda:0")


def diff(got, want):
    g, w = pr.rview(got), pr.rview(want)
    bad = np.flatnonzero(~((g == w) | (np.isnan(g) & np.isnan(w))))
    return (f"{bad.size} of {g.size} reals differ, first at {bad[:4]}: "
            f"got {g[bad[:4]]}, want {w[bad[:4]]}")


def check(y, want, msg):
    """Output ``y`` holds ``want`` bit for bit, its guards the sentinel."""
    full = y.fetch()
    assert y.guards_intact(full), f"guard overwritten: {msg}"
    got = y.value(full)
    assert pr.same(got, want), f"{msg}: {diff(got, want)}"


@lru_cache(maxsize=None)
def ew_data(dname, n, seed):
    """Standard normals with, from n = 255 up, denormals, +-0 and +-inf
    sprinkled at seed-dependent places.  Shared and read-only."""
    dt = DT[dname]
    rng = np.random.default_rng([seed, n, NAMES.index(dname)])
    x = rng.standard_normal(n)
    if pr.is_complex(dt):
        x = x + 1j * rng.standard_normal(n)
    x = x.astype(dt)
    if n >= 255:
        fi = np.finfo(pr.real_type(dt))
        sp = [fi.smallest_subnormal, -3 * fi.smallest_subnormal,
              fi.tiny / 4, -fi.tiny * 0.75, 0.0, -0.0, np.inf, -np.inf]
        r = pr.rview(x)
        r[(np.arange(len(sp)) * 31 + 5 * seed + 1) % r.size] = sp
    x.setflags(write=False)
    return x


# ------------------------------------------------------------ element-wise
# complex entry points kernels.py routes to (everything else runs complex
# arrays through the real kernels on the interleaved view)
CPLX_ENTRY = {"mul": "pam_cmul", "conj": "pam_conj", "cscale": "pam_cscale",
              "thresh": "pam_thresh"}


def ew(name, y, ins, *scal):
    """kernels.<name>(y, *ins, *scal) on the placed operands.  A complex128
    operand one real off alignment has no tensor: the entry point
    kernels.py would pick is then called with the raw pointers."""
    ts = [p.tensor for p in (y, *ins)]
    if all(t is not None for t in ts):
        return getattr(kernels, name)(*ts, *scal)
    assert y.dtype == np.complex128
    entry = CPLX_ENTRY.get(name)
    n, code = (y.n, _ffi.C128) if entry else (2 * y.n, _ffi.F64)
    post = ()
    if name == "thresh":
        pre, post = (), (int(scal[0]), float(scal[1]))
    elif name == "cscale":
        pre = (scal[0].real, scal[0].imag)
    elif name in ("axpy_d", "xpby_d"):
        pre = (scal[0].data_ptr(), float(scal[1]))
    else:
        pre = tuple(float(s) for s in scal)
    rc = getattr(_ffi.lib(), entry or "pam_" + name)(
        stream(), y.ptr, *[p.ptr for p in ins], *pre, n, *post, code)
    assert rc == 0, (name, rc)


REF = {     # (y before the call, input arrays, scalars) -> expected y
    "neg": lambda y, i, s: pr.neg(i[0]),
    "add": lambda y, i, s: pr.add(i[0], i[1]),
    "sub": lambda y, i, s: pr.sub(i[0], i[1]),
    "mul": lambda y, i, s: pr.mul(i[0], i[1]),
    "conj": lambda y, i, s: pr.conj(i[0]),
    "scale": lambda y, i, s: pr.scale(i[0], s[0]),
    "cscale": lambda y, i, s: pr.cscale(i[0], s[0]),
    "axpy": lambda y, i, s: pr.axpy(y, i[0], s[0]),
    "xpby": lambda y, i, s: pr.xpby(y, i[0], s[0]),
    "axpy_d": lambda y, i, s: pr.axpy_d(y, i[0], A64, s[1]),
    "xpby_d": lambda y, i, s: pr.xpby_d(y, i[0], A64, s[1]),
}


def ew_cases(dname, alpha_t):
    """(kernel, operand roles, scalars): roles[0] is the output."""
    c = [("neg", "ya", ()), ("add", "yab", ()), ("sub", "yab", ()),
         ("mul", "yab", ()), ("scale", "ya", (ALPHA,)),
         ("axpy", "ya", (ALPHA,)), ("xpby", "ya", (-ALPHA,))]
    c += [(k, "ya", (alpha_t, s)) for k in ("axpy_d", "xpby_d")
          for s in (1.0, -1.0)]
    if pr.is_complex(DT[dname]):
        c += [("conj", "ya", ()), ("cscale", "ya", (CALPHA,))]
    return c


def alias_cases(dname, alpha_t):
    """Every aliasing the package uses — the in-place y of axpy / xpby
    (DistributedArray.iaxpy_, xpby_ and their device-scalar forms, also
    with x the same array: x += x) and thresh(y, y) (sparsity.py, tested
    with the thresholds) — and the output standing for either input."""
    c = [("add", "yyb", ()), ("add", "yay", ()), ("sub", "yyb", ()),
         ("sub", "yay", ()), ("mul", "yyy", ()), ("mul", "yyb", ()),
         ("mul", "yay", ()), ("add", "yyy", ()), ("neg", "yy", ()),
         ("scale", "yy", (ALPHA,)), ("axpy", "yy", (ALPHA,)),
         ("xpby", "yy", (-ALPHA,)), ("axpy_d", "yy", (alpha_t, -1.0)),
         ("xpby_d", "yy", (alpha_t, 1.0))]
    if pr.is_complex(DT[dname]):
        c += [("conj", "yy", ()), ("cscale", "yy", (CALPHA,))]
    return c


def run_ew_case(case, host, placed, msg):
    name, roles, scal = case
    y = placed["y"]
    ew(name, y, [placed[r] for r in roles[1:]], *scal)
    want = REF[name](host["y"], [host[r] for r in roles[1:]], scal)
    if y.n == 0:
        assert y.untouched(), f"n=0 wrote something: {msg}"
    check(y, want, f"{name}({','.join(roles)}) {msg}")


@pytest.mark.parametrize("dname", NAMES)
def test_elementwise_bitexact(dname):
    alpha_t = dev64(A64)
    for n in EW_SIZES:
        host = {r: ew_data(dname, n, s) for s, r in enumerate("yab")}
        for oy, oa, ob in OFFSETS:
            a, b = Placed(host["a"], oa), Placed(host["b"], ob)
            for case in ew_cases(dname, alpha_t):
                run_ew_case(case, host,
                            {"y": Placed(host["y"], oy), "a": a, "b": b},
                            f"{dname} n={n} offsets={oy}{oa}{ob}")
            assert a.untouched() and b.untouched(), (n, oy, oa, ob)


@pytest.mark.parametrize("dname", NAMES)
def test_elementwise_aliasing(dname):
    alpha_t = dev64(A64)
    for n in EW_SIZES:
        host = {r: ew_data(dname, n, s) for s, r in enumerate("yab")}
        for oy, oo in ((0, 0), (1, 1), (0, 1), (1, 0)):
            a, b = Placed(host["a"], oo), Placed(host["b"], oo)
            for case in alias_cases(dname, alpha_t):
                run_ew_case(case, host,
                            {"y": Placed(host["y"], oy), "a": a, "b": b},
                            f"{dname} n={n} offsets={oy}{oo}")
            assert a.untouched() and b.untouched(), (n, oy, oo)


@pytest.mark.parametrize("dname", NAMES)
def test_fill(dname):
    """pam_fill has no wrapper in kernels.py: the C entry point, on the
    real view as the other componentwise kernels run complex arrays."""
    dt = DT[dname]
    k = 2 if pr.is_complex(dt) else 1
    code = _ffi.F64 if pr.real_type(dt) is np.float64 else _ffi.F32
    for n in EW_SIZES:
        for off in (0, 1):
            y = Placed(ew_data(dname, n, 0), off)
            rc = _ffi.lib().pam_fill(stream(), y.ptr, k * n, ALPHA, code)
            assert rc == 0
            check(y, pr.fill(n, ALPHA, dt), f"fill {dname} n={n} off={off}")


def test_scalar_kernels():
    for num in (-3.7, 2.5e-3):
        for d0, d1 in ((-1.3, 0.9), (0.3, -7.1), (1e-300, 3.0)):
            for damp in (0.0, 0.49):
                out = dev64(pr.SENTINEL, pr.SENTINEL, pr.SENTINEL)
                kernels.scalar_alpha(out[1:2], dev64(num), dev64(d0, d1),
                                     damp)
                want = pr.scalar_alpha(num, d0, d1, damp)
                assert out.cpu().tolist() == [pr.SENTINEL, want, pr.SENTINEL]
            out = dev64(pr.SENTINEL, pr.SENTINEL, pr.SENTINEL)
            kernels.scalar_div(out[1:2], dev64(num), dev64(d0))
            assert out.cpu().tolist() == [pr.SENTINEL,
                                          pr.scalar_div(num, d0), pr.SENTINEL]


# ---------------------------------------------------------------- threshold
def check_thresh(dname, kind, got, x0, msg):
    """Tolerances: real soft and hard, complex hard — exact.  Complex soft:
    8 eps max(|z|, t) absolute (y = z (a - t) / a: one ulp of hypot moves
    it by eps t, three more roundings are relative to |y| <= |z|).  Half:
    1e-12 in double precision; in single 4 eps |x| (the factor is formed
    in double, then two roundings in T and hypot for complex)."""
    dt = DT[dname]
    want = pr.THRESH_REF[kind](x0, THRESH)
    cplx = pr.is_complex(dt)
    if kind == 1 or (kind == 0 and not cplx):
        assert want.dtype == dt
        assert pr.same(got, want), f"{msg}: {diff(got, want)}"
        return
    wide = np.complex128 if cplx else np.float64
    err = np.abs(got.astype(wide) - want)
    mag = np.abs(x0.astype(wide))
    if kind == 0:
        bound = 8 * pr.eps(dt) * np.maximum(mag, pr.cast_thresh(THRESH, dt))
    elif pr.real_type(dt) is np.float64:
        assert_allclose(got, want, rtol=1e-12, atol=1e-12, err_msg=msg)
        return
    else:
        bound = 4 * pr.eps(np.float32) * mag
    worst = int(np.argmax(err - bound))
    assert np.all(err <= bound), (msg, worst, err[worst], bound[worst])
    assert np.array_equal(got == 0, want == 0), msg     # the same branch


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("dname", NAMES)
def test_thresh(dname, kind):
    dt = DT[dname]
    rng = np.random.default_rng([7, kind, NAMES.index(dname)])
    for n in (1, 255, 256, 257, 1025):
        x0 = pr.thresh_data(rng, dt, n, kind, THRESH)
        assert pr.thresh_margin(x0, kind, pr.cast_thresh(THRESH, dt)) >= 1e-3
        for oy, ox in ((0, 0), (1, 1), (1, 0), (0, None), (1, None)):
            msg = f"thresh {dname} kind={kind} n={n} offsets={oy}{ox}"
            y = Placed(np.full(n, 5, dtype=dt) if ox is not None else x0, oy)
            x = y if ox is None else Placed(x0, ox)     # None: in place
            ew("thresh", y, [x], kind, THRESH)
            full = y.fetch()
            assert y.guards_intact(full), msg
            check_thresh(dname, kind, y.value(full), x0, msg)
            assert x is y or x.untouched(), msg


@pytest.mark.parametrize("dname", ["f64", "f32"])
def test_soft_thresh_propagates_nan(dname):
    dt = DT[dname]
    rng = np.random.default_rng(8)
    for n in (65, 257):
        for pos in (0, n // 2, n - 1):
            x0 = pr.thresh_data(rng, dt, n, 0, THRESH)
            x0[pos] = np.nan
            want = pr.soft(x0, THRESH)
            assert np.isnan(want[pos]) and np.isnan(want).sum() == 1
            for off in (0, 1):
                y = Placed(x0, off)
                ew("thresh", y, [y], 0, THRESH)
                check(y, want, f"soft NaN {dname} n={n} pos={pos}")


# --------------------------------------------------------------- reductions
RED_SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 262143, 262144,
             262145, 524291)    # BLK * NPARTIAL = 262144: stage 1 strides


def red(name, ins, *extras):
    """kernels.<name>(*ins, *extras) -> float64 host array (1 or 2
    results); raw pointers for complex128 one real off alignment."""
    ts = [p.tensor for p in ins]
    if all(t is not None for t in ts):
        return getattr(kernels, name)(*ts, *extras).cpu().numpy().copy()
    lib = _ffi.lib()
    ws = torch.empty(2 * int(lib.pam_reduce_ws_elems()),
                     dtype=torch.float64, device="cuda:0")
    out = dev64(pr.SENTINEL, pr.SENTINEL, pr.SENTINEL)
    nout = 2 if name == "cdot" else 1
    rc = getattr(lib, "pam_" + name)(
        stream(), *[p.ptr for p in ins], ins[0].n,
        *[int(e) if i == 0 else float(e) for i, e in enumerate(extras)],
        ws.data_ptr(), out.data_ptr(), _ffi.C128)
    assert rc == 0, (name, rc)
    got = out.cpu().numpy()
    assert np.all(got[nout:] == pr.SENTINEL)
    return got[:nout].copy()


def norm(x, op, p=0.0):
    return red("norm_local", [x], op, p)[0]


@lru_cache(maxsize=None)
def int_data(dname, n, seed, axis_only=False):
    """Integers in [-4, 4] (zeros included): every product and partial sum
    is exact in float64 whatever the tree.  ``axis_only``: complex values
    with one part zero, so that |z| is an integer too."""
    dt = DT[dname]
    rng = np.random.default_rng([seed, n, 99])
    x = rng.integers(-4, 5, n).astype(np.float64)
    if pr.is_complex(dt):
        im = rng.integers(-4, 5, n)
        if axis_only:
            pick = rng.integers(0, 2, n).astype(bool)
            x = np.where(pick, x, 0) + 1j * np.where(pick, 0, im)
        else:
            x = x + 1j * im
    x = x.astype(dt)
    x.setflags(write=False)
    return x


@lru_cache(maxsize=None)
def normal_data(dname, n, seed):
    dt = DT[dname]
    rng = np.random.default_rng([seed, n, 77])
    x = rng.standard_normal(n)
    if pr.is_complex(dt):
        x = x + 1j * rng.standard_normal(n)
    x = x.astype(dt)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("dname", NAMES)
def test_reductions_exact_on_integers(dname):
    dt = DT[dname]
    cplx = pr.is_complex(dt)
    for n in RED_SIZES:
        x0, y0 = int_data(dname, n, 0), int_data(dname, n, 1)
        xi = x0.astype(np.complex128 if cplx else np.float64)
        yi = y0.astype(np.complex128 if cplx else np.float64)
        for off in (0, 1):
            msg = f"{dname} n={n} off={off}"
            x, y = Placed(x0, off), Placed(y0, off)
            if cplx:
                for conjx in (False, True):
                    want = np.sum((np.conj(xi) if conjx else xi) * yi)
                    got = red("cdot", [x, y], conjx)
                    assert got.tolist() == [want.real, want.imag], \
                        (msg, conjx)
                ax = int_data(dname, n, 2, axis_only=True)
                assert norm(Placed(ax, off), 0, 1.0) == np.sum(
                    np.abs(ax.real) + np.abs(ax.imag)), msg
            else:
                assert red("dot", [x, y])[0] == np.sum(xi * yi), msg
                assert norm(x, 0, 1.0) == np.sum(np.abs(xi)), msg
                assert norm(x, 1) == np.max(np.abs(xi), initial=0.0), msg
                assert norm(x, 2) == np.min(np.abs(xi), initial=np.inf), msg
            assert norm(x, 0, 2.0) == np.sum(xi.real ** 2
                                             + xi.imag ** 2), msg
            assert norm(x, 3) == np.count_nonzero(x0), msg
            if n == 0:      # the documented empty results
                assert [norm(x, 0, 2.0), norm(x, 1), norm(x, 2),
                        norm(x, 3)] == [0.0, 0.0, np.inf, 0.0], msg
            assert x.untouched() and y.untouched(), msg


def poke(x, pos, value):
    """Overwrite element ``pos`` of the placed operand on the device."""
    k = 2 if pr.is_complex(x.dtype) else 1
    v = complex(value)
    x.buf[x.lo + k * pos] = v.real
    if k == 2:
        x.buf[x.lo + k * pos + 1] = v.imag


@pytest.mark.parametrize("dname", NAMES)
def test_reductions_find_one_element(dname):
    """A unique largest, a unique smallest and an only nonzero element at
    the first, middle and last index (and at 262144, the first element of
    the second stride pass) of an otherwise constant array.  Complex
    values are Pythagorean — |9+12j| = 15, |9+40j| = 41, |9+0j| = 9 — and
    the sentinels differ from the constant in the imaginary part only."""
    dt = DT[dname]
    base, big, small, lone = ((9 + 12j, 9 + 40j, 9 + 0j, 40j)
                              if pr.is_complex(dt) else (2.0, -3.0, 1.0, -3.0))
    for n in RED_SIZES[1:]:
        spots = sorted({0, n // 2, n - 1} | ({262144} if n == 262145
                                             else set()))
        for off in (0, 1):
            x = Placed(np.full(n, base, dtype=dt), off)
            z = Placed(np.zeros(n, dtype=dt), off)
            for pos in spots:
                msg = f"{dname} n={n} off={off} pos={pos}"
                poke(x, pos, big)
                assert norm(x, 1) == abs(big), msg
                assert norm(x, 2) == abs(base if n > 1 else big), msg
                poke(x, pos, small)
                assert norm(x, 2) == abs(small), msg
                assert norm(x, 1) == abs(base if n > 1 else small), msg
                poke(x, pos, base)
                poke(z, pos, lone)
                assert norm(z, 3) == 1.0, msg
                assert norm(z, 1) == abs(lone), msg
                assert norm(z, 2) == (0.0 if n > 1 else abs(lone)), msg
                assert norm(z, 0, 2.0) == abs(lone) ** 2, msg
                poke(z, pos, 0.0)
            assert norm(z, 3) == 0.0 and norm(x, 1) == abs(base)
            assert x.guards_intact() and z.guards_intact()


def within(got, terms, msg):
    ref, bound = pr.lsum(terms)
    err = abs(np.longdouble(got) - ref)
    print(f"{msg}: got {got!r} err {float(err):.3e} bound {float(bound):.3e}")
    assert err <= bound, (msg, got, float(ref), float(err), float(bound))


@pytest.mark.parametrize("dname", NAMES)
def test_reductions_rounded(dname):
    dt = DT[dname]
    cplx = pr.is_complex(dt)
    for n in RED_SIZES[1:]:
        x0, y0 = normal_data(dname, n, 0), normal_data(dname, n, 1)
        dots = ({c: pr.cdot_terms(x0, y0, c) for c in (False, True)}
                if cplx else pr.dot_terms(x0, y0))
        pows = {p: pr.powsum_terms(x0, p) for p in (1.0, 2.0)}
        gen = {p: float(pr.lsum(pr.powsum_terms(x0, p))[0])
               for p in (3.0, 0.5)}
        absgen = float(pr.lsum(pr.powsum_terms(np.abs(x0), 0.5))[0])
        a = pr.abs_terms(x0)
        # |x| is exact on reals; one ulp for the complex hypot
        tol = 2.0 ** -52 if cplx else 0.0
        for off in (0, 1):
            msg = f"{dname} n={n} off={off}"
            x, y = Placed(x0, off), Placed(y0, off)
            if cplx:
                for conjx in (False, True):
                    got = red("cdot", [x, y], conjx)
                    within(got[0], dots[conjx][0],
                           f"cdot.re conjx={conjx} {msg}")
                    within(got[1], dots[conjx][1],
                           f"cdot.im conjx={conjx} {msg}")
            else:
                within(red("dot", [x, y])[0], dots, f"dot {msg}")
            for p in (1.0, 2.0):
                within(norm(x, 0, p), pows[p], f"powsum p={p} {msg}")
            # float_power semantics: on a real dtype a negative element
            # makes the p = 0.5 sum NaN (assert_allclose: NaN equals NaN),
            # so the fractional power is also run on |x|
            for p in (3.0, 0.5):
                assert_allclose(norm(x, 0, p), gen[p], rtol=1e-13,
                                err_msg=f"powsum p={p} {msg}")
            if not cplx:
                assert np.isnan(gen[0.5]) == bool(np.any(x0 < 0)), msg
                assert_allclose(norm(Placed(np.abs(x0), off), 0, 0.5),
                                absgen, rtol=1e-13, err_msg=msg)
            assert_allclose(norm(x, 1), float(a.max()), rtol=tol, atol=0)
            assert_allclose(norm(x, 2), float(a.min()), rtol=tol, atol=0)
            assert norm(x, 3) == n, msg
            assert x.untouched() and y.untouched(), msg


@pytest.mark.parametrize("dname", ["f32", "c64", "f64", "c128"])
def test_reductions_deterministic(dname):
    n = 524291
    x = Placed(normal_data(dname, n, 0), 0)
    y = Placed(normal_data(dname, n, 1), 1)
    name, extra = (("cdot", (True,)) if pr.is_complex(DT[dname])
                   else ("dot", ()))
    first = (red(name, [x, y], *extra), norm(x, 0, 2.0))
    for _ in range(3):
        again = (red(name, [x, y], *extra), norm(x, 0, 2.0))
        assert np.array_equal(pr.bits(first[0]), pr.bits(again[0]))
        assert np.float64(first[1]).tobytes() == np.float64(
            again[1]).tobytes()


@pytest.mark.parametrize("dname", NAMES)
def test_reductions_nonfinite(dname):
    """One NaN: the max and min norms, the power sums and the dot products
    return NaN (np.max(np.abs(x)) does) and count_nonzero counts it.  One
    +inf: max and the power sums are inf, min is unchanged."""
    dt = DT[dname]
    cplx = pr.is_complex(dt)
    for n in (65, 262145):
        x0, y0 = int_data(dname, n, 0), normal_data(dname, n, 1)
        for off in (0, 1):
            x, y = Placed(x0, off), Placed(y0, off)
            for pos in (0, n // 2, n - 1):
                msg = f"{dname} n={n} off={off} pos={pos}"
                x1 = x0.copy()
                # complex: the NaN sits in the imaginary part only
                x1[pos] = complex(x0[pos].real, np.nan) if cplx else np.nan
                poke(x, pos, x1[pos])
                for op, p in ((1, 0.0), (2, 0.0), (0, 1.0), (0, 2.0),
                              (0, 3.0)):
                    assert np.isnan(norm(x, op, p)), (msg, op, p)
                assert norm(x, 3) == np.count_nonzero(x1), msg
                if cplx:
                    for conjx in (False, True):
                        assert np.all(np.isnan(red("cdot", [x, y], conjx)))
                        assert np.all(np.isnan(red("cdot", [y, x], conjx)))
                else:
                    assert np.isnan(red("dot", [x, y])[0]), msg
                    assert np.isnan(red("dot", [y, x])[0]), msg
                x1[pos] = np.inf
                poke(x, pos, x1[pos])
                assert norm(x, 1) == np.inf, msg
                assert norm(x, 2) == float(pr.abs_terms(x1).min()), msg
                assert norm(x, 0, 1.0) == np.inf, msg
                assert norm(x, 0, 2.0) == np.inf, msg
                poke(x, pos, x0[pos])
            assert x.untouched() and y.untouched()


@pytest.mark.parametrize("dname", NAMES)
def test_empty_reductions_on_side_stream(dname):
    """n == 0 on a non-default stream: ``out`` is filled with the sentinel
    on that stream, then every reduction is called there with NULL arrays.
    After a stream sync ``out`` holds the documented empty result
    (include/pam.h) and the slots past it the sentinel: the result is
    written in stream order, after the fill.  pam_group_norm returns
    PAM_EARG for a NULL among its first ncomp components whatever n is
    (tests/test_group_cpu.py), so its unread components point at ``ws``."""
    lib, code = _ffi.lib(), NAMES.index(dname)
    side = torch.cuda.Stream()
    ws = torch.empty(2 * int(lib.pam_reduce_ws_elems()), dtype=torch.float64,
                     device="cuda:0")
    out = torch.empty(4, dtype=torch.float64, device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())
    s, w, o = side.cuda_stream, ws.data_ptr(), out.data_ptr()
    calls = [(f"norm_local op {op}", [want], lambda op=op: lib.pam_norm_local(
        s, None, 0, op, 2.0, w, o, code))
        for op, want in enumerate((0.0, 0.0, np.inf, 0.0))]
    if pr.is_complex(DT[dname]):
        calls += [(f"cdot conjx={c}", [0.0, 0.0], lambda c=c: lib.pam_cdot(
            s, None, None, 0, c, w, o, code)) for c in (0, 1)]
    else:
        calls.append(("dot", [0.0], lambda: lib.pam_dot(
            s, None, None, 0, w, o, code)))
    calls += [(f"group_norm ncomp={k}", [0.0], lambda k=k: lib.pam_group_norm(
        s, k, *([w] * k + [None] * (4 - k)), 0, w, o, code))
        for k in (1, 4)]
    for name, want, call in calls:
        with torch.cuda.stream(side):
            out.fill_(pr.SENTINEL)
        assert call() == 0, (dname, name)
        side.synchronize()
        got = out.cpu().numpy()
        assert pr.bits(got).tolist() == pr.bits(np.array(
            want + [pr.SENTINEL] * (4 - len(want)))).tolist(), (dname, name)


# --------------------------------------------------------------------- GEMV
GEMV_SHAPES = ((1, 1), (1, 257), (3, 4), (5, 63), (63, 64), (64, 65),
               (65, 255), (130, 256), (2, 1025), (4097, 3), (1000, 1))


@pytest.mark.parametrize("dname", ["f64", "f32"])
def test_gemv(dname):
    """Integer data: the exact integer product.  Random data with a row
    and a column trend (a transposed read is then far off): within
    nc * 2^-53 * (|A| @ |x|) of the longdouble product, nr for trans, plus
    eps(float32) |ref| for the float32 result's final cast."""
    dt = DT[dname]
    rng = np.random.default_rng([9, NAMES.index(dname)])
    for nr, nc in GEMV_SHAPES:
        Ai = rng.integers(-4, 5, (nr, nc))
        Ar = (rng.standard_normal((nr, nc)) + np.arange(nc) * 1e-3
              + np.arange(nr)[:, None] * 2e-3).astype(dt)
        for trans in (0, 1):
            nin, nout = (nr, nc) if trans else (nc, nr)
            xi = rng.integers(-4, 5, nin)
            xr = rng.standard_normal(nin).astype(dt)
            want_i = ((Ai.T if trans else Ai) @ xi).astype(dt)
            ref, bound = pr.gemv(Ar, xr, trans)
            for oa, ox in ((0, 0), (1, 0), (0, 1), (1, 1)):
                msg = f"gemv {dname} {nr}x{nc} trans={trans} offs={oa}{ox}"
                for A0, x0 in ((Ai.astype(dt), xi.astype(dt)), (Ar, xr)):
                    A, x = Placed(A0, oa), Placed(x0, ox)
                    y = Placed(np.full(nout, 5, dtype=dt), ox)
                    kernels.gemv(y.tensor, A.tensor.view(nr, nc), x.tensor,
                                 bool(trans))
                    full = y.fetch()
                    assert y.guards_intact(full), msg
                    got = y.value(full)
                    if A0 is Ar:
                        err = np.abs(got.astype(np.longdouble) - ref)
                        assert np.all(err <= bound), (
                            msg, float(np.max(err / bound)))
                    else:
                        assert pr.same(got, want_i), \
                            f"{msg}: {diff(got, want_i)}"
                    assert A.untouched() and x.untouched(), msg


# ----------------------------------------------------------- (de)interleave
ZIP_T_SHAPES = ((1, 1), (1, 33), (33, 1), (31, 32), (32, 33), (65, 7),
                (7, 65), (100, 37))
WIDE_GUARD = 40     # a 32-wide tile row of the transposing kernels and more


@pytest.mark.parametrize("dname", ["c128", "c64"])
def test_zip_unzip_transposed(dname):
    dt = DT[dname]
    R = pr.real_type(dt)
    for nt, m in ZIP_T_SHAPES:
        k, j = np.arange(nt)[:, None], np.arange(m)[None, :]
        re = (1000.0 * k + j).astype(R)                     # (nt, m)
        z = (re + 1j * (7.0 + 3.0 * k + 100.0 * j)).astype(dt)
        msg = f"{dname} nt={nt} m={m}"
        src = Placed(z, 0, guard=WIDE_GUARD)
        dst = Placed(np.full(m * nt, 5, dtype=R), 0, guard=WIDE_GUARD)
        kernels.unzip(dst.tensor.view(m, nt), src.tensor.view(nt, m),
                      transposed=True)
        check(dst, np.ascontiguousarray(re.T).ravel(), "unzip_t " + msg)
        assert src.untouched(), msg
        src = Placed(np.ascontiguousarray(re.T), 0, guard=WIDE_GUARD)
        dst = Placed(np.full(nt * m, 5 + 5j, dtype=dt), 0, guard=WIDE_GUARD)
        kernels.zip(dst.tensor.view(nt, m), src.tensor.view(m, nt),
                    transposed=True)
        check(dst, re.astype(dt).ravel(), "zip_t " + msg)   # imag: exact 0
        assert src.untouched(), msg


def zip_pair(dname, n, od, os_, unzip):
    """One plain zip / unzip launch -> (dst, src, expected dst)."""
    dt = DT[dname]
    R = pr.real_type(dt)
    z = ew_data(dname, n, 0)
    if unzip:
        src, dst = Placed(z, os_), Placed(np.full(n, 5, dtype=R), od)
        want = np.ascontiguousarray(z.real)
    else:
        src = Placed(np.ascontiguousarray(z.real), os_)
        dst = Placed(np.full(n, 5 + 5j, dtype=dt), od)
        want = z.real.astype(dt)
    if src.tensor is not None and dst.tensor is not None:
        (kernels.unzip if unzip else kernels.zip)(dst.tensor, src.tensor)
    else:       # complex128 one real off alignment
        lib = _ffi.lib()
        rc = (lib.pam_unzip if unzip else lib.pam_zip)(
            stream(), dst.ptr, src.ptr, n, _ffi.C128)
        assert rc == 0
    return dst, src, want


@pytest.mark.parametrize("dname", ["c128", "c64"])
def test_zip_unzip_offsets(dname):
    for n in (0, 1, 3, 5, 257, 1027):
        for od, os_ in ((0, 0), (1, 0), (0, 1), (1, 1)):
            for unzip in (True, False):
                msg = f"{'un' * unzip}zip {dname} n={n} offs={od}{os_}"
                dst, src, want = zip_pair(dname, n, od, os_, unzip)
                check(dst, want, msg)
                assert src.untouched(), msg
                assert n or dst.untouched(), msg


# ------------------------------------------------------------ the grid cap
def run_capped():
    """add, axpy, the complex product, the soft threshold, zip and unzip
    at n = 4099 with operands at offsets 0 and 1, float64 and float32 (and
    their complex types), bit for bit against primref -> list of failures.
    Meant for a process started with PAM_EW_CAP=3: three blocks, so every
    lane takes several passes of the stride loop and the scalar tail starts
    at a later pass."""
    n, bad = 4099, []
    alpha_t = dev64(A64)
    rng = np.random.default_rng(10)
    for dname, cname in (("f64", "c128"), ("f32", "c64")):
        for off in (0, 1):
            for dn in (dname, cname):
                host = {r: ew_data(dn, n, s) for s, r in enumerate("yab")}
                for case in (("add", "yab", ()), ("axpy", "ya", (ALPHA,)),
                             ("axpy_d", "ya", (alpha_t, -1.0)),
                             ("mul", "yab", ())):
                    placed = {r: Placed(host[r], off) for r in "yab"}
                    try:
                        run_ew_case(case, host, placed, f"{dn} off={off}")
                    except AssertionError as e:
                        bad.append(str(e))
            x0 = pr.thresh_data(rng, DT[dname], n, 0, THRESH)
            y = Placed(x0, off)
            ew("thresh", y, [y], 0, THRESH)
            if not (y.guards_intact() and pr.same(y.value(),
                                                  pr.soft(x0, THRESH))):
                bad.append(f"thresh {dname} off={off}")
            for unzip in (True, False):
                dst, src, want = zip_pair(cname, n, off, off, unzip)
                if not (dst.guards_intact() and src.untouched()
                        and pr.same(dst.value(), want)):
                    bad.append(f"zip unzip={unzip} {cname} off={off}")
    return bad


CHILD = """
import sys
sys.path[:0] = [{tests!r}, {root!r}]
import test_gpu_primitives as t
bad = t.run_capped()
print("\\n".join(bad))
sys.exit(1 if bad else 0)
"""


def test_stride_loop_under_grid_cap():
    """PAM_EW_CAP is read once per process, so the capped launches run in
    a fresh child process."""
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PAM_EW_CAP="3")
    r = subprocess.run(
        [sys.executable, "-c",
         CHILD.format(tests=tests, root=os.path.dirname(tests))],
        env=env, timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:],
                               r.stderr[-2000:])

"""Kernel-by-kernel tests of the matrix-core family in csrc/gemm.hip and
csrc/gemm256.hip — pam_gemm, pam_gemm_batched, pam_cgemm_batched,
pam_gemm_kt, pam_transpose, pam_ctranspose — each called through the C-ABI
with raw pointers, against the NumPy references of tests/gemmref.py (itself
checked in tests/test_gemmref_cpu.py).

Every operand sits inside a larger buffer (gemmref.Placed2D) with a leading
dimension or batch stride that is dense or padded, at a 16-byte aligned
start or one element off it.  Padding and guards of an input are NaN, of an
output primref.SENTINEL; an output without accumulate starts as NaN, so an
entry that was not stored, or was added to, shows.  Every case checks the
value, that guards and padding of the output hold the sentinel bit for bit,
that the inputs hold their uploaded bits, and that the result has no NaN.

Values.  Integer data (parts in [-4, 4], row and column trends) are
compared for equality with an int64 matmul: every partial sum is exact in
float32 and float64, so one dropped, doubled or misplaced term fails
wherever it is.  Random normals (B with the column trend 1e-3 * n) are held
to the forward bound of any summation order, (K + 1) u (|A| @ |B| + |C0|),
complex (2K + 2) u ((|Ar| + |Ai|) @ (|Br| + |Bi|) + |C0r| + |C0i|) per
part, against an np.longdouble product.  The bound is not widened for any
dtype.

Variants reached (template arguments), all for T = double and float:
  gemm_kernel<T, ACC, GUARD>: all four, dense and with lda/ldb/ldc padded
  gemm_batched_kernel<T, NPL, CT, ACC, BK>, NPL values per element:
    real <T, 1, CT, ACC, 16>: all four
    complex <T, 2, CT, false, 8> for K <= 64, <T, 2, CT, false, 16> above,
    <T, 2, CT, true, 16>; in child processes BK 8 above K = 64 and BK 16
    below (PAM_CGEMM_BK=8 / 16)
  gemm256_f32_kernel<ACC>: both, 1, 2, 3 and 16 panels
  transpose_kernel<T, NV, CONJ>: <T, 1, false>, <T, 2, false>, <T, 2, true>

Worst err / bound seen on an MI355X, per entry point (RATIO collects them,
WORST the case; the environment-selected variants stay below the same
figures):
  pam_gemm           f64 0.362 (513x5x3)    f32 0.383 (513x5x3)
  pam_gemm_batched   f64 0.385 (3x63x7x65)  f32 0.381 (3x63x7x65)
  pam_cgemm_batched  c128 0.107 (3x63x7x65) c64 0.089 (3x63x7x65)
  pam_gemm_kt        f32 0.119 (256x32x256)
The bound grows with K and the error with about its root, so the small K
come closest; at K >= 64 every ratio is below 0.12."""
import os
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest
import torch

import gemmref as gr
import primref as pr
from gemmref import Placed2D
from pylops_mpi_amd import _ffi

pytestmark = pytest.mark.gpu

DT = pr.DTYPES
NAMES = list(DT)
CODE = {"f64": _ffi.F64, "f32": _ffi.F32, "c128": _ffi.C128, "c64": _ffi.C64}
NAN = float("nan")
PAM_EARG, PAM_EDTYPE = -1, -2
RATIO = {}              # (entry point, dtype) -> worst err / bound seen
WORST = {}              # ... and the case that gave it


def stream():
    return torch.cuda.current_stream().cuda_stream


def call(name, *args):
    return getattr(_ffi.lib(), name)(stream(), *args)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@lru_cache(maxsize=None)
def operands(kind, dname, batch, M, K, N, opa):
    """A [batch, M, K] ([batch, K, M] with opa), B [batch, K, N] and C0
    [batch, M, N]: integers of gemmref.int_operand ("int") or standard
    normals, B with a column trend ("rand").  Shared and read-only."""
    dt = DT[dname]
    rng = np.random.default_rng([kind == "rand", NAMES.index(dname), batch,
                                 M, K, N, opa])
    shapes = ((batch, K, M) if opa else (batch, M, K), (batch, K, N),
              (batch, M, N))
    if kind == "int":
        return frozen(*(gr.int_operand(rng, s, dt) for s in shapes))
    out = []
    for s in shapes:
        x = rng.standard_normal(s)
        if pr.is_complex(dt):
            x = x + 1j * rng.standard_normal(s)
        out.append(x)
    out[1] = out[1] + np.arange(N)[None, None, :] * 1e-3
    return frozen(*(x.astype(dt) for x in out))


@lru_cache(maxsize=None)
def rand_product(dname, batch, M, K, N, opa, share):
    A, B, _ = operands("rand", dname, batch, M, K, N, opa)
    return gr.product(A[:1] if share == "A" else A,
                      B[:1] if share == "B" else B, opa)


def expected(kind, dname, batch, M, K, N, opa, acc, share=""):
    """The int64 result, or (ref, bound); ``share``: "A" or "B" when the
    first matrix of that stack serves every batch."""
    A, B, C0 = operands(kind, dname, batch, M, K, N, opa)
    c0 = C0 if acc else None
    if kind == "int":
        return gr.int_gemm(A[:1] if share == "A" else A,
                           B[:1] if share == "B" else B, c0, opa)
    ref, mag = rand_product(dname, batch, M, K, N, opa, share)
    return gr.finish(ref, mag, K, DT[dname], c0)


def verify(tag, entry, dname, kind, rc, pc, ins, want, fails):
    """The four checks of one case; failures are appended to ``fails``."""
    if rc != 0:
        fails.append(f"{tag}: returned {rc}")
        return
    full = pc.fetch()
    got = pc.value(full)
    if not pc.guards_intact(full):
        fails.append(f"{tag}: guard or padding of C overwritten")
    for name, p in ins:
        if not p.untouched():
            fails.append(f"{tag}: input {name} written")
    nan = int(np.isnan(pr.rview(got.reshape(-1))).sum())
    if nan:
        fails.append(f"{tag}: {nan} NaN in the result")
    if kind == "int":
        want = want.reshape(got.shape)
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            i = tuple(int(v) for v in bad[0])
            fails.append(f"{tag}: {len(bad)} of {got.size} entries differ, "
                         f"first at {i}: got {got[i]}, want {want[i]}")
    else:
        ref, bound = want
        r = gr.err_ratio(got, ref.reshape(got.shape),
                         bound.reshape(got.shape))
        key = (entry, dname)
        if not r <= RATIO.setdefault(key, 0.0):     # also records a NaN
            RATIO[key], WORST[key] = r, tag
        if not r <= 1.0:
            fails.append(f"{tag}: err / bound = {r}")


def output(C0, acc):
    """What C holds before the launch: C0, or NaN in every part."""
    if acc:
        return C0
    out = np.empty(C0.shape, dtype=C0.dtype)
    pr.rview(out.reshape(-1))[...] = NAN
    return out


def report(fails):
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:25])


# ------------------------------------------------------------------ pam_gemm
def gemm_case(dname, M, K, N, acc, pad, off, kind, fails):
    A, B, C0 = operands(kind, dname, 1, M, K, N, False)
    lda, ldb, ldc = (K + 3, N + 5, N + 1) if pad else (K, N, N)
    pa = Placed2D(A[0], lda, off=off, fill=NAN)
    pb = Placed2D(B[0], ldb, off=off, fill=NAN)
    pc = Placed2D(output(C0[0], acc), ldc, off=off)
    rc = call("pam_gemm", pa.ptr, pb.ptr, pc.ptr, M, N, K, lda, ldb, ldc,
              int(acc), CODE[dname])
    verify(f"gemm {dname} {M}x{K}x{N} acc={acc} pad={pad} off={off} {kind}",
           "pam_gemm", dname, kind, rc, pc, (("A", pa), ("B", pb)),
           expected(kind, dname, 1, M, K, N, False, acc), fails)


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("dname", ["f64", "f32"])
def test_gemm_exact(dname, acc):
    """Integer data on every shape, dense and with lda = K + 3, ldb = N + 5,
    ldc = N + 1; on GEMM_OFF_SHAPES also with every operand one element off
    16-byte alignment."""
    fails = []
    for M, K, N in gr.GEMM_SHAPES:
        for pad in (False, True):
            gemm_case(dname, M, K, N, acc, pad, 0, "int", fails)
            if (M, K, N) in gr.GEMM_OFF_SHAPES:
                gemm_case(dname, M, K, N, acc, pad, 1, "int", fails)
    report(fails)


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("dname", ["f64", "f32"])
def test_gemm_random_within_bound(dname, acc):
    fails = []
    for M, K, N in gr.GEMM_RANDOM_SHAPES:
        for pad in (False, True):
            gemm_case(dname, M, K, N, acc, pad, 0, "rand", fails)
    report(fails)
    assert RATIO[("pam_gemm", dname)] <= 1.0


# --------------------------------------- pam_gemm_batched, pam_cgemm_batched
def batched_case(dname, batch, M, K, N, opa, acc, pad, kind, fails,
                 share=""):
    """One launch of the batched entry point of ``dname``.  pad: odd gaps
    between the batches of A, B and C; share "A" / "B": one matrix for
    every batch, passed with stride 0."""
    entry = ("pam_cgemm_batched" if pr.is_complex(DT[dname])
             else "pam_gemm_batched")
    A, B, C0 = operands(kind, dname, batch, M, K, N, opa)
    gap = (7, 3, 5) if pad else (0, 0, 0)
    pa = Placed2D(A[:1] if share == "A" else A, bstride=M * K + gap[0],
                  fill=NAN)
    pb = Placed2D(B[:1] if share == "B" else B, bstride=K * N + gap[1],
                  fill=NAN)
    pc = Placed2D(output(C0, acc), bstride=M * N + gap[2])
    rc = call(entry, pa.ptr, pb.ptr, pc.ptr, batch, M, N, K,
              0 if share == "A" else pa.bstride,
              0 if share == "B" else pb.bstride, pc.bstride, int(opa),
              int(acc), CODE[dname])
    verify(f"{entry} {dname} {batch}x{M}x{K}x{N} opa={opa} acc={acc} "
           f"pad={pad} share={share!r} {kind}", entry, dname, kind, rc, pc,
           (("A", pa), ("B", pb)),
           expected(kind, dname, batch, M, K, N, opa, acc, share), fails)


SHARE_SHAPES = [(3, 63, 7, 65), (3, 129, 17, 63), (3, 64, 64, 64)]


def batched_sweep(dname, opa, acc, shapes, random_shapes):
    fails = []
    for s in shapes:
        for pad in (False, True):
            batched_case(dname, *s, opa, acc, pad, "int", fails)
        if s in random_shapes:
            batched_case(dname, *s, opa, acc, True, "rand", fails)
        if s in SHARE_SHAPES:
            batched_case(dname, *s, opa, acc, True, "int", fails, share="A")
            batched_case(dname, *s, opa, acc, False, "int", fails, share="B")
    return fails


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("opa", [False, True])
@pytest.mark.parametrize("dname", ["f64", "f32"])
def test_gemm_batched(dname, opa, acc):
    report(batched_sweep(dname, opa, acc, gr.BATCHED_SHAPES,
                         gr.BATCHED_RANDOM_SHAPES))
    assert RATIO[("pam_gemm_batched", dname)] <= 1.0


CSHAPES = gr.BATCHED_SHAPES + gr.VARIANT_SHAPES
CRANDOM = gr.BATCHED_RANDOM_SHAPES + gr.VARIANT_SHAPES[1:]


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("opa", [False, True])
@pytest.mark.parametrize("dname", ["c128", "c64"])
def test_cgemm_batched(dname, opa, acc):
    """Gaussian integers and random data.  Without accumulate K <= 64 runs
    the BK = 8 kernel and K = 65, 80 the BK = 16 one; with accumulate
    always BK = 16."""
    report(batched_sweep(dname, opa, acc, CSHAPES, CRANDOM))
    assert RATIO[("pam_cgemm_batched", dname)] <= 1.0


def run_cgemm_variants():
    """The complex cases above; the caller selects the kernel through the
    environment.  Returns the failures."""
    fails = []
    for dname in ("c128", "c64"):
        for opa in (False, True):
            for acc in (False, True):
                fails += batched_sweep(dname, opa, acc, CSHAPES, CRANDOM)
    return fails


CHILD = """
import sys
sys.path[:0] = [{tests!r}, {root!r}]
import test_gpu_gemm as t
bad = t.run_cgemm_variants()
print("\\n".join(bad[:25]))
print("worst err / bound:", t.RATIO)
sys.exit(1 if bad else 0)
"""
VARIANTS = [("PAM_CGEMM_BK", "8"), ("PAM_CGEMM_BK", "16")]


def test_cgemm_env_variants():
    """PAM_CGEMM_BK is read once per process, so each
    setting runs in a fresh child process, one after another; the first
    child that fails, dies or runs out of time ends the test."""
    tests = os.path.dirname(os.path.abspath(__file__))
    base = {k: v for k, v in os.environ.items()
            if not k.startswith("PAM_CGEMM_")}
    for key, val in VARIANTS:
        r = subprocess.run(
            [sys.executable, "-c",
             CHILD.format(tests=tests, root=os.path.dirname(tests))],
            env=dict(base, **{key: val}), timeout=180, capture_output=True,
            text=True)
        print(f"{key}={val}: {r.stdout[-300:]}")
        assert r.returncode == 0, (key, val, r.returncode, r.stdout[-3000:],
                                   r.stderr[-2000:])


# --------------------------------------------------------------- pam_gemm_kt
def kt_case(M, K, N, acc, kind, fails):
    A, B, C0 = operands(kind, "f32", 1, M, K, N, False)
    pat = Placed2D(np.ascontiguousarray(A[0].T), fill=NAN)  # host transpose
    pb = Placed2D(B[0], fill=NAN)
    pc = Placed2D(output(C0[0], acc))
    rc = call("pam_gemm_kt", pat.ptr, pb.ptr, pc.ptr, M, N, K, int(acc),
              _ffi.F32)
    verify(f"gemm_kt {M}x{K}x{N} acc={acc} {kind}", "pam_gemm_kt", "f32",
           kind, rc, pc, (("At", pat), ("B", pb)),
           expected(kind, "f32", 1, M, K, N, False, acc), fails)


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("M,K,N", gr.KT_SHAPES)
def test_gemm_kt(M, K, N, acc):
    """One panel (no prefetch is issued), two, three and sixteen: exact on
    integers, within the bound on random data."""
    fails = []
    kt_case(M, K, N, acc, "int", fails)
    kt_case(M, K, N, acc, "rand", fails)
    report(fails)
    assert RATIO[("pam_gemm_kt", "f32")] <= 1.0


def test_gemm_kt_refusals():
    """Each unmet precondition returns PAM_EARG, launches nothing and
    leaves C as it was.  All buffers have the full size of the shape that
    is passed (K = 31 and K = 0: of K = 32), so even a launch would stay
    inside them."""
    rng = np.random.default_rng(11)
    cases = [("M % 256", (384, 32, 256), None, (0, 0, 0)),
             ("N % 256", (256, 32, 384), None, (0, 0, 0)),
             ("K = 31", (256, 32, 256), 31, (0, 0, 0)),
             ("K = 0", (256, 32, 256), 0, (0, 0, 0)),
             ("At 4 bytes off", (256, 32, 256), None, (1, 0, 0)),
             ("B 4 bytes off", (256, 32, 256), None, (0, 1, 0)),
             ("C 4 bytes off", (256, 32, 256), None, (0, 0, 1))]
    for what, (M, K, N), kpass, offs in cases:
        At = gr.int_operand(rng, (K, M), np.float32)
        B = gr.int_operand(rng, (K, N), np.float32)
        pat = Placed2D(At, off=offs[0], fill=NAN)
        pb = Placed2D(B, off=offs[1], fill=NAN)
        pc = Placed2D(np.full((M, N), pr.SENTINEL, np.float32), off=offs[2])
        for acc in (0, 1):
            rc = call("pam_gemm_kt", pat.ptr, pb.ptr, pc.ptr, M, N,
                      K if kpass is None else kpass, acc, _ffi.F32)
            assert rc == PAM_EARG, (what, acc, rc)
        assert pc.untouched(), what
    assert call("pam_gemm_kt", pat.ptr, pb.ptr, pc.ptr, 256, 256, 32, 0,
                _ffi.F64) == PAM_EDTYPE
    assert pc.untouched()


# --------------------------------------------- pam_transpose, pam_ctranspose
T_SHAPES = [(1, 1), (1, 33), (31, 1), (31, 32), (32, 31), (32, 32), (32, 33),
            (33, 65), (65, 31), (65, 65), (1, 257), (257, 1)]


@pytest.mark.parametrize("dname", NAMES)
def test_transpose_bit_for_bit(dname):
    """At = A^T (complex: A^T or A^H) bit for bit, destination guards
    intact, source untouched; both operands aligned and one element off."""
    dt = DT[dname]
    cplx = pr.is_complex(dt)
    rng = np.random.default_rng([12, NAMES.index(dname)])
    fails = []
    for nr, nc in T_SHAPES:
        A = rng.standard_normal((nr, nc))
        if cplx:
            A = A + 1j * rng.standard_normal((nr, nc))
        A = A.astype(dt)
        if A.size >= 3:
            A.flat[1] = 0.0             # conj must give -0 in the imaginary
        for off in (0, 1):
            for conj in ((0, 1) if cplx else (None,)):
                src = Placed2D(A, off=off, fill=NAN)
                dst = Placed2D(output(np.empty((nc, nr), dt), False),
                               off=off)
                if cplx:
                    rc = call("pam_ctranspose", src.ptr, dst.ptr, nr, nc,
                              conj, CODE[dname])
                    want = pr.conj(A.T) if conj else A.T
                else:
                    rc = call("pam_transpose", src.ptr, dst.ptr, nr, nc,
                              CODE[dname])
                    want = A.T
                tag = f"{dname} {nr}x{nc} off={off} conj={conj}"
                full = dst.fetch()
                got = dst.value(full)
                if rc != 0:
                    fails.append(f"{tag}: returned {rc}")
                if not dst.guards_intact(full):
                    fails.append(f"{tag}: destination guard overwritten")
                if not src.untouched():
                    fails.append(f"{tag}: source written")
                if not np.array_equal(pr.bits(got.reshape(-1)),
                                      pr.bits(np.ascontiguousarray(
                                          want).reshape(-1))):
                    fails.append(f"{tag}: bits differ")
    report(fails)


# ------------------------------------------------------------ argument errors
def refused(entry, good, changes, pc):
    """Each (what, {position: value}, code) replaces arguments of the valid
    call ``good``; the entry point must return ``code`` and leave the
    SENTINEL-filled C bit-identical."""
    for what, change, code in changes:
        args = list(good)
        for i, v in change.items():
            args[i] = v
        rc = call(entry, *args)
        assert rc == code, (entry, what, rc)
        assert pc.untouched(), (entry, what)


def small(dname, *shape):
    return gr.int_operand(np.random.default_rng(13), shape, DT[dname])


def sentinel(dname, *shape):
    out = np.empty(shape, dtype=DT[dname])
    pr.rview(out.reshape(-1))[...] = pr.SENTINEL
    return out


@pytest.mark.parametrize("dname", ["f64", "f32"])
def test_gemm_argument_errors(dname):
    M, K, N = 4, 3, 5
    pa = Placed2D(small(dname, M, K), K + 1, fill=NAN)
    pb = Placed2D(small(dname, K, N), N + 1, fill=NAN)
    pc = Placed2D(sentinel(dname, M, N), N + 1)
    good = [pa.ptr, pb.ptr, pc.ptr, M, N, K, K + 1, N + 1, N + 1, 0,
            CODE[dname]]
    for acc in (0, 1):
        good[9] = acc
        refused("pam_gemm", good, [
            ("M = 0", {3: 0}, PAM_EARG), ("M < 0", {3: -1}, PAM_EARG),
            ("N = 0", {4: 0}, PAM_EARG), ("N < 0", {4: -1}, PAM_EARG),
            ("K < 0", {5: -1}, PAM_EARG),
            ("A NULL", {0: None}, PAM_EARG), ("B NULL", {1: None}, PAM_EARG),
            ("C NULL", {2: None}, PAM_EARG),
            ("lda < K", {6: K - 1}, PAM_EARG),
            ("ldb < N", {7: N - 1}, PAM_EARG),
            ("ldc < N", {8: N - 1}, PAM_EARG),
            ("lda = 0", {6: 0}, PAM_EARG),
            ("complex128", {10: _ffi.C128}, PAM_EDTYPE),
            ("complex64", {10: _ffi.C64}, PAM_EDTYPE),
            ("dtype 4", {10: 4}, PAM_EDTYPE),
            ("dtype -1", {10: -1}, PAM_EDTYPE)], pc)
    # the smallest leading dimensions are accepted
    pa, pb = Placed2D(small(dname, M, K), fill=NAN), Placed2D(
        small(dname, K, N), fill=NAN)
    assert call("pam_gemm", pa.ptr, pb.ptr, pc.ptr, M, N, K, K, N, N, 0,
                CODE[dname]) == 0
    assert not pc.untouched()


@pytest.mark.parametrize("dname", NAMES)
def test_batched_argument_errors(dname):
    cplx = pr.is_complex(DT[dname])
    entry = "pam_cgemm_batched" if cplx else "pam_gemm_batched"
    batch, M, K, N = 2, 4, 3, 5
    pa = Placed2D(small(dname, batch, M, K), fill=NAN)
    pb = Placed2D(small(dname, batch, K, N), fill=NAN)
    pc = Placed2D(sentinel(dname, batch, M, N))
    wrong = (_ffi.F64, _ffi.F32) if cplx else (_ffi.C128, _ffi.C64)
    for opa in (0, 1):
        for acc in (0, 1):
            good = [pa.ptr, pb.ptr, pc.ptr, batch, M, N, K, M * K, K * N,
                    M * N, opa, acc, CODE[dname]]
            refused(entry, good, [
                ("batch = 0", {3: 0}, PAM_EARG),
                ("batch < 0", {3: -1}, PAM_EARG),
                ("M = 0", {4: 0}, PAM_EARG), ("M < 0", {4: -1}, PAM_EARG),
                ("N = 0", {5: 0}, PAM_EARG), ("N < 0", {5: -1}, PAM_EARG),
                ("K < 0", {6: -1}, PAM_EARG),
                ("A NULL", {0: None}, PAM_EARG),
                ("B NULL", {1: None}, PAM_EARG),
                ("C NULL", {2: None}, PAM_EARG),
                ("other family", {12: wrong[0]}, PAM_EDTYPE),
                ("other family", {12: wrong[1]}, PAM_EDTYPE),
                ("dtype 4", {12: 4}, PAM_EDTYPE),
                ("dtype -1", {12: -1}, PAM_EDTYPE)], pc)


def test_gemm_kt_argument_errors():
    M, K, N = 256, 32, 256
    pat = Placed2D(small("f32", K, M), fill=NAN)
    pb = Placed2D(small("f32", K, N), fill=NAN)
    pc = Placed2D(sentinel("f32", M, N))
    for acc in (0, 1):
        good = [pat.ptr, pb.ptr, pc.ptr, M, N, K, acc, _ffi.F32]
        refused("pam_gemm_kt", good, [
            ("M = 0", {3: 0}, PAM_EARG), ("M < 0", {3: -256}, PAM_EARG),
            ("N = 0", {4: 0}, PAM_EARG), ("N < 0", {4: -256}, PAM_EARG),
            ("K < 0", {5: -32}, PAM_EARG),
            ("At NULL", {0: None}, PAM_EARG), ("B NULL", {1: None}, PAM_EARG),
            ("C NULL", {2: None}, PAM_EARG),
            ("float64", {7: _ffi.F64}, PAM_EDTYPE),
            ("complex64", {7: _ffi.C64}, PAM_EDTYPE),
            ("dtype 4", {7: 4}, PAM_EDTYPE)], pc)


@pytest.mark.parametrize("dname", NAMES)
def test_transpose_argument_errors(dname):
    cplx = pr.is_complex(DT[dname])
    nr, nc = 3, 5
    src = Placed2D(small(dname, nr, nc), fill=NAN)
    dst = Placed2D(sentinel(dname, nc, nr))
    wrong = (_ffi.F64, _ffi.F32) if cplx else (_ffi.C128, _ffi.C64)
    d = 5 if cplx else 4                    # position of the dtype code
    goods = ([[src.ptr, dst.ptr, nr, nc, c, CODE[dname]] for c in (0, 1)]
             if cplx else [[src.ptr, dst.ptr, nr, nc, CODE[dname]]])
    for good in goods:
        refused("pam_ctranspose" if cplx else "pam_transpose", good, [
            ("nr = 0", {2: 0}, PAM_EARG), ("nr < 0", {2: -1}, PAM_EARG),
            ("nc = 0", {3: 0}, PAM_EARG), ("nc < 0", {3: -1}, PAM_EARG),
            ("A NULL", {0: None}, PAM_EARG),
            ("At NULL", {1: None}, PAM_EARG),
            ("other family", {d: wrong[0]}, PAM_EDTYPE),
            ("other family", {d: wrong[1]}, PAM_EDTYPE),
            ("dtype 4", {d: 4}, PAM_EDTYPE),
            ("dtype -1", {d: -1}, PAM_EDTYPE)], dst)

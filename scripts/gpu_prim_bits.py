"""Bit-identity probe of the vector primitives (run on the GPU box): a fixed
case list over every primitive entry point of csrc/pam.hip, one line
``<sha256 of the output bytes>  <case>`` per case and a closing count.
Two builds compute the same bits iff their outputs of this script are equal
line for line; ``--lib`` loads another build's libpam.so instead of the
tree's.  Reductions and GEMV hash their result words, element-wise kernels
the whole output buffer with its sentinel guards.

Operands are float64 / float32 storage (complex: interleaved), 16-byte
aligned (off=0) or one real element past that (off=1)."""
import argparse
import hashlib
import os
import sys
from functools import lru_cache

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pylops_mpi_amd import _ffi  # noqa: E402

SIZES = (1, 5, 257, 1027, 262145)
GEMV_SHAPES = ((7, 5), (130, 66), (257, 1024))
ZIP_T_SHAPES = ((33, 31), (64, 96))
NAMES = ("f64", "f32", "c128", "c64")            # index = PAM dtype code
REAL = {"f64": np.float64, "f32": np.float32,
        "c128": np.float64, "c64": np.float32}
E = {"f64": 1, "f32": 1, "c128": 2, "c64": 2}    # reals per element
GUARD = 8
SENTINEL = -8191.5
NCASES = 0


@lru_cache(maxsize=None)
def host(dname, nreal, k):
    rng = np.random.default_rng([k, nreal])
    return rng.standard_normal(nreal).astype(REAL[dname])


class Buf:
    """nreal reals between sentinel guards; k: the seed of its data (None:
    sentinel everywhere, an output)."""

    def __init__(self, dname, nreal, off, k=None):
        full = np.full(nreal + 2 * GUARD + 1, SENTINEL, REAL[dname])
        lo = GUARD + off
        if k is not None:
            full[lo:lo + nreal] = host(dname, nreal, k)
        self.t = torch.from_numpy(full).cuda()
        self.ptr = self.t.data_ptr() + lo * self.t.element_size()
        assert (self.ptr % 16 == 0) == (off == 0)

    def bytes(self):
        return self.t.cpu().numpy().tobytes()


def stream():
    return torch.cuda.current_stream().cuda_stream


def emit(case, rc, *outs):
    global NCASES
    assert rc == 0, (case, rc)
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for o in outs:
        h.update(o.bytes() if isinstance(o, Buf)
                 else o.cpu().numpy().tobytes())
    print(f"{h.hexdigest()}  {case}", flush=True)
    NCASES += 1


def dev64(n):
    return torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")


def elementwise(lib):
    alpha = torch.tensor([0.7 / 3.0, 0.0], dtype=torch.float64, device="cuda")
    for code, d in enumerate(NAMES[:2]):
        for n in SIZES:
            for off in (0, 1):
                s, tag = stream(), f"{d} n={n} off={off}"
                a, b = Buf(d, n, off, 1), Buf(d, n, off, 2)
                y = Buf(d, n, off)
                emit(f"fill {tag}", lib.pam_fill(s, y.ptr, n, 0.7, code), y)
                y = Buf(d, n, off)
                emit(f"neg {tag}", lib.pam_neg(s, y.ptr, a.ptr, n, code), y)
                for name in ("add", "sub", "mul"):
                    y = Buf(d, n, off)
                    emit(f"{name} {tag}", getattr(lib, "pam_" + name)(
                        s, y.ptr, a.ptr, b.ptr, n, code), y)
                y = Buf(d, n, off)
                emit(f"scale {tag}",
                     lib.pam_scale(s, y.ptr, a.ptr, 0.7, n, code), y)
                for name in ("axpy", "xpby"):
                    y = Buf(d, n, off, 3)
                    emit(f"{name} {tag}", getattr(lib, "pam_" + name)(
                        s, y.ptr, a.ptr, -0.7, n, code), y)
                    y = Buf(d, n, off, 3)
                    emit(f"{name}_d {tag}", getattr(lib, f"pam_{name}_d")(
                        s, y.ptr, a.ptr, alpha.data_ptr(), -1.0, n, code), y)
    out = dev64(2)
    num = torch.tensor([3.7, 0.0], dtype=torch.float64, device="cuda")
    den = torch.tensor([-1.3, 0.9], dtype=torch.float64, device="cuda")
    emit("scalar_alpha", lib.pam_scalar_alpha(
        stream(), out.data_ptr(), num.data_ptr(), den.data_ptr(), 0.3), out)
    out = dev64(2)
    emit("scalar_div", lib.pam_scalar_div(
        stream(), out.data_ptr(), num.data_ptr(), den.data_ptr()), out)


def complex_ops(lib):
    for d in NAMES[2:]:
        code = NAMES.index(d)
        for n in SIZES:
            for off in (0, 1):
                s, tag = stream(), f"{d} n={n} off={off}"
                a, b = Buf(d, 2 * n, off, 1), Buf(d, 2 * n, off, 2)
                y = Buf(d, 2 * n, off)
                emit(f"cmul {tag}",
                     lib.pam_cmul(s, y.ptr, a.ptr, b.ptr, n, code), y)
                y = Buf(d, 2 * n, off)
                emit(f"cscale {tag}",
                     lib.pam_cscale(s, y.ptr, a.ptr, 0.7, -1.3, n, code), y)
                y = Buf(d, 2 * n, off)
                emit(f"conj {tag}", lib.pam_conj(s, y.ptr, a.ptr, n, code), y)
                y = Buf(d, n, off)
                emit(f"unzip {tag}",
                     lib.pam_unzip(s, y.ptr, a.ptr, n, code), y)
                r, y = Buf(d, n, off, 4), Buf(d, 2 * n, off)
                emit(f"zip {tag}", lib.pam_zip(s, y.ptr, r.ptr, n, code), y)
        for nt, m in ZIP_T_SHAPES:
            for off in (0, 1):
                s, tag = stream(), f"{d} nt={nt} m={m} off={off}"
                a, y = Buf(d, 2 * nt * m, off, 1), Buf(d, nt * m, off)
                emit(f"unzip_t {tag}",
                     lib.pam_unzip_t(s, y.ptr, a.ptr, nt, m, code), y)
                r, y = Buf(d, nt * m, off, 4), Buf(d, 2 * nt * m, off)
                emit(f"zip_t {tag}",
                     lib.pam_zip_t(s, y.ptr, r.ptr, nt, m, code), y)


def thresholds(lib):
    for code, d in enumerate(NAMES):
        for n in SIZES:
            for off in (0, 1):
                x = Buf(d, E[d] * n, off, 1)
                for kind in (0, 1, 2):
                    y = Buf(d, E[d] * n, off)
                    emit(f"thresh kind={kind} {d} n={n} off={off}",
                         lib.pam_thresh(stream(), y.ptr, x.ptr, n, kind, 0.7,
                                        code), y)


def reductions(lib):
    ws = torch.empty(2 * int(lib.pam_reduce_ws_elems()), dtype=torch.float64,
                     device="cuda")
    for code, d in enumerate(NAMES):
        for n in SIZES:
            for off in (0, 1):
                s, tag = stream(), f"{d} n={n} off={off}"
                x, y = Buf(d, E[d] * n, off, 1), Buf(d, E[d] * n, off, 2)
                if E[d] == 1:
                    out = dev64(3)
                    emit(f"dot {tag}", lib.pam_dot(
                        s, x.ptr, y.ptr, n, ws.data_ptr(), out.data_ptr(),
                        code), out)
                else:
                    for conjx in (0, 1):
                        out = dev64(3)
                        emit(f"cdot conjx={conjx} {tag}", lib.pam_cdot(
                            s, x.ptr, y.ptr, n, conjx, ws.data_ptr(),
                            out.data_ptr(), code), out)
                for op, p in ((0, 2.0), (0, 1.0), (0, 3.0), (1, 0.0),
                              (2, 0.0), (3, 0.0)):
                    out = dev64(3)
                    emit(f"norm_local op={op} p={p} {tag}",
                         lib.pam_norm_local(s, x.ptr, n, op, p, ws.data_ptr(),
                                            out.data_ptr(), code), out)


def groups(lib):
    ws = torch.empty(int(lib.pam_reduce_ws_elems()), dtype=torch.float64,
                     device="cuda")
    for code, d in enumerate(NAMES):
        for n in SIZES:
            for off in (0, 1):
                a = [Buf(d, E[d] * n, off, 10 + c) for c in range(4)]
                b = [Buf(d, E[d] * n, off, 20 + c) for c in range(4)]
                for nc in (1, 2, 3, 4):
                    tag = f"ncomp={nc} {d} n={n} off={off}"
                    pad = [None] * (4 - nc)
                    ap = [p.ptr for p in a[:nc]] + pad
                    out = dev64(3)
                    emit(f"group_norm {tag}", lib.pam_group_norm(
                        stream(), nc, *ap, n, ws.data_ptr(), out.data_ptr(),
                        code), out)
                    for shift in (0, 1):
                        bp = ([p.ptr for p in b[:nc]] + pad if shift
                              else [None] * 4)
                        for mode in (0, 1):
                            y = [Buf(d, E[d] * n, off) for _ in range(nc)]
                            yp = [p.ptr for p in y] + pad
                            emit(f"group_shrink shift={shift} mode={mode} "
                                 f"{tag}", lib.pam_group_shrink(
                                     stream(), mode, nc, *yp, *ap, *bp, -0.6,
                                     n, 0.9, code), *y)


def gemv(lib):
    for code, d in enumerate(NAMES[:2]):
        for nr, nc in GEMV_SHAPES:
            ws = torch.empty(int(lib.pam_gemv_ws_elems(nr, nc)),
                             dtype=torch.float64, device="cuda")
            for off in (0, 1):
                A = Buf(d, nr * nc, off, 1)
                for trans in (0, 1):
                    nin, nout = (nr, nc) if trans else (nc, nr)
                    x, y = Buf(d, nin, off, 2), Buf(d, nout, off)
                    emit(f"gemv trans={trans} {d} ({nr},{nc}) off={off}",
                         lib.pam_gemv(stream(), trans, A.ptr, x.ptr, y.ptr,
                                      nr, nc, ws.data_ptr(), code), y)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", help="libpam.so to load instead of the tree's")
    args = ap.parse_args()
    if args.lib:
        _ffi._LIB_PATH = os.path.abspath(args.lib)
    lib = _ffi.lib()
    torch.cuda.set_device(0)
    for family in (elementwise, complex_ops, thresholds, reductions, groups,
                   gemv):
        family(lib)
    print(f"cases: {NCASES}", flush=True)


if __name__ == "__main__":
    main()

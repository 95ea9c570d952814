"""Kernel perf probe (run on the GPU box): GEMM TF/s, GEMV GB/s and the
vector primitives (HBM-bound rows in TB/s by the algorithmic byte count,
launch-bound rows in host microseconds per call).  Prints one JSON line per
measurement.  --rows picks the families, --lib another build's libpam.so
(for A/Bs against this tree's)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pylops_mpi_amd import _ffi  # noqa: E402
from pylops_mpi_amd.comm import init_default_comm  # noqa: E402


def timeit(fn, iters=10, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def bench_gemm(M, K, N, tdt, label):
    # random data (guide §5.4 rule 25: never zero-filled operands)
    A = torch.rand((M, K), dtype=tdt, device="cuda") * 2 - 1
    B = torch.rand((K, N), dtype=tdt, device="cuda") * 2 - 1
    C = torch.empty((M, N), dtype=tdt, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    dt = _ffi.dtype_code(tdt)

    def run():
        _ffi.checked(_ffi.lib().pam_gemm(
            s, A.data_ptr(), B.data_ptr(), C.data_ptr(), M, N, K, K, N, N,
            0, dt), "gemm")

    sec = timeit(run)
    tf = 2.0 * M * N * K / sec / 1e12
    print(json.dumps({"probe": label, "M": M, "K": K, "N": N,
                      "ms": sec * 1e3, "TF": tf}), flush=True)


def bench_gemv(n, label):
    A = torch.rand((n, n), dtype=torch.float64, device="cuda")
    x = torch.rand(n, dtype=torch.float64, device="cuda")
    y = torch.empty(n, dtype=torch.float64, device="cuda")
    ws = torch.empty(int(_ffi.lib().pam_gemv_ws_elems(n, n)),
                     dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for trans in (0, 1):
        def run(tr=trans):
            _ffi.checked(_ffi.lib().pam_gemv(
                s, tr, A.data_ptr(), x.data_ptr(), y.data_ptr(), n, n,
                ws.data_ptr(), 0), "gemv")
        sec = timeit(run, iters=20)
        gbs = 8.0 * n * n / sec / 1e9
        print(json.dumps({"probe": f"{label}_t{trans}", "n": n,
                          "ms": sec * 1e3, "GB/s": gbs}), flush=True)


NBENCH = 2048 * 2048 * 128      # the bench length (scripts/gpu_ew_sweep.py)


def rand(n, tdt=torch.float64):
    return torch.rand(n, dtype=tdt, device="cuda") * 2 - 1


def bench_prim(label, nbytes, call, iters=20):
    """One HBM-bound row: call() launches, nbytes is what it must move."""
    def run():
        _ffi.checked(call(), label)
    sec = timeit(run, iters=iters)
    print(json.dumps({"probe": label, "ms": sec * 1e3,
                      "TB/s": nbytes / sec / 1e12}), flush=True)


def bench_launch(label, call, calls=1000):
    """One launch-bound row: host time per call, the queue drained after."""
    for _ in range(50):
        call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    sec = (time.perf_counter() - t0) / calls
    torch.cuda.synchronize()
    print(json.dumps({"probe": label, "calls": calls,
                      "host_us": sec * 1e6}), flush=True)


def bench_primitives():
    lib = _ffi.lib()
    s = torch.cuda.current_stream().cuda_stream
    n = NBENCH
    ws = torch.empty(2 * int(lib.pam_reduce_ws_elems()), dtype=torch.float64,
                     device="cuda")
    out = torch.empty(2, dtype=torch.float64, device="cuda")
    alpha = torch.full((1,), 0.5, dtype=torch.float64, device="cuda")
    w, o = ws.data_ptr(), out.data_ptr()

    # float64 at the bench length
    x, y, z = rand(n), rand(n), torch.empty(n, dtype=torch.float64,
                                            device="cuda")
    xp, yp, zp = x.data_ptr(), y.data_ptr(), z.data_ptr()
    bench_prim("axpy_f64", 24 * n, lambda: lib.pam_axpy(s, yp, xp, 0.5, n, 0))
    bench_prim("axpy_d_f64", 24 * n, lambda: lib.pam_axpy_d(
        s, yp, xp, alpha.data_ptr(), 1.0, n, 0))
    bench_prim("add_f64", 24 * n, lambda: lib.pam_add(s, zp, xp, yp, n, 0))
    bench_prim("thresh_soft_f64", 16 * n,
               lambda: lib.pam_thresh(s, zp, xp, n, 0, 0.3, 0))
    bench_prim("dot_f64", 16 * n, lambda: lib.pam_dot(s, xp, yp, n, w, o, 0))
    bench_prim("norm2_f64", 8 * n,
               lambda: lib.pam_norm_local(s, xp, n, 0, 2.0, w, o, 0))
    # the same storage as n complex64 (8 B each)
    x32, y32, z32 = (t.view(torch.float32) for t in (x, y, z))
    x32.copy_(rand(2 * n, torch.float32))
    y32.copy_(rand(2 * n, torch.float32))
    bench_prim("cmul_c64", 24 * n, lambda: lib.pam_cmul(s, zp, xp, yp, n, 3))
    bench_prim("cdot_c64", 16 * n,
               lambda: lib.pam_cdot(s, xp, yp, n, 1, w, o, 3))
    del x32, y32, z32
    x.copy_(rand(n))
    y.copy_(rand(n))
    # ... as 2 float64 components of n / 2: y_c = shrink(a_c + beta b_c)
    h = n // 2
    hb = 8 * h
    bench_prim("group_shrink_nc2_shift_f64", 24 * n,
               lambda: lib.pam_group_shrink(
                   s, 0, 2, zp, zp + hb, None, None, xp, xp + hb, None, None,
                   yp, yp + hb, None, None, -0.5, h, 0.3, 0))
    bench_prim("group_norm_nc2_f64", 8 * n, lambda: lib.pam_group_norm(
        s, 2, xp, xp + hb, None, None, h, w, o, 0))
    # ... as n / 2 complex128: 16 B read + 8 B written per element
    bench_prim("unzip_c128", 12 * n, lambda: lib.pam_unzip(s, zp, xp, h, 2))
    nt = 2048
    bench_prim("zip_t_c128", 12 * n,
               lambda: lib.pam_zip_t(s, zp, xp, nt, h // nt, 2))
    del x, y, z

    m = 4096
    xs, ys = rand(m), rand(m)
    bench_launch("axpy_f64_n4096", lambda: lib.pam_axpy(
        s, ys.data_ptr(), xs.data_ptr(), 0.5, m, 0))
    bench_launch("dot_f64_n4096", lambda: lib.pam_dot(
        s, xs.data_ptr(), ys.data_ptr(), m, w, o, 0))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split(".")[0])
    ap.add_argument("--rows", choices=("all", "gemm", "prim"), default="all")
    ap.add_argument("--lib", help="libpam.so to load instead of the tree's")
    args = ap.parse_args()
    if args.lib:
        _ffi._LIB_PATH = os.path.abspath(args.lib)
    init_default_comm(torch.device("cuda:0"))
    if args.rows != "gemm":
        bench_primitives()
    if args.rows == "prim":
        return
    bench_gemm(4096, 4096, 4096, torch.float32, "gemm_f32")
    bench_gemm(8192, 8192, 8192, torch.float32, "gemm_f32")
    bench_gemm(4096, 4096, 4096, torch.float64, "gemm_f64")
    bench_gemm(8192, 8192, 8192, torch.float64, "gemm_f64")
    bench_gemv(4096, "gemv_f64")
    bench_gemv(8192, "gemv_f64")


if __name__ == "__main__":
    main()

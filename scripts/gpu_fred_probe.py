"""Fredholm1-only timing at the cfg5 judged shape (batched GEMM A/Bs).
Usage: gpu_fred_probe.py [dtype], default complex64; a real dtype (float32,
float64) times pam_gemm_batched."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pylops_mpi_amd as pm  # noqa: E402
from pylops_mpi_amd.comm import init_default_comm  # noqa: E402
from pylops_mpi_amd.distributedarray import as_torch_dtype  # noqa: E402


def timeit(fn, iters=30):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters


def main():
    init_default_comm(torch.device("cuda:0"))
    g = torch.Generator(device="cuda").manual_seed(7)
    nf, ns, nr, nv = 513, 64, 256, 256
    dtype = np.dtype(sys.argv[1] if len(sys.argv) > 1 else "complex64")
    cplx = dtype.kind == "c"
    tdt = as_torch_dtype(dtype)

    def rand(shape):
        v = torch.rand(shape, generator=g, device="cuda") - 0.5
        if cplx:
            v = v + 1j * (torch.rand(shape, generator=g, device="cuda") - 0.5)
        return v.to(tdt)

    G = rand((nf, ns, nr))
    for saveGt in (False, True):
        op = pm.MPIFredholm1(G, nv, saveGt=saveGt, dtype=dtype)
        x = pm.DistributedArray((op.shape[1],),
                                partition=pm.Partition.BROADCAST,
                                dtype=dtype)
        x[:] = rand(op.shape[1])
        y = op.matvec(x)
        tm = timeit(lambda: op.matvec(x)) * 1e3
        tr = timeit(lambda: op.rmatvec(y)) * 1e3
        # real flops: 2 per MAC; 4 real mul-adds per cmac -> 8
        fl = (8.0 if cplx else 2.0) * nf * ns * nr * nv
        print(f"{dtype} saveGt={saveGt}: matvec {tm:.3f} ms "
              f"({fl/tm/1e9:.1f} TF) rmatvec {tr:.3f} ms "
              f"({fl/tr/1e9:.1f} TF)", flush=True)


if __name__ == "__main__":
    main()

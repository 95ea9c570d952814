"""Stencil launch-shape sweep at a given dims (env PAM_FD_*, DIMS, RMATVEC,
REPS).  Prints which kernel served the shape (pam_fd_variant)."""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pylops_mpi_amd as pm
from pylops_mpi_amd import kernels
from pylops_mpi_amd.comm import init_default_comm

def main():
    init_default_comm(torch.device("cuda:0"))
    dims = tuple(int(v) for v in os.environ.get("DIMS", "512x4096x256").split("x"))
    reps = int(os.environ.get("REPS", "20"))
    n = int(np.prod(dims))
    op = pm.MPIFirstDerivative(dims, kind="centered", order=3)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = pm.DistributedArray((n,))
    x[:] = torch.randn(n, generator=g, dtype=torch.float64, device="cuda")
    rmv = os.environ.get("RMATVEC") == "1"
    apply = op.rmatvec if rmv else op.matvec
    for _ in range(3):
        y = apply(x)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        y = apply(x)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t) / reps
    planes = y.local_array.view(dims[0], -1)
    variant = ("row", "roll", "band")[
        kernels.fd_variant(planes, planes, None, None, 0, dims[0])]
    env = " ".join(f"{k[7:].lower()}={os.environ[k]}" for k in sorted(os.environ)
                   if k.startswith("PAM_FD_"))
    print(f"dims={dims} {'rmv' if rmv else 'mv'} kernel={variant} [{env}]: "
          f"{dt*1e3:7.3f} ms {16*n/dt/1e12:5.2f} TB/s")

main()

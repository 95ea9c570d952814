"""Isotropic total-variation denoising of a piecewise-constant image:

    min_x 0.5 ||x - noisy||^2 + lam * || grad x ||_{2,1}

with MPIL2 (data term), MPIL21 over the components of MPIGradient (the
L2,1 group prox kernels) and the PrimalDual (Chambolle-Pock) solver — no
inner least-squares solve.  ||grad||^2 <= 8 in 2-D, hence the steps.
Run on N GPUs of one node with:

    python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
        --master-addr 127.0.0.1 examples/tv_denoise.py
"""
import os
import sys
from math import sqrt

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pylops_mpi_amd as pm
from pylops_mpi_amd.comm import init_default_comm
from pylops_mpi_amd.proximal import MPIL2, MPIL21
from pylops_mpi_amd.proximal.optimization import PrimalDual


def main():
    comm = init_default_comm()
    dims = (256, 192)
    lam = 0.3

    # every rank draws the same image and keeps its own rows
    rng = np.random.default_rng(0)
    img = np.zeros(dims)
    img[64:192, 48:144] = 1.0
    img[96:160, 80:112] = 2.0
    noisy_img = img + 0.3 * rng.standard_normal(dims)
    truth = pm.DistributedArray.to_dist(
        torch.as_tensor(img.ravel(), device=comm.device), comm)
    noisy = pm.DistributedArray.to_dist(
        torch.as_tensor(noisy_img.ravel(), device=comm.device), comm)

    Gop = pm.MPIGradient(dims, kind="forward")
    l2 = MPIL2(b=noisy)
    l21 = MPIL21(sigma=lam)
    tau = mu = 0.99 / sqrt(8.0)
    x = PrimalDual(l2, l21, Gop, noisy, tau=tau, mu=mu, theta=1.0,
                   niter=200)

    def objective(v):
        return l2(v) + l21(Gop @ v)

    err0 = (noisy - truth).norm() / truth.norm()
    err = (x - truth).norm() / truth.norm()
    f0, f = objective(noisy), objective(x)
    if comm.rank == 0:
        print(f"TV objective {f0:.4e} -> {f:.4e}; relative error "
              f"{err0:.3f} -> {err:.3f}")


if __name__ == "__main__":
    main()

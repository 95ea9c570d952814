"""Least-squares migration — the reference's tutorials/lsm.py on the
Kirchhoff kernels.

Sources are distributed over the ranks; every rank holds one
``LSMLocal`` whose ``Demop`` (KirchhoffLocal: traveltime spread, then the
wavelet) models its own shots from the BROADCAST reflectivity:

    lsm = pm.LSMLocal(z, x, t, sources, recs, v0, wav, wavc, mode="analytic")
    VStack = pm.MPIVStack(ops=[lsm.Demop])

The script models the data of a two-interface reflectivity, migrates it
(adjoint), re-models the migrated image and inverts with cgls.  Defaults
are the tutorial's: nx=81, nz=60, 11 receivers, 10 sources per rank,
nt=651, a 41-tap 20 Hz ricker (``--ntwav 41`` gives the 81 taps of the
tutorial's ``ricker(t[:41])``).

``--time`` (one GPU) prints what profiles/kirchhoff.log keeps: time per
apply and pairs per second of the spread and the gather at the tutorial's
shape and at ``--big`` (a shape that fills the chip), every choice of the
launch plan next to the automatic one, the same apply written with
torch.index_add_ / gather on the same device for scale, and whether two
runs of a maximum-collision spread gave the same bits.

    python examples/lsm.py [--nx 81 --nz 60 --nr 11 --ns 10 --nt 651]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
        --master-addr 127.0.0.1 examples/lsm.py
    python examples/lsm.py --time [--big NS NR NX NZ NT]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pylops_mpi_amd as pm
from pylops_mpi_amd import kernels
from pylops_mpi_amd.comm import init_default_comm


def geometry(args, rank, size):
    """The tutorial's model: constant velocity, receivers at depth 20,
    sources at depth 10, this rank's ns sources out of ns * size."""
    dx, dz = 4.0, 4.0
    nx, nz = args.nx, args.nz
    x, z = np.arange(nx) * dx, np.arange(nz) * dz
    edge = min(10, nx // 4)
    rx = np.linspace(edge * dx, (nx - edge) * dx, args.nr)
    recs = np.vstack((rx, 20.0 * np.ones(args.nr)))
    nstot = args.ns * size
    sxtot = np.linspace(dx * edge, (nx - edge) * dx, nstot)
    sx = sxtot[rank * args.ns:(rank + 1) * args.ns]
    sources = np.vstack((sx, 10.0 * np.ones(args.ns)))
    return z, x, sources, recs, nstot


def invert(args, comm):
    rank, size = comm.rank, comm.size
    nx, nz, nr, nt = args.nx, args.nz, args.nr, args.nt
    z, x, sources, recs, nstot = geometry(args, rank, size)
    v0 = 1000.0
    refl = np.zeros((nx, nz))
    refl[:, nz // 2] = -1.0
    refl[:, (5 * nz) // 6] = 0.5

    t = np.arange(nt) * 0.004
    wav, _, wavc = pm.ricker(t[:args.ntwav], f0=20)
    lsm = pm.LSMLocal(z, x, t, sources, recs, v0, wav, wavc, mode="analytic")
    VStack = pm.MPIVStack(ops=[lsm.Demop])
    refl_dist = pm.DistributedArray(global_shape=nx * nz,
                                    partition=pm.Partition.BROADCAST)
    refl_dist[:] = torch.as_tensor(refl.ravel(), device=comm.device)
    d_dist = VStack @ refl_dist
    d = d_dist.asarray().reshape(nstot, nr, nt)

    # adjoint, and the data modelled from the adjoint image
    madj_dist = VStack.H @ d_dist
    d_adj_dist = VStack @ madj_dist

    x0 = pm.DistributedArray(VStack.shape[1],
                             partition=pm.Partition.BROADCAST)
    x0[:] = 0
    minv_dist, _, _, _, _, cost = pm.cgls(VStack, d_dist, x0=x0,
                                          niter=args.niter, tol=0.0)
    d_inv_dist = VStack @ minv_dist

    def rel(a, b):
        return float((a - b).norm() / b.norm())

    res = rel(d_inv_dist, d_dist)
    minv = minv_dist.asarray().reshape(nx, nz)
    madj = madj_dist.asarray().reshape(nx, nz)
    if rank == 0:
        err = float(torch.linalg.norm(
            minv - torch.as_tensor(refl, device=minv.device))
            / np.linalg.norm(refl))
        print(f"lsm {nx}x{nz} image, {nstot} sources x {nr} receivers x "
              f"{nt} samples, {len(wav)}-tap ricker, {size} rank(s): "
              f"|d| {float(d.norm()):.4e}, |m_adj| {float(madj.norm()):.4e}, "
              f"|d_adj| {float(d_adj_dist.norm()):.4e}; cgls x{args.niter}: "
              f"cost {cost[0]:.4e} -> {cost[-1]:.4e}, data residual "
              f"{res:.2e}, model error {err:.3f}")
    assert cost[-1] < cost[0] and res < 0.5
    return res


# ------------------------------------------------------------------ timing
def _time_ms(fn, reps):
    beg = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return beg.elapsed_time(end) / reps


def _alternate(cases, rounds, window_ms=50.0):
    """{name: median ms} of callables timed in turn inside each round;
    each timed window holds at least 3 applies and ``window_ms``."""
    n = {}
    for k, fn in cases.items():
        fn()
        torch.cuda.synchronize()
        n[k] = max(3, int(window_ms / max(_time_ms(fn, 2), 1e-3)))
    t = {k: [] for k in cases}
    for _ in range(rounds):
        for k, fn in cases.items():
            t[k].append(_time_ms(fn, n[k]))
    return {k: float(np.median(v)) for k, v in t.items()}


ENV = ("PAM_KIRCH_WINDOW", "PAM_KIRCH_SPLIT", "PAM_KIRCH_STAGE")


def _forced(env, fn):
    def run():
        for k in ENV:
            os.environ.pop(k, None)
        os.environ.update({k: str(v) for k, v in env.items()})
        fn()
    return run


def torch_spread(m, qs, qr, nt):
    q = (qs[:, None, :] + qr[None, :, :]).reshape(-1, m.numel())
    f = torch.floor(q)
    keep = (q >= 0) & (f < nt - 1)
    it = torch.where(keep, f, torch.zeros_like(f)).long()
    w = torch.where(keep, q - f, torch.zeros_like(q))
    mk = torch.where(keep, m[None, :].expand_as(q), torch.zeros_like(q))
    idx = (it + nt * torch.arange(q.shape[0], device=q.device)[:, None])
    d = torch.zeros(q.shape[0] * nt, dtype=m.dtype, device=m.device)
    d.index_add_(0, idx.reshape(-1), (mk * (1 - w)).reshape(-1))
    d.index_add_(0, idx.reshape(-1) + 1, (mk * w).reshape(-1))
    return d


def torch_gather(d, qs, qr, nt):
    q = (qs[:, None, :] + qr[None, :, :]).reshape(-1, qs.shape[1])
    f = torch.floor(q)
    keep = (q >= 0) & (f < nt - 1)
    it = torch.where(keep, f, torch.zeros_like(f)).long()
    w = torch.where(keep, q - f, torch.zeros_like(q))
    d2 = d.reshape(-1, nt)
    term = (1 - w) * torch.gather(d2, 1, it) + w * torch.gather(d2, 1, it + 1)
    return torch.where(keep, term, torch.zeros_like(term)).sum(dim=0)


def timing(args, comm):
    assert comm.size == 1, "--time measures one GPU"
    dev = comm.device
    print(f"# pam_kirch on {torch.cuda.get_device_name(0)}: median ms per "
          f"apply over {args.rounds} rounds of at least 3 applies and 50 ms,"
          f" the cases alternating inside a round; Gpair/s counts ns * nr * "
          f"ni (trace, image point) pairs per apply")
    P = kernels.kirchhoff_points()
    shapes = [("tutorial", args.ns, args.nr, args.nx, args.nz, args.nt),
              ("big", *args.big)]
    for tdt in (torch.float32, torch.float64):
        for name, ns, nr, nx, nz, nt in shapes:
            a = argparse.Namespace(ns=ns, nr=nr, nx=nx, nz=nz, nt=nt)
            z, x, sources, recs, _ = geometry(a, 0, 1)
            t = np.arange(nt) * 0.004
            # a velocity that spreads the events over the whole trace
            far = np.hypot(x[-1], z[-1]) * 2.0
            op = pm.KirchhoffLocal(z, x, t, sources, recs, far / t[-1],
                                   dtype=str(tdt)[6:])
            qs, qr = op._tables(dev)
            ni = nx * nz
            pairs = ns * nr * ni
            gen = torch.Generator(device=dev).manual_seed(0)
            m = torch.randn(ni, dtype=tdt, device=dev, generator=gen)
            d = torch.randn((ns, nr, nt), dtype=tdt, device=dev,
                            generator=gen)
            dout, mout = torch.empty_like(d), torch.empty_like(m)
            for k in ENV:
                os.environ.pop(k, None)
            chunk = kernels.kirchhoff_chunk(d, m, qs, qr)
            win = kernels.kirchhoff_window(d, m, qs, qr)
            stage = kernels.kirchhoff_variant(d, m, qs, qr)
            print(f"{str(tdt)[6:]} {name}: ns={ns} nr={nr} ni={nx}x{nz}="
                  f"{ni} nt={nt}, {pairs / 1e6:.1f} Mpair; automatic plan: "
                  f"window {win}, chunk {chunk} of {ns * nr} traces, body "
                  f"{stage}, {P} points per workgroup")

            def fwd():
                kernels.kirchhoff(dout, m, qs, qr, False)

            def adj():
                kernels.kirchhoff(d, mout, qs, qr, True)
            cases = {"fwd auto": _forced({}, fwd)}
            for W in (128, 256, 512, 1024, 4096):
                if W < nt:
                    cases[f"fwd W={W}"] = _forced({"PAM_KIRCH_WINDOW": W},
                                                  fwd)
            cases[f"fwd W={nt}"] = _forced({"PAM_KIRCH_WINDOW": nt}, fwd)
            cases["adj auto"] = _forced({}, adj)
            for split in (0, 1):
                for st in (0, 1):
                    cases[f"adj split={split} stage={st}"] = _forced(
                        {"PAM_KIRCH_SPLIT": split, "PAM_KIRCH_STAGE": st},
                        adj)
            ms = _alternate(cases, args.rounds)
            for k in ENV:
                os.environ.pop(k, None)
            for k, v in ms.items():
                print(f"  {k:<24} {v:9.4f} ms  {pairs / v / 1e6:8.2f} "
                      f"Gpair/s")
            reps = 3 if pairs > 5e7 else 10
            torch_spread(m, qs, qr, nt)
            torch_gather(d, qs, qr, nt)
            torch.cuda.synchronize()
            tf = _time_ms(lambda: torch_spread(m, qs, qr, nt), reps)
            ta = _time_ms(lambda: torch_gather(d, qs, qr, nt), reps)
            print(f"  torch index_add_ spread    {tf:9.4f} ms  "
                  f"{pairs / tf / 1e6:8.2f} Gpair/s  "
                  f"({tf / ms['fwd auto']:.1f}x fwd auto)")
            print(f"  torch gather + sum         {ta:9.4f} ms  "
                  f"{pairs / ta / 1e6:8.2f} Gpair/s  "
                  f"({ta / ms['adj auto']:.1f}x adj auto)")
            # the wavelet stage next to the traveltime stage
            wav, _, wavc = pm.ricker(t[:args.ntwav], f0=20)
            full = pm.KirchhoffLocal(z, x, t, sources, recs, far / t[-1],
                                     wav, wavc, dtype=str(tdt)[6:])
            dv = d.view(-1)
            mo = _alternate({"op fwd": lambda: full.matvec(m),
                             "op adj": lambda: full.rmatvec(dv)},
                            args.rounds)
            print(f"  KirchhoffLocal + {len(wav)}-tap wavelet: matvec "
                  f"{mo['op fwd']:.4f} ms, rmatvec {mo['op adj']:.4f} ms")
            del op, full, m, d, dout, mout
    # maximum collision: every point of every trace on one sample pair
    for tdt in (torch.float32, torch.float64):
        ni, nt = 100000, 64
        gen = torch.Generator(device=dev).manual_seed(1)
        m = torch.randn(ni, dtype=tdt, device=dev, generator=gen)
        qs = torch.full((2, ni), 10.25, dtype=tdt, device=dev)
        qr = torch.full((3, ni), 7.5, dtype=tdt, device=dev)
        runs = []
        for _ in range(2):
            out = torch.empty((2, 3, nt), dtype=tdt, device=dev)
            kernels.kirchhoff(out, m, qs, qr, False)
            runs.append(out)
        same = torch.equal(runs[0].view(torch.uint8).cpu(),
                           runs[1].view(torch.uint8).cpu())
        print(f"# collision spread, {ni} points on one sample pair, "
              f"{str(tdt)[6:]}, run twice: bits "
              f"{'identical' if same else 'DIFFER'}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nx", type=int, default=81)
    ap.add_argument("--nz", type=int, default=60)
    ap.add_argument("--nr", type=int, default=11)
    ap.add_argument("--ns", type=int, default=10, help="sources per rank")
    ap.add_argument("--nt", type=int, default=651)
    ap.add_argument("--ntwav", type=int, default=21,
                    help="samples of the wavelet's half axis (taps: 2n - 1)")
    ap.add_argument("--niter", type=int, default=100)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--big", type=int, nargs=5, default=(64, 64, 256, 128,
                                                         1024),
                    metavar=("NS", "NR", "NX", "NZ", "NT"))
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    comm = init_default_comm()
    if args.time:
        timing(args, comm)
    else:
        invert(args, comm)


if __name__ == "__main__":
    main()

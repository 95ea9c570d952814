"""Post-stack seismic inversion and reflectivity deconvolution — the
reference's tutorials/poststack.py and tutorials/reflectivity.py on the
fused convolution kernel.

A seeded layered log-impedance volume (ny, nx, nz), split along y over the
ranks, is modelled with

    MPIBlockDiag([PoststackLinearModellingLocal(wav, nz, (ny_i, nx),
                                                axis=-1)])

(time along the contiguous last axis: no Transpose sandwich) and inverted
from a smoothed background, first with plain cgls, then with the
MPILaplacian-regularised MPIStackedVStack system.  ``--reflectivity``
instead deconvolves sparse reflectivity traces with fista on
MPIBlockDiag([Convolve1DLocal(...)]).  ``--time`` measures pam_conv1d's
kernels against each other on one GPU (device events, warmed up, the
variants alternating inside each round) and prints the table kept in
profiles/conv1d_variants.log.

    python examples/poststack_inversion.py [--reflectivity] [--dims NY NX NZ]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
        --master-addr 127.0.0.1 examples/poststack_inversion.py
    python examples/poststack_inversion.py --time [--mib 256]
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


def layered_model(ny, nx, nz, seed=0):
    """Log-impedance of nlay gently dipping layers plus its smoothed
    background; every rank draws the same volume."""
    rng = np.random.default_rng(seed)
    nlay = max(3, nz // 12)
    tops = np.sort(rng.choice(np.arange(2, nz - 2), nlay - 1, replace=False))
    vals = np.log(1500.0 + 120.0 * np.arange(nlay)
                  + 80.0 * rng.standard_normal(nlay))
    dip = (0.04 * nz / max(ny, 1)) * np.arange(ny)[:, None, None] \
        + (0.02 * nz / max(nx, 1)) * np.arange(nx)[None, :, None]
    z = np.arange(nz)[None, None, :] - dip
    m = vals[np.searchsorted(tops, z.ravel(), side="right")].reshape(
        ny, nx, nz)
    nsm = max(3, nz // 8) | 1
    pad = np.pad(m, ((0, 0), (0, 0), (nsm // 2, nsm // 2)), mode="edge")
    back = np.apply_along_axis(
        lambda v: np.convolve(v, np.ones(nsm) / nsm, mode="valid"), 2, pad)
    return m, back


def rows_of(ny, comm, rank):
    return pm.local_split((ny,), comm.size, rank, pm.Partition.SCATTER, 0)[0]


def dist(a, comm):
    """The (ny, ...) volume flattened, whole y-slabs per rank."""
    slab = a[0].size
    shapes = [(rows_of(a.shape[0], comm, r) * slab,)
              for r in range(comm.size)]
    return pm.DistributedArray.to_dist(
        torch.as_tensor(np.ascontiguousarray(a).ravel(), device=comm.device),
        comm, local_shapes=shapes)


def local_rows(ny, comm):
    return rows_of(ny, comm, comm.rank)


def poststack(args, comm):
    ny, nx, nz = args.dims
    wav = pm.ricker(np.arange(args.ntwav) * 0.004, f0=args.f0)[0]
    m, back = layered_model(ny, nx, nz)
    ny_i = local_rows(ny, comm)
    PPop = pm.PoststackLinearModellingLocal(wav, nz, spatdims=(ny_i, nx),
                                            axis=-1)
    BDiag = pm.MPIBlockDiag([PPop])
    m_dist, back_dist = dist(m, comm), dist(back, comm)
    d_dist = BDiag @ m_dist

    def err(x):
        return float((x - m_dist).norm() / m_dist.norm())

    x0 = back_dist.copy()
    minv = pm.cgls(BDiag, d_dist, x0, niter=args.niter, tol=0.0)[0]
    # regularised: [BDiag; sqrt(epsR) Lap] x = [d; 0]
    epsR = 1e-2
    LapOp = pm.MPILaplacian(dims=(ny, nx, nz), axes=(0, 1, 2),
                            weights=(1, 1, 1), sampling=(1, 1, 1))
    StackOp = pm.MPIStackedVStack([BDiag, np.sqrt(epsR) * LapOp])
    d0_dist = d_dist.zeros_like()
    dstack = pm.StackedDistributedArray([d_dist, d0_dist])
    mreg = pm.cgls(StackOp, dstack, back_dist.copy(), niter=args.niter,
                   tol=0.0)[0]
    res = float((BDiag @ minv - d_dist).norm() / d_dist.norm())
    if comm.rank == 0:
        print(f"poststack {ny}x{nx}x{nz}, {len(wav)}-tap ricker: relative "
              f"model error {err(back_dist):.4f} (background) -> "
              f"{err(minv):.4f} (cgls) / {err(mreg):.4f} (cgls + Laplacian);"
              f" data residual {res:.2e}")
    assert res < 0.5 and err(minv) <= err(back_dist) * 1.001


def reflectivity(args, comm):
    ny, nx, nz = args.dims
    wav, _, wavc = pm.ricker(np.arange(args.ntwav) * 0.004, f0=args.f0)
    rng = np.random.default_rng(1)
    r = np.zeros((ny, nx, nz))
    nspk = max(2, nz // 16)
    for iy in range(ny):
        for ix in range(nx):
            r[iy, ix, rng.choice(nz, nspk, replace=False)] = \
                rng.standard_normal(nspk)
    ny_i = local_rows(ny, comm)
    Cop = pm.Convolve1DLocal((ny_i, nx, nz), wav, offset=wavc, axis=-1)
    CDiag = pm.MPIBlockDiag([Cop])
    r_dist = dist(r, comm)
    d_dist = CDiag @ r_dist
    r0 = r_dist.zeros_like()
    rinv = pm.fista(CDiag, d_dist, r0, niter=args.niter, eps=2e-2,
                    tol=1e-8)[0]
    e0 = float((CDiag.H @ d_dist - r_dist).norm() / r_dist.norm())
    e1 = float((rinv - r_dist).norm() / r_dist.norm())
    res = float((CDiag @ rinv - d_dist).norm() / d_dist.norm())
    if comm.rank == 0:
        print(f"reflectivity {ny}x{nx}x{nz}, {len(wav)}-tap ricker: relative"
              f" error {e0:.4f} (adjoint) -> {e1:.4f} (fista); data "
              f"residual {res:.2e}")
    assert res < 0.5


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


def _alternate(cases, rounds, reps, window_ms=100.0):
    """{name: median ms} of callables timed in turn inside each round;
    each timed window holds at least ``reps`` applies and ``window_ms``."""
    n = {}
    for k, fn in cases.items():       # warm-up: code objects, caches
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        n[k] = max(reps, int(window_ms / max(_time_ms(fn, 5), 1e-3)))
    t = {k: [] for k in cases}
    for _ in range(rounds):
        for k, fn in cases.items():
            t[k].append(_time_ms(fn, n[k]))
    return {k: float(np.median(v)) for k, v in t.items()}


def _forced(v, fn):
    def run():
        if v is None:
            os.environ.pop("PAM_CONV_VARIANT", None)
        else:
            os.environ["PAM_CONV_VARIANT"] = str(v)
        fn()
    return run


def timing(args, comm):
    """pam_conv1d variants 0 / 1 / 2 and fused against two launches, at
    ``--mib`` MiB per volume with 41 taps, float32 and float64, contiguous
    traces (m = 1) and time-first columns; then the m sweep."""
    assert comm.size == 1, "--time measures one GPU"
    dev, nh, d = comm.device, 41, 1024
    wav = pm.ricker(np.arange(21) * 0.004, f0=20)[0]
    print(f"# pam_conv1d on {torch.cuda.get_device_name(0)}: median ms per "
          f"apply over {args.rounds} rounds of at least {args.reps} applies "
          f"and 100 ms, variants "
          f"alternating inside a round; nh = {nh}, offset = {nh // 2}; "
          f"GB/s counts one read and one write of the volume")
    print("# dtype layout [batch, d, m] MiB | dir deriv | plain trace "
          "column auto (ms) | best tiled vs plain | 2-launch (ms, auto)")
    gen = torch.Generator(device=dev).manual_seed(0)
    for tdt, size in ((torch.float32, 4), (torch.float64, 8)):
        n = args.mib * (1 << 20) // size
        for name, shape in (("trace", (n // d, d, 1)),
                            ("column", (1, d, n // d))):
            x = torch.randn(shape, dtype=tdt, device=dev, generator=gen)
            y, t1 = torch.empty_like(x), torch.empty_like(x)
            h = torch.as_tensor(wav, dtype=tdt, device=dev)
            for adj, deriv in ((False, 0), (True, 0), (False, 1), (True, 1)):
                def conv(dv=deriv, a=adj):
                    kernels.conv1d(y, x, h, a, nh // 2, dv)

                def two(a=adj):
                    if a:
                        kernels.conv1d(t1, x, h, True, nh // 2, 0)
                        kernels.fd_serial(y, t1, 5, False, 1.0)
                    else:
                        kernels.fd_serial(t1, x, 4, False, 1.0)
                        kernels.conv1d(y, t1, h, False, nh // 2, 0)
                # a column tile of one trace, or a flat run across rows
                # of thousands of columns, is not a configuration to time
                os.environ["PAM_CONV_VARIANT"] = "1"
                ok1 = kernels.conv1d_variant(x, nh) == 1
                os.environ["PAM_CONV_VARIANT"] = "2"
                ok2 = kernels.conv1d_variant(x, nh) == 2 and shape[2] >= 8
                cases = {"v0": _forced(0, conv)}
                if ok1:
                    cases["v1"] = _forced(1, conv)
                if ok2:
                    cases["v2"] = _forced(2, conv)
                cases["auto"] = _forced(None, conv)
                if deriv:
                    cases["two"] = _forced(None, two)
                t = _alternate(cases, args.rounds, args.reps)
                os.environ.pop("PAM_CONV_VARIANT", None)
                tiled = [t[k] for k, ok in (("v1", ok1), ("v2", ok2)) if ok]
                gbs = 2 * n * size / 1e6 / t["auto"]
                print(f"{str(tdt)[6:]} {name} {list(shape)} {args.mib} | "
                      f"{'adj' if adj else 'fwd'} {deriv} | {t['v0']:.3f} "
                      f"{t['v1'] if ok1 else float('nan'):.3f} "
                      f"{t['v2'] if ok2 else float('nan'):.3f} "
                      f"{t['auto']:.3f} ({gbs:.0f} GB/s) | "
                      f"{t['v0'] / min(tiled):.2f}x | "
                      f"{t.get('two', float('nan')):.3f}", flush=True)
            del x, y, t1
    print("# the 64 MiB volumes below fit the 256 MiB Infinity Cache: they "
          "rank the kernels, they are not HBM rates")
    print("# m sweep, [batch, 512, m] of 64 MiB, forward, deriv 0: ms "
          "plain / trace / column (nan: halo does not fit, or a column "
          "tile of fewer than 8 columns)")
    for tdt, size in ((torch.float32, 4), (torch.float64, 8)):
        n = 64 * (1 << 20) // size
        for m in (1, 2, 4, 8, 16, 24, 32, 48, 64, 65, 80, 96, 128, 160, 192,
                  256, 512, 1024):
            shape = (n // (512 * m), 512, m)
            x = torch.randn(shape, dtype=tdt, device=dev, generator=gen)
            y = torch.empty_like(x)
            h = torch.as_tensor(wav, dtype=tdt, device=dev)

            def conv():
                kernels.conv1d(y, x, h, False, nh // 2, 0)
            cases, ok = {}, {}
            for v in (0, 1, 2):
                os.environ["PAM_CONV_VARIANT"] = str(v)
                ok[v] = kernels.conv1d_variant(x, nh) == v and \
                    (v != 2 or m >= 8)
                if ok[v]:
                    cases[f"v{v}"] = _forced(v, conv)
            t = _alternate(cases, args.rounds, args.reps)
            os.environ.pop("PAM_CONV_VARIANT", None)
            print(f"{str(tdt)[6:]} m={m} | " + " ".join(
                f"{t.get(f'v{v}', float('nan')):.3f}" for v in (0, 1, 2))
                + f" | auto: {kernels.conv1d_variant(x, nh)}", flush=True)
            del x, y
    print("# nh sweep, 64 MiB, forward, deriv 0, offset nh // 2: ms plain / "
          "trace / column | kernel the automatic dispatch picks")
    for tdt, size in ((torch.float32, 4), (torch.float64, 8)):
        n = 64 * (1 << 20) // size
        for shape in ((n // 512, 512, 1), (n // (512 * 8), 512, 8),
                      (n // (512 * 64), 512, 64),
                      (n // (512 * 1024), 512, 1024)):
            x = torch.randn(shape, dtype=tdt, device=dev, generator=gen)
            y = torch.empty_like(x)
            for nhs in (1, 3, 9, 21, 41, 101):
                h = torch.randn(nhs, dtype=tdt, device=dev, generator=gen)

                def conv(h=h, nhs=nhs):
                    kernels.conv1d(y, x, h, False, nhs // 2, 0)
                cases = {}
                for v in (0, 1, 2):
                    os.environ["PAM_CONV_VARIANT"] = str(v)
                    if kernels.conv1d_variant(x, nhs) == v and \
                            (v != 2 or shape[2] >= 8):
                        cases[f"v{v}"] = _forced(v, conv)
                t = _alternate(cases, args.rounds, args.reps)
                os.environ.pop("PAM_CONV_VARIANT", None)
                print(f"{str(tdt)[6:]} m={shape[2]} nh={nhs} | " + " ".join(
                    f"{t.get(f'v{v}', float('nan')):.3f}"
                    for v in (0, 1, 2))
                    + f" | auto: {kernels.conv1d_variant(x, nhs)}",
                    flush=True)
            del x, y


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reflectivity", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--dims", type=int, nargs=3, default=(8, 12, 128),
                    metavar=("NY", "NX", "NZ"))
    ap.add_argument("--niter", type=int, default=60)
    ap.add_argument("--ntwav", type=int, default=21,
                    help="samples of the wavelet's half axis (taps: 2n - 1)")
    ap.add_argument("--f0", type=float, default=20.0)
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    comm = init_default_comm()
    if args.time:
        timing(args, comm)
    elif args.reflectivity:
        reflectivity(args, comm)
    else:
        poststack(args, comm)


if __name__ == "__main__":
    main()

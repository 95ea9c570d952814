"""Throughput of the L2,1 group kernel against axpy, in one run: 3
components of 2048*2048*32 float64, group_shrink in place with and
without the fused shift, and pam_axpy on one such array as the streaming
yardstick.  HIP events around each call, the three kernels alternating
within every repetition; GB/s from algorithmic bytes (group_shrink 16 B
per component-point, 24 B with shift; axpy 24 B per point).  Prints one
JSON line per kernel and one with the ratios to axpy.

Mode 1 (projection) keeps the in-place data from collapsing to zero over
the repetitions; the branch taken is a select, not a different memory
pattern, so the rate does not depend on it."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pylops_mpi_amd import kernels  # noqa: E402

NCOMP, N = 3, 2048 * 2048 * 32
WARMUP, REPS = 5, 30


def main():
    assert torch.cuda.is_available(), "this probe measures on the GPU"
    g = torch.Generator(device="cuda").manual_seed(0)

    def randn():
        return torch.randn(N, generator=g, dtype=torch.float64,
                           device="cuda")

    xs = [randn() for _ in range(NCOMP)]
    sh = [randn() for _ in range(NCOMP)]
    ax, ay = randn(), randn()
    runs = {
        "group_shrink": (lambda: kernels.group_shrink(xs, xs, 1, 1.0),
                         16 * NCOMP * N),
        "group_shrink_shift": (lambda: kernels.group_shrink(
            xs, xs, 1, 1.0, shift=sh, beta=1e-3), 24 * NCOMP * N),
        "axpy": (lambda: kernels.axpy(ay, ax, 1e-3), 24 * N),
    }
    ms = {name: [] for name in runs}
    for rep in range(WARMUP + REPS):
        for name, (fn, _) in runs.items():
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            if rep >= WARMUP:
                ms[name].append(t0.elapsed_time(t1))
    gbs = {}
    for name, (_, nbytes) in runs.items():
        t = sorted(ms[name])
        med = t[len(t) // 2]
        gbs[name] = nbytes / (med * 1e-3) / 1e9
        print(json.dumps({"probe": name, "ms_median": round(med, 4),
                          "ms_min": round(t[0], 4),
                          "ms_max": round(t[-1], 4),
                          "GB/s": round(gbs[name], 1)}), flush=True)
    print(json.dumps({"probe": "ratio_to_axpy",
                      "group_shrink": round(
                          gbs["group_shrink"] / gbs["axpy"], 3),
                      "group_shrink_shift": round(
                          gbs["group_shrink_shift"] / gbs["axpy"], 3)}),
          flush=True)


if __name__ == "__main__":
    main()

"""Environment feature gates — the analogue of the reference's
pylops_mpi/utils/deps.py:58-66 (NCCL_PYLOPS_MPI / PYLOPS_MPI_CUDA_AWARE):

  PAM_DISABLE_OVERLAP=1   serialize the halo exchange before the stencil
                          kernel instead of overlapping it with the
                          interior rows (debug aid)
  PAM_FD_GY / PAM_FD_CAP  row-parallel stencil launch-shape A/B knobs
                          (defaults: one block-row per row, ~4 vector
                          iterations per block — the measured optimum,
                          csrc/pam.hip fd_plan)
  PAM_FD_ROLL             rolling-window stencil select: unset = AUTO
                          (rows > PAM_FD_LONGROW bytes, default 4 MiB, or
                          >= 5/8 of it with a row count that is no
                          multiple of 1024, use the 1-load/pt rolling
                          kernel — the r02 long-row fix, 4.85 -> 5.35 TB/s
                          at the N=8 per-rank shape); -1 = force
                          row-parallel; > 0 = force rolling wherever 16-B
                          lanes exist
  PAM_FD_BAND             row-band stencil select (RT rows of one 16-B
                          column vector per thread, RT+2W loads up front):
                          unset = AUTO, 1 = band wherever eligible (16-B
                          lanes; any row count), -1 = never.  Read on every
                          launch, so it can be flipped in-process;
                          kernels.fd_variant reports the kernel a launch
                          will use.  AUTO picks it where it measured
                          faster: 2.5-4 MiB rows with a row count that is
                          no multiple of 1024 and >= 16 (5.63 vs the
                          rolling kernel's 5.34 TB/s at 1536x1536x256); it
                          lost to the row-parallel kernel at the bench
                          shape and to the rolling kernel above 4 MiB rows
                          
  PAM_FD_ROLL_TGT         rolling kernel's target grid size (default 2048,
                          the r02 swept optimum)
  PAM_CGEMM_BK            complex batched GEMM K-panel depth without
                          accumulate: unset = AUTO (8 for K <= 64, else 16:
                          each won on its side at the cfg5 shapes,
                          csrc/gemm.hip cgemm_bk), 8 / 16 = force.  Read
                          once per process
  PAM_EW_CAP              1-D elementwise grid cap (default: none — one
                          block per 256 vector items; the old 4096-block
                          grid-stride loop cost 28% of axpy bandwidth)
  PAM_DISABLE_DEVSCALARS=1  run CG/CGLS with host-side scalars (one
                          blocking readback per dot) instead of the
                          single-sync device-scalar iteration (debug aid;
                          both paths are bit-identical)

The knobs that only selected measured-negative code went with that code
(DESIGN.md "Negative results kept"): the stencils' lane-width forcing, nt
stores and loads, and the rolling kernel's chains per thread, now the
constant 8; the complex GEMM's 128x64 tile and single-buffered panels.

The RCCL data plane itself has no gate: it IS the backend (there is no
MPI in this stack to fall back to)."""
import os


def env_flag(name: str, default: bool = False) -> bool:
    v = os.environ.get(name)
    return default if v is None else v not in ("0", "", "false", "False")


overlap_enabled = not env_flag("PAM_DISABLE_OVERLAP")
devscalars_enabled = not env_flag("PAM_DISABLE_DEVSCALARS")

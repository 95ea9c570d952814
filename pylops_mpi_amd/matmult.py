"""MPIMatrixMult — distributed matrix-matrix multiplication (block-row and
SUMMA kinds) on MFMA panel GEMMs + RCCL grid collectives.

Drop-in for /root/reference/pylops_mpi/basicoperators/MatrixMult.py:
  active_grid_comm      -> ref :24-79
  local_block_split     -> ref :82-129
  block_gather          -> ref :132-175
  _MPIBlockMatrixMult   -> ref :178-427
  _MPISummaMatrixMult   -> ref :430-765
  MPIMatrixMult factory -> ref :768-872

MI355X-first differences:
  * local panels run on hand-written MFMA kernels (pam_gemm:
    v_mfma_f32_32x32x2_f32 exact-f32 / v_mfma_f64_16x16x4_f64; complex
    dtypes on the 4-chain MFMA pam_cgemm_batched with batch=1) instead
    of CuPy matmul; A^T/A^H panels are materialized by LDS-tiled
    transpose kernels (pam_transpose / pam_ctranspose; `saveAt=True`
    stores it once, ref :317-318);
  * row/col communicators are RCCL process groups (comm.split_by); the
    SUMMA adjoint's tag-routed A^T exchange (ref :745-760) is posted as
    one batched isend/irecv round per step — RCCL has no tags, and each
    (src,dst) pair carries exactly one message per round, so ordering is
    preserved by construction;
  * metadata (shape gathers) travels on the gloo control plane of the
    WORLD communicator (all memberships are deterministic).
Like the reference (ref :295-298,564-566), both kinds default to a
square number of ranks, and active_grid_comm carves an active square
grid out of a non-square world (e.g. 2x2 out of 8).  BEYOND the
reference, the summa kind also accepts an explicit rectangular process
grid (``grid=(Pr, Pc)`` with Pr*Pc == comm size): BASELINE cfg4 names a
2x4 grid on 8 GPUs, which the reference cannot run (its SUMMA is
square-only, so active_grid_comm would idle 4 of 8 GPUs).  The
rectangular path is classic panel SUMMA: K is padded to a multiple of
L = lcm(Pr, Pc) and walked in L panels; each step row-broadcasts an A
panel, col-broadcasts an X panel and accumulates on the MFMA panel
GEMM; the adjoint reuses the same A-panel broadcast and turns the
tag-routed A^T exchange into a col-comm reduce-to-owner (RCCL-friendly
— no tags needed).  Results match dense A@X / A^H y exactly like the
square path (world-8 gloo tests, tests/test_dist_gloo_rect.py).
"""
import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import kernels
from .comm import PamComm, get_default_comm
from .distributedarray import DistributedArray, Partition, as_torch_dtype
from .linearoperator import MPILinearOperator


def active_grid_comm(base_comm: PamComm, N: int, M: int):
    """ref :24-79 — carve the largest useful square grid; inactive ranks
    get (None, rank, row, col, False)."""
    rank, size = base_comm.rank, base_comm.size
    p_prime = math.isqrt(size)
    row, col = divmod(rank, p_prime)
    active_dim = min(N, M, p_prime)
    is_active = (row < active_dim and col < active_dim)
    # every rank participates in group creation (torch.distributed rule)
    colors = []
    for r in range(size):
        rr, cc = divmod(r, p_prime)
        colors.append(0 if (rr < active_dim and cc < active_dim) else 1 + r)
    new_comm = base_comm.split_by(colors, keys=list(range(size)))
    if not is_active:
        return None, rank, row, col, False
    p_new = math.isqrt(new_comm.size)
    new_rank = new_comm.rank
    new_row, new_col = divmod(new_rank, p_new)
    return new_comm, new_rank, new_row, new_col, True


def local_block_split(global_shape: Tuple[int, int], rank: int,
                      comm: PamComm) -> Tuple[slice, slice]:
    """ref :82-129 — this rank's (row_slice, col_slice) of a 2-D array on
    a square process grid."""
    size = comm.size
    p_prime = math.isqrt(size)
    if p_prime * p_prime != size:
        raise RuntimeError(f"Number of processes must be a square number, "
                           f"provided {size} instead...")
    if not (isinstance(rank, (int, np.integer)) and 0 <= rank < size):
        raise ValueError(
            f"rank must be an integer in [0, {size}), got {rank!r}")
    pr, pc = divmod(int(rank), p_prime)
    orig_r, orig_c = global_shape
    blkr = math.ceil(orig_r / p_prime)
    blkc = math.ceil(orig_c / p_prime)
    rs, cs = pr * blkr, pc * blkc
    re, ce = min(rs + blkr, orig_r), min(cs + blkc, orig_c)
    return slice(rs, re), slice(cs, ce)


def block_gather(x: DistributedArray, orig_shape: Tuple[int, int],
                 comm: PamComm) -> torch.Tensor:
    """ref :132-175 — reassemble a 2-D-block-distributed matrix."""
    p_prime = math.isqrt(comm.size)
    if p_prime * p_prime != comm.size:
        raise RuntimeError(
            f"Communicator size must be a perfect square, got {comm.size!r}")
    nr, nc = orig_shape
    shapes = [(int(np.prod(s)),) for s in x.local_shapes]
    blks = comm.allgather_tensors(x.local_array.reshape(-1), shapes)
    C = torch.zeros((nr, nc), dtype=x.local_array.dtype,
                    device=x.local_array.device)
    for rank in range(p_prime * p_prime):
        rs, cs = local_block_split(orig_shape, rank, comm)
        if blks[rank].numel() != 0:
            C[rs, cs] = blks[rank].reshape(rs.stop - rs.start,
                                           cs.stop - cs.start)
    return C


def summa_grid_splits(N: int, K: int, M: int, Pr: int, Pc: int):
    """Per-rank (row_slice, col_slice) for A [N,K] and X [K,M] on a
    rectangular Pr x Pc grid (rank = row*Pc + col).

    The K direction is padded to a multiple of L = lcm(Pr, Pc) so that
    both A's column split (by Pc) and X's row split (by Pr) land on
    panel boundaries — the rectangular analogue of the reference's
    square padding (ref :589-601)."""
    L = math.lcm(Pr, Pc)
    K_pad = math.ceil(K / L) * L
    bn = math.ceil(N / Pr)
    bkA = K_pad // Pc
    bkX = K_pad // Pr
    bm = math.ceil(M / Pc)
    a_slices, x_slices, y_slices = [], [], []
    for q in range(Pr * Pc):
        qr, qc = divmod(q, Pc)
        a_slices.append((slice(qr * bn, min((qr + 1) * bn, N)),
                         slice(qc * bkA, min((qc + 1) * bkA, K))))
        x_slices.append((slice(qr * bkX, min((qr + 1) * bkX, K)),
                         slice(qc * bm, min((qc + 1) * bm, M))))
        y_slices.append((slice(qr * bn, min((qr + 1) * bn, N)),
                         slice(qc * bm, min((qc + 1) * bm, M))))
    return a_slices, x_slices, y_slices


class _MatMultBase(MPILinearOperator):
    """Shared plumbing: grid comms + HIP panel GEMM/transpose."""

    def _make_grid(self, comm: PamComm):
        size = comm.size
        self._P_prime = math.isqrt(size)
        if self._P_prime * self._P_prime != size:
            raise Exception(f"Number of processes must be a square number, "
                            f"provided {size} instead...")
        return self._P_prime

    # local HIP panels (overridable in CPU comm-logic tests)
    def _local_gemm(self, A: torch.Tensor, B: torch.Tensor,
                    C: Optional[torch.Tensor] = None,
                    accumulate: bool = False) -> torch.Tensor:
        if C is None:
            C = torch.empty((A.shape[0], B.shape[1]), dtype=A.dtype,
                            device=A.device)
        # complex panels: the batched MFMA cgemm with batch=1
        # (ref MatrixMult.py supports complex dtypes throughout)
        kernels.gemm(C, A, B, accumulate)
        return C

    def _local_transpose(self, A: torch.Tensor) -> torch.Tensor:
        """A^T for real dtypes, A^H for complex (ref :317-318,416,737
        ``A.T.conj()`` — conj is a no-op on reals)."""
        At = torch.empty((A.shape[1], A.shape[0]), dtype=A.dtype,
                         device=A.device)
        kernels.transpose(At, A, conj=True)
        return At

    def _AH(self) -> torch.Tensor:
        # ref :416,737: use saved At or compute A.T.conj() on the fly
        return self.At if hasattr(self, "At") else self._local_transpose(self.A)

    @staticmethod
    def _check_scatter(x: DistributedArray):
        if x.partition != Partition.SCATTER:
            raise ValueError(f"x should have partition={Partition.SCATTER} "
                             f"Got {x.partition} instead...")


class _MPIBlockMatrixMult(_MatMultBase):
    """1-D block-row A x column-replicated X (ref :178-427)."""

    def __init__(self, A: torch.Tensor, M: int, saveAt: bool = False,
                 base_comm: Optional[PamComm] = None, dtype="float64"):
        comm = base_comm if base_comm is not None else get_default_comm()
        rank, size = comm.rank, comm.size
        self.base_comm_grid = comm
        P = self._make_grid(comm)
        self._col_id = rank % P
        self._row_id = rank // P
        # ref :305-306
        self._row_comm = comm.split_by([r // P for r in range(size)],
                                       [r % P for r in range(size)])
        self._col_comm = comm.split_by([r % P for r in range(size)],
                                       [r // P for r in range(size)])
        self.A = A.to(as_torch_dtype(np.dtype(dtype)))
        if saveAt:
            self.At = self._local_transpose(self.A)
        # N = sum of A-rows across the row communicator (ref :320)
        all_rows = comm.allgather_obj(int(A.shape[0]))
        row_members = [r for r in range(size) if r // P == self._row_id]
        self._row_nlocs = [all_rows[r] for r in row_members]
        self.N = int(sum(self._row_nlocs))
        self.K = int(A.shape[1])
        self.M = M
        block_cols = int(math.ceil(self.M / P))
        blk_rows = int(math.ceil(self.N / P))
        self._row_start = self._col_id * blk_rows
        self._row_end = min(self.N, self._row_start + blk_rows)
        self._col_start = self._row_id * block_cols
        self._col_end = min(self.M, self._col_start + block_cols)
        self._local_ncols = max(0, self._col_end - self._col_start)
        self._rank_col_lens = comm.allgather_obj(self._local_ncols)
        total_ncols = int(np.sum(self._rank_col_lens))
        dims = (self.K, total_ncols)
        dimsd = (self.N, total_ncols)
        super().__init__(dims=dims, dimsd=dimsd, dtype=np.dtype(dtype),
                         base_comm=comm)

    def _matvec(self, x: DistributedArray) -> DistributedArray:
        # ref :341-377
        self._check_scatter(x)
        y = DistributedArray(
            int(self.N * self.dimsd[1]), x.base_comm, Partition.SCATTER, 0,
            local_shapes=[(int(self.N * c),) for c in self._rank_col_lens],
            dtype=self.dtype)
        my_cols = self._rank_col_lens[self.rank]
        x_arr = x.local_array.reshape(self.dims[0], my_cols).to(self.A.dtype)
        prod = self._local_gemm(self.A, x_arr)          # (N_loc, M_loc)
        tiles = self._row_comm.allgather_tensors(
            prod.reshape(-1),
            [(n, my_cols) for n in self._row_nlocs])    # ref :369-375
        y[:] = torch.vstack(tiles).reshape(-1)
        return y

    def _rmatvec(self, x: DistributedArray) -> DistributedArray:
        # ref :379-427
        self._check_scatter(x)
        y = DistributedArray(
            int(self.K * self.dimsd[1]), x.base_comm, Partition.SCATTER, 0,
            local_shapes=[(int(self.K * c),) for c in self._rank_col_lens],
            dtype=self.dtype)
        x_arr = x.local_array.reshape(self.N, self._local_ncols).to(self.A.dtype)
        X_tile = x_arr[self._row_start: self._row_end, :].contiguous()
        Y_local = self._local_gemm(self._AH(), X_tile)  # (K, M_loc)
        self._row_comm.allreduce_(Y_local, "sum")       # ref :419-425
        y[:] = Y_local.reshape(-1)
        return y


class _MPISummaMatrixMult(_MatMultBase):
    """2-D SUMMA (ref :430-765); ``grid=(Pr, Pc)`` extends it to
    rectangular process grids (BASELINE cfg4's 2x4 on 8 ranks — beyond
    the reference's square-only restriction, ref :564-566)."""

    def __init__(self, A: torch.Tensor, M: int, saveAt: bool = False,
                 base_comm: Optional[PamComm] = None, dtype="float64",
                 grid: Optional[Tuple[int, int]] = None):
        comm = base_comm if base_comm is not None else get_default_comm()
        rank, size = comm.rank, comm.size
        self.base_comm_grid = comm
        if grid is not None and tuple(grid)[0] != tuple(grid)[1]:
            self._init_rect(A, M, comm, dtype, tuple(grid))
            return
        if grid is not None and grid[0] * grid[1] != size:
            raise ValueError(f"grid {grid} does not tile {size} ranks")
        self._rect = False
        P = self._make_grid(comm)
        self._row_id, self._col_id = divmod(rank, P)
        self._row_comm = comm.split_by([r // P for r in range(size)],
                                       [r % P for r in range(size)])
        self._col_comm = comm.split_by([r % P for r in range(size)],
                                       [r // P for r in range(size)])
        self.A = A.to(as_torch_dtype(np.dtype(dtype)))
        all_rows = comm.allgather_obj(int(A.shape[0]))
        all_cols = comm.allgather_obj(int(A.shape[1]))
        col_members = [r for r in range(size) if r % P == self._col_id]
        row_members = [r for r in range(size) if r // P == self._row_id]
        self.N = int(sum(all_rows[r] for r in col_members))   # ref :585
        self.K = int(sum(all_cols[r] for r in row_members))   # ref :586
        self.M = M
        self._N_padded = math.ceil(self.N / P) * P
        self._K_padded = math.ceil(self.K / P) * P
        self._M_padded = math.ceil(self.M / P) * P
        bn = self._N_padded // P
        bk = self._K_padded // P
        pr = (bn - int(A.shape[0])) if self._row_id == P - 1 else 0
        pc = (bk - int(A.shape[1])) if self._col_id == P - 1 else 0
        if pr > 0 or pc > 0:  # ref :597-601
            Ap = torch.zeros((int(A.shape[0]) + pr, int(A.shape[1]) + pc),
                             dtype=self.A.dtype, device=self.A.device)
            Ap[: A.shape[0], : A.shape[1]] = self.A
            self.A = Ap
        if saveAt:
            self.At = self._local_transpose(self.A)
        super().__init__(dims=(self.K, self.M), dimsd=(self.N, self.M),
                         dtype=np.dtype(dtype), base_comm=comm)

    # ------------------------------------------------ rectangular grid
    def _init_rect(self, A: torch.Tensor, M: int, comm: PamComm, dtype,
                   grid: Tuple[int, int]):
        Pr, Pc = grid
        if Pr * Pc != comm.size:
            raise ValueError(f"grid {grid} does not tile {comm.size} ranks")
        self._rect = True
        self._grid = (Pr, Pc)
        rank, size = comm.rank, comm.size
        self._row_id, self._col_id = divmod(rank, Pc)
        self._row_comm = comm.split_by([r // Pc for r in range(size)],
                                       [r % Pc for r in range(size)])
        self._col_comm = comm.split_by([r % Pc for r in range(size)],
                                       [r // Pc for r in range(size)])
        self.A = A.to(as_torch_dtype(np.dtype(dtype)))
        all_rows = comm.allgather_obj(int(A.shape[0]))
        all_cols = comm.allgather_obj(int(A.shape[1]))
        col_members = [r for r in range(size) if r % Pc == self._col_id]
        row_members = [r for r in range(size) if r // Pc == self._row_id]
        self.N = int(sum(all_rows[r] for r in col_members))
        self.K = int(sum(all_cols[r] for r in row_members))
        self.M = M
        L = math.lcm(Pr, Pc)
        self._L = L
        self._N_padded = math.ceil(self.N / Pr) * Pr
        self._K_padded = math.ceil(self.K / L) * L
        self._M_padded = math.ceil(self.M / Pc) * Pc
        bn = self._N_padded // Pr
        bkA = self._K_padded // Pc
        # remainder-only-on-last-block rule (inherited from the
        # reference's square padding, ref :589-601)
        if self.N < (Pr - 1) * bn or self.K < (Pc - 1) * bkA \
                or self.K < (Pr - 1) * (self._K_padded // Pr) \
                or self.M < (Pc - 1) * (self._M_padded // Pc):
            raise ValueError(
                f"shape ({self.N},{self.K},{self.M}) too small for grid "
                f"{grid}: non-final blocks would be ragged")
        pr_ = (bn - int(A.shape[0])) if self._row_id == Pr - 1 else 0
        pc_ = (bkA - int(A.shape[1])) if self._col_id == Pc - 1 else 0
        if pr_ > 0 or pc_ > 0:
            Ap = torch.zeros((int(A.shape[0]) + pr_, int(A.shape[1]) + pc_),
                             dtype=self.A.dtype, device=self.A.device)
            Ap[: A.shape[0], : A.shape[1]] = self.A
            self.A = Ap
        # saveAt is a no-op on the rect path: the adjoint transposes the
        # BROADCAST-RECEIVED panels, not this rank's own A
        MPILinearOperator.__init__(
            self, dims=(self.K, self.M), dimsd=(self.N, self.M),
            dtype=np.dtype(dtype), base_comm=comm)

    def _rect_sizes(self):
        Pr, Pc = self._grid
        bn = self._N_padded // Pr
        bkX = self._K_padded // Pr
        bm = self._M_padded // Pc
        local_n = bn if self._row_id != Pr - 1 else self.N - (Pr - 1) * bn
        local_k = max(0, bkX if self._row_id != Pr - 1
                      else self.K - (Pr - 1) * bkX)
        local_m = bm if self._col_id != Pc - 1 else self.M - (Pc - 1) * bm
        return bn, bkX, bm, local_n, local_k, local_m

    def _rect_counts(self, kind: str):
        Pr, Pc = self._grid
        bn = self._N_padded // Pr
        bkX = self._K_padded // Pr
        bm = self._M_padded // Pc
        out = []
        for q in range(Pr * Pc):
            qr, qc = divmod(q, Pc)
            ln = bn if qr != Pr - 1 else self.N - (Pr - 1) * bn
            lk = max(0, bkX if qr != Pr - 1 else self.K - (Pr - 1) * bkX)
            lm = bm if qc != Pc - 1 else self.M - (Pc - 1) * bm
            out.append(int((ln if kind == "n" else lk) * lm))
        return out

    def _rect_panels(self, t: int):
        """Step t owners/offsets: A panel lives at grid col cA (offset
        pA within its block), X panel at grid row rX (offset pX)."""
        Pr, Pc = self._grid
        L = self._L
        cA, pA = divmod(t, L // Pc)
        rX, pX = divmod(t, L // Pr)
        return cA, pA, rX, pX

    def _matvec_rect(self, x: DistributedArray) -> DistributedArray:
        self._check_scatter(x)
        Pr, Pc = self._grid
        L = self._L
        bkp = self._K_padded // L
        bn, bkX, bm, local_n, local_k, local_m = self._rect_sizes()
        y = DistributedArray(
            int(self.N * self.M), x.base_comm, Partition.SCATTER, 0,
            local_shapes=[(c,) for c in self._rect_counts("n")],
            dtype=self.dtype)
        x_block = self._pad_block(
            x.local_array.reshape(local_k, local_m).to(self.A.dtype),
            bkX, bm)
        Y_local = torch.zeros((bn, bm), dtype=self.A.dtype,
                              device=self.A.device)

        def post(t):
            cA, pA, rX, pX = self._rect_panels(t)
            if self._col_id == cA:
                Aslice = self.A[:, pA * bkp: (pA + 1) * bkp].contiguous()
            else:
                Aslice = torch.empty((bn, bkp), dtype=self.A.dtype,
                                     device=self.A.device)
            wa = self._row_comm.broadcast_async(Aslice, root=cA)
            if self._row_id == rX:
                Xslice = x_block[pX * bkp: (pX + 1) * bkp, :].contiguous()
            else:
                Xslice = torch.empty((bkp, bm), dtype=self.A.dtype,
                                     device=self.A.device)
            wx = self._col_comm.broadcast_async(Xslice, root=rX)
            return Aslice, Xslice, [w for w in (wa, wx) if w is not None]

        cur = post(0)
        for t in range(L):
            nxt = post(t + 1) if t + 1 < L else None
            Aslice, Xslice, works = cur
            for w in works:
                w.wait()
            self._local_gemm(Aslice, Xslice, Y_local, accumulate=True)
            cur = nxt
        y[:] = Y_local[:local_n, :local_m].reshape(-1)
        return y

    def _rmatvec_rect(self, x: DistributedArray) -> DistributedArray:
        self._check_scatter(x)
        Pr, Pc = self._grid
        L = self._L
        bkp = self._K_padded // L
        bn, bkX, bm, local_n, local_k, local_m = self._rect_sizes()
        y = DistributedArray(
            int(self.K * self.M), x.base_comm, Partition.SCATTER, 0,
            local_shapes=[(c,) for c in self._rect_counts("k")],
            dtype=self.dtype)
        x_block = self._pad_block(
            x.local_array.reshape(local_n, local_m).to(self.A.dtype),
            bn, bm)
        Z = torch.zeros((bkX, bm), dtype=self.A.dtype,
                        device=self.A.device)

        def post(t):
            cA, pA, rX, pX = self._rect_panels(t)
            if self._col_id == cA:
                Aslice = self.A[:, pA * bkp: (pA + 1) * bkp].contiguous()
            else:
                Aslice = torch.empty((bn, bkp), dtype=self.A.dtype,
                                     device=self.A.device)
            wa = self._row_comm.broadcast_async(Aslice, root=cA)
            return Aslice, rX, pX, ([wa] if wa is not None else [])

        cur = post(0)
        for t in range(L):
            nxt = post(t + 1) if t + 1 < L else None
            Aslice, rX, pX, works = cur
            for w in works:
                w.wait()
            # G = Aslice^H @ x_block, summed over the grid column to the
            # X-panel owner (replaces the square path's tag-routed A^T
            # exchange, ref :745-760 — RCCL has no tags)
            G = self._local_gemm(self._local_transpose(Aslice), x_block)
            self._col_comm.reduce_(G, root=rX)
            if self._row_id == rX:
                Z[pX * bkp: (pX + 1) * bkp, :] = G
            cur = nxt
        y[:] = Z[:local_k, :local_m].reshape(-1)
        return y

    def _tile_sizes(self):
        P = self._P_prime
        bn = self._N_padded // P
        bk = self._K_padded // P
        bm = self._M_padded // P
        local_n = bn if self._row_id != P - 1 else self.N - (P - 1) * bn
        local_k = bk if self._row_id != P - 1 else self.K - (P - 1) * bk
        local_m = bm if self._col_id != P - 1 else self.M - (P - 1) * bm
        return bn, bk, bm, local_n, local_k, local_m

    def _all_counts(self, kind: str):
        """Deterministic per-rank output element counts (the reference
        allgathers them, ref :630,688)."""
        P = self._P_prime
        bn = self._N_padded // P
        bk = self._K_padded // P
        bm = self._M_padded // P
        out = []
        for q in range(P * P):
            qr, qc = divmod(q, P)
            ln = bn if qr != P - 1 else self.N - (P - 1) * bn
            lk = bk if qr != P - 1 else self.K - (P - 1) * bk
            lm = bm if qc != P - 1 else self.M - (P - 1) * bm
            out.append(int((ln if kind == "n" else lk) * lm))
        return out

    def _pad_block(self, blk: torch.Tensor, rows: int, cols: int):
        if blk.shape[0] == rows and blk.shape[1] == cols:
            return blk.contiguous()
        out = torch.zeros((rows, cols), dtype=blk.dtype, device=blk.device)
        out[: blk.shape[0], : blk.shape[1]] = blk
        return out

    def _matvec(self, x: DistributedArray) -> DistributedArray:
        # ref :610-672
        if self._rect:
            return self._matvec_rect(x)
        self._check_scatter(x)
        P = self._P_prime
        bn, bk, bm, local_n, local_k, local_m = self._tile_sizes()
        y = DistributedArray(
            int(self.N * self.M), x.base_comm, Partition.SCATTER, 0,
            local_shapes=[(c,) for c in self._all_counts("n")],
            dtype=self.dtype)
        x_block = self._pad_block(
            x.local_array.reshape(local_k, local_m).to(self.A.dtype), bk, bm)
        Y_local = torch.zeros((self.A.shape[0], bm), dtype=self.A.dtype,
                              device=self.A.device)

        # bcasts pipelined across the k-loop: step k+1's tiles are in
        # flight while step k's panel GEMM runs (the reference serializes
        # bcast -> GEMM every step, ref :666-668)
        def post(k):
            Atemp = self.A.contiguous() if self._col_id == k \
                else torch.empty_like(self.A)
            Xtemp = x_block if self._row_id == k \
                else torch.empty_like(x_block)
            wa = self._row_comm.broadcast_async(Atemp, root=k)  # ref :666
            wx = self._col_comm.broadcast_async(Xtemp, root=k)  # ref :667
            return Atemp, Xtemp, [w for w in (wa, wx) if w is not None]

        cur = post(0)
        for k in range(P):
            nxt = post(k + 1) if k + 1 < P else None
            Atemp, Xtemp, works = cur
            for w in works:
                w.wait()
            self._local_gemm(Atemp, Xtemp, Y_local, accumulate=True)
            cur = nxt
        y[:] = Y_local[:local_n, :local_m].reshape(-1)
        return y

    def _rmatvec(self, x: DistributedArray) -> DistributedArray:
        # ref :674-765
        if self._rect:
            return self._rmatvec_rect(x)
        self._check_scatter(x)
        P = self._P_prime
        bn, bk, bm, local_n, local_k, local_m = self._tile_sizes()
        y = DistributedArray(
            int(self.K * self.M), x.base_comm, Partition.SCATTER, 0,
            local_shapes=[(c,) for c in self._all_counts("k")],
            dtype=self.dtype)
        x_block = self._pad_block(
            x.local_array.reshape(local_n, local_m).to(self.A.dtype), bn, bm)
        A_local = self._AH()                         # (bk, bn)
        Y_local = torch.zeros((self.A.shape[1], bm), dtype=self.A.dtype,
                              device=self.A.device)
        comm = self.base_comm_grid
        me = comm.rank

        # comm pipelined across the k-loop like the forward: step k+1's
        # X bcast and A^H routing round are in flight under step k's GEMM
        def post(k):
            Xtemp = x_block if self._row_id == k \
                else torch.empty_like(x_block)
            wx = self._col_comm.broadcast_async(Xtemp, root=k)
            # A^T routing (ref :745-760): rank (r,c) consumes the A^T of
            # grid rank (k, r); grid-row-k members send theirs to every
            # member of grid row <their col_id>.
            srcA = k * P + self._row_id
            sends, recvs = [], []
            if self._row_id == k:
                for moving_col in range(P):
                    destA = self._col_id * P + moving_col
                    if destA != me:
                        sends.append((A_local.contiguous(), destA))
            if srcA == me:
                ATtemp = A_local
            else:
                ATtemp = torch.empty_like(A_local)
                recvs.append((ATtemp, srcA))
            works = comm.exchange_async(sends, recvs)
            if wx is not None:
                works = works + [wx]
            return ATtemp, Xtemp, works

        cur = post(0)
        for k in range(P):
            nxt = post(k + 1) if k + 1 < P else None
            ATtemp, Xtemp, works = cur
            for w in works:
                w.wait()
            self._local_gemm(ATtemp, Xtemp, Y_local, accumulate=True)
            cur = nxt
        y[:] = Y_local[:local_k, :local_m].reshape(-1)
        return y


def MPIMatrixMult(A: torch.Tensor, M: int, saveAt: bool = False,
                  base_comm: Optional[PamComm] = None,
                  kind: str = "summa", dtype="float64",
                  grid: Optional[Tuple[int, int]] = None):
    """Factory, ref :768-872.  ``grid=(Pr, Pc)`` (summa only) selects a
    rectangular process grid — the cfg4 2x4-on-8-GPUs layout the
    reference's square-only SUMMA cannot express."""
    if kind == "summa":
        return _MPISummaMatrixMult(A, M, saveAt, base_comm, dtype,
                                   grid=grid)
    elif kind == "block":
        if grid is not None:
            raise NotImplementedError(
                "rectangular grids are a summa-kind extension")
        return _MPIBlockMatrixMult(A, M, saveAt, base_comm, dtype)
    raise NotImplementedError("kind must be summa or block")

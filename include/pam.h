/* pam — pylops-mpi hot path, MI355X-native (gfx950) C-ABI.
 *
 * Stateless kernel entry points over raw device pointers + HIP streams.
 * Device memory ownership, rank partitioning and RCCL collectives live in
 * the host layer (pylops_mpi_amd, PyTorch-ROCm device tensors +
 * torch.distributed over RCCL); this library is pure compute.
 *
 * Each entry point names the reference interface it replaces
 * (paths relative to /root/reference/pylops_mpi/).
 *
 * Conventions:
 *  - `stream` is a hipStream_t passed as void* (the caller's current
 *    stream; the library never synchronizes).
 *  - all functions return 0 on success, a hipError_t (>0) on launch
 *    failure, or a PAM_E* code (<0) on argument errors.
 *  - `dtype`: 0 = float64, 1 = float32, 2 = complex128, 3 = complex64
 *    (complex: interleaved re,im pairs of the base type).
 *  - scalar outputs (`out`) are single-element float64 device buffers.
 *  - n == 0: the element-wise, (de)interleave and reduction entry points
 *    read no array and accept NULL array pointers (an empty block has no
 *    storage).  The element-wise and (de)interleave ones launch nothing;
 *    the reductions still write their empty result to `out`, from a
 *    kernel on `stream`: in stream order, with no host-blocking call.
 */
#ifndef PAM_H
#define PAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PAM_F64 0
#define PAM_F32 1
#define PAM_C128 2 /* complex: interleaved (re, im) pairs of the base type */
#define PAM_C64 3

#define PAM_EARG   (-1)  /* bad argument */
#define PAM_EDTYPE (-2)  /* unsupported dtype */
#define PAM_EOP    (-3)  /* unknown op code */

/* ABI version, bumped on any signature change. */
int64_t pam_version(void);

/* Number of float64 workspace elements the reduction entry points need in
 * `ws` (device buffer). */
int64_t pam_reduce_ws_elems(void);

/* ------------------------------------------------------------------ *
 * Element-wise vector ops.
 * Replaces DistributedArray.add/iadd/multiply/__neg__/__setitem__
 * (ref DistributedArray.py:605-683,214-252) — per-rank local math on the
 * HBM-resident block.
 * ------------------------------------------------------------------ */
int pam_fill(void* stream, void* y, int64_t n, double value, int dtype);
int pam_neg(void* stream, void* y, const void* x, int64_t n, int dtype);
/* y = a + b */
int pam_add(void* stream, void* y, const void* a, const void* b, int64_t n,
            int dtype);
/* y = a - b (bitwise equal to the reference's add(-b), ref :624-628) */
int pam_sub(void* stream, void* y, const void* a, const void* b, int64_t n,
            int dtype);
/* y = a * b */
int pam_mul(void* stream, void* y, const void* a, const void* b, int64_t n,
            int dtype);
/* y = alpha * x */
int pam_scale(void* stream, void* y, const void* x, double alpha, int64_t n,
              int dtype);
/* y += alpha * x — the fused CGLS update (x += a*c / s -= a*q,
 * ref optimization/cls_basic.py:390-391: the reference materializes two
 * temporaries per axpy; this is one pass). */
int pam_axpy(void* stream, void* y, const void* x, double alpha, int64_t n,
             int dtype);
/* y = x + beta * y — the CGLS direction update c = r + b*c
 * (ref optimization/cls_basic.py:396). */
int pam_xpby(void* stream, void* y, const void* x, double beta, int64_t n,
             int dtype);

/* Device-scalar solver fast path.  alpha/beta are 1-element f64 DEVICE
 * buffers written by a prior pam_dot / pam_scalar_* launch on the same
 * stream; scale is a host constant (+-1.0, exact).  Together with the two
 * recurrence-scalar kernels below, a whole CG/CGLS iteration
 * (ref optimization/cls_basic.py:370-404) is launched with a single host
 * synchronization — the stop-test readback of k — instead of one blocking
 * readback per dot/norm. */
/* y += scale * (*alpha) * x */
int pam_axpy_d(void* stream, void* y, const void* x, const void* alpha,
               double scale, int64_t n, int dtype);
/* y = x + scale * (*beta) * y */
int pam_xpby_d(void* stream, void* y, const void* x, const void* beta,
               double scale, int64_t n, int dtype);
/* *out = |num[0] / (den[0] + damp * den[1])| — a = |kold / (q.q + damp^2
 * c.c)|, ref cls_basic.py:379-383 (CG: damp == 0, ref :121-123). */
int pam_scalar_alpha(void* stream, void* out, const void* num,
                     const void* den, double damp);
/* *out = |num[0] / den[0]| — b = k / kold, ref cls_basic.py:394-395. */
int pam_scalar_div(void* stream, void* out, const void* num, const void* den);

/* Complex element-wise ops (interleaved storage).  add/sub/neg/fill and
 * real-alpha axpy/xpby on complex arrays are the REAL kernels above on the
 * 2n-float view (the solvers' a,b scalars are real, ref cls_basic.py:389).
 * These cover the truly complex cases (ref DistributedArray.py:661-683
 * multiply, :840-854 conj). */
int pam_cmul(void* stream, void* y, const void* a, const void* b, int64_t n,
             int dtype);
int pam_cscale(void* stream, void* y, const void* x, double alpha_re,
               double alpha_im, int64_t n, int dtype);
int pam_conj(void* stream, void* y, const void* x, int64_t n, int dtype);

/* Thresholding for ISTA/FISTA (pylops _softthreshold/_hardthreshold/
 * _halfthreshold formulas, imported by ref optimization/cls_sparsity.py:10;
 * half = the published Xu et al. 2012 L1/2 prox, see pam.hip).
 * kind: 0 = soft, 1 = hard, 2 = half.  In-place safe (y may equal x).
 * NaN: kind 0 returns NaN for a NaN input on real dtypes too, as NumPy's
 * sign(x) * maximum(|x| - t, 0) does (the complex soft branch and kind 2
 * propagate it through their products); finite inputs are unaffected. */
int pam_thresh(void* stream, void* y, const void* x, int64_t n, int kind,
               double thresh, int dtype);

/* ------------------------------------------------------------------ *
 * Reductions (wavefront-shuffle + LDS tree, deterministic tree shape for
 * a given n — fixed partial count, fixed combine order).
 * `ws` is a device float64 scratch of >= pam_reduce_ws_elems() elements;
 * `out` is a 1-element float64 device buffer (the caller allreduces it
 * across ranks, replacing ref Distributed.py:35-112).
 * ------------------------------------------------------------------ */
/* out = sum(x[i] * y[i]) in float64.
 * Replaces the local part of DistributedArray.dot (ref :685-717). */
int pam_dot(void* stream, const void* x, const void* y, int64_t n, void* ws,
            void* out, int dtype);

/* out = sum(x[i] * y[i]) for complex arrays (conjx != 0: vdot,
 * conj(x)*y); `out` is a 2-element float64 device buffer (re, im) and
 * `ws` needs 2*pam_reduce_ws_elems() float64 elements.
 * Replaces the complex branch of DistributedArray.dot (ref :685-717). */
int pam_cdot(void* stream, const void* x, const void* y, int64_t n,
             int conjx, void* ws, void* out, int dtype);

/* Local part of DistributedArray.norm / _compute_vector_norm
 * (ref :719-838).  op: 0 = sum(|x^p|) (float_power semantics, ref :786),
 * 1 = max(|x|), 2 = min(|x|), 3 = count_nonzero.  Complex dtypes reduce
 * over |z| (|z^p| == |z|^p for real p).
 * NaN: ops 1 and 2 return NaN if any element is NaN, as np.max(np.abs(x))
 * and np.min do (every combine of the tree propagates it); op 0 returns
 * NaN through the sum and op 3 counts a NaN as nonzero.  This holds for
 * the LOCAL block: the caller's cross-rank max / min allreduce is RCCL's,
 * and whether that propagates NaN is RCCL's behaviour, not this
 * library's.
 * n == 0: x (and y of pam_dot / pam_cdot) is not read and may be NULL;
 * out = 0, 0, +inf, 0 for ops 0..3 and 0 for the dot products. */
int pam_norm_local(void* stream, const void* x, int64_t n, int op, double p,
                   void* ws, void* out, int dtype);

/* ------------------------------------------------------------------ *
 * L2,1 group operators — isotropic total variation.  The group at index
 * i is (x_0[i], ..., x_{ncomp-1}[i]): the components of a stacked array
 * (e.g. the output of MPIGradient) travel as PAM_GROUP_MAX pointer slots,
 * the unused ones NULL.  pyproximal's L21 prox / Euclidean-ball
 * projection, applied across components without stacking them.
 *
 * pam_group_shrink, one pass:
 *   v_c[i] = a_c[i]                     (all b NULL)
 *   v_c[i] = a_c[i] + beta * b_c[i]     (two roundings: bitwise equal to
 *                                        pam_scale followed by pam_add)
 *   rho    = sqrt(sum_c |v_c[i]|^2)     (c ascending, in the array's real
 *                                        type; complex: re^2 + im^2)
 *   mode 0: s = rho > thresh ? (rho - thresh) / rho : 0
 *           — the prox of thresh * ||.||_{2,1}
 *   mode 1: s = rho > thresh ? thresh / rho : 1
 *           — projection on the per-point L2 ball, its Moreau dual
 *   y_c[i] = v_c[i] * s                 (a zero group gives zeros)
 * y_c may alias a_c.  n counts elements (complex pairs for complex
 * dtypes).  PAM_EARG: ncomp outside [1, PAM_GROUP_MAX], a NULL among the
 * first ncomp y / a, b partly NULL, n < 0, thresh < 0; PAM_EOP: mode not
 * 0 or 1; all checked before anything is launched.
 *
 * pam_group_norm: out[0] = sum_i sqrt(sum_c |x_c[i]|^2), accumulated in
 * float64 on pam_dot's deterministic tree (`ws`: pam_reduce_ws_elems()
 * float64 elements); 0 for n == 0.
 * ------------------------------------------------------------------ */
#define PAM_GROUP_MAX 4
int pam_group_shrink(void* stream, int mode, int64_t ncomp,
                     void* y0, void* y1, void* y2, void* y3,
                     const void* a0, const void* a1, const void* a2,
                     const void* a3,
                     const void* b0, const void* b1, const void* b2,
                     const void* b3,
                     double beta, int64_t n, double thresh, int dtype);
int pam_group_norm(void* stream, int64_t ncomp,
                   const void* x0, const void* x1, const void* x2,
                   const void* x3,
                   int64_t n, void* ws, void* out, int dtype);

/* ------------------------------------------------------------------ *
 * Fused finite-difference stencils along axis 0 of a SCATTER-partitioned
 * array.  One kernel per (operator, kind, direction): no materialized
 * ghost concatenation (the reference copies the whole array per apply,
 * ref DistributedArray.py:974,992-994,1028).
 *
 * Replaces MPIFirstDerivative._matvec_* and ._rmatvec_*
 * (ref basicoperators/FirstDerivative.py:141-318) and
 * MPISecondDerivative (ref basicoperators/SecondDerivative.py:124-256).
 *
 * Layout: x, y are [nloc, m] row-major (m = prod(dims[1:]) elements);
 * gf/gb hold pam_fd_halo_width(op) neighbour planes ([w, m]; gf = last
 * planes of rank-1, gb = first planes of rank+1; may be NULL at the
 * global edges).  row0 = global row of local row 0, nglob = dims[0].
 * coeff = 1/sampling (first derivative) or 1/sampling^2 (second).
 *
 * op codes:
 *   0 fd1 forward  matvec   1 fd1 forward  rmatvec
 *   2 fd1 backward matvec   3 fd1 backward rmatvec
 *   4 fd1 cent3    matvec   5 fd1 cent3    rmatvec
 *   6 fd1 cent5    matvec   7 fd1 cent5    rmatvec
 *   8 fd2 forward  matvec   9 fd2 forward  rmatvec
 *  10 fd2 backward matvec  11 fd2 backward rmatvec
 *  12 fd2 centered matvec  13 fd2 centered rmatvec
 *
 * Arithmetic, per output, in the block's type T: acc = 0; for each term of
 * the op that is active on global row g, acc += T(c_t) * x[g + off_t] (the
 * product rounded, then the sum); with edge the fix-up of the row; last
 * acc *= T(coeff).  All three kernels and pam_fd_serial share it bit for
 * bit.
 *
 * Shortest axis.  With edge != 0 the fix-ups of the centered ops read rows
 * next to either end of the axis, which must exist:
 *   ops 4, 5          nglob >= 2   (rows 1 and N-2)
 *   ops 6, 7, 12, 13  nglob >= 3   (rows 2 and N-3)
 *   every other op, and edge == 0: nglob >= 1
 * pam_fd_apply (nglob) and pam_fd_serial (d) return PAM_EARG on a shorter
 * axis, before anything is launched; the reference raises IndexError there.
 *
 * Ops 6/7 at N == 3 with edge: op 7 is NOT the transpose of op 6.  The
 * matvec overwrites row 1 twice (y[1] and y[-2] are one row), the rmatvec
 * adds both fix-ups: its matrix is [[-1,-1,0],[1,0,-1],[0,1,1]] where the
 * transpose has -0.5 at [0,1] and 0.5 at [2,1].  This is the reference's
 * own slice algebra, kept for parity; every other (op, edge, N) pair is an
 * exact transpose pair.
 *
 * PAM_EOP: op outside 0..13; PAM_EDTYPE: dtype not PAM_F64 / PAM_F32 (a
 * complex block runs as its real view, m doubled); PAM_EARG: nloc < 0,
 * m <= 0, rbegin < 0, rend > nloc, or the axis too short.
 * ------------------------------------------------------------------ */
int64_t pam_fd_halo_width(int op);
/* rbegin/rend restrict the computed LOCAL row range [rbegin, rend) so the
 * interior (halo-independent) rows can be launched concurrently with the
 * RCCL halo exchange and the boundary rows after it completes. */
int pam_fd_apply(void* stream, int op, int edge, const void* x,
                 const void* gf, const void* gb, void* y, int64_t nloc,
                 int64_t m, int64_t row0, int64_t nglob, int64_t rbegin,
                 int64_t rend, double coeff, int dtype);
/* Which kernel pam_fd_apply runs for a launch of nrows = rend - rbegin rows
 * of m elements (host-side query, no GPU work): 0 row-parallel, 1 rolling
 * window, 2 row band.  aligned16 != 0 iff x, y and the non-NULL ghost
 * planes are all 16-byte aligned.  Honours the PAM_FD_* environment
 * selectors exactly as the launch does (PAM_FD_BAND is re-read per call).
 * pam_fd_band_rows: output rows per thread of the row-band kernel. */
int pam_fd_variant(int dtype, int64_t m, int64_t nrows, int aligned16);
int64_t pam_fd_band_rows(void);

/* Serial non-stationary 1-D convolution along axis d of [batch, d, m]
 * (the local operator of MPINonStationaryConvolve1D's Halo sandwich,
 * ref signalprocessing/NonStatConvolve1d.py:129-168): filters hs[nf][hsize]
 * anchored at oh + q*dh, linearly interpolated per position, clamped at
 * the ends.  forward != 0: y[n] = sum_t x[n+hh-t] h_{n+hh-t}[t];
 * adjoint: y[n] = sum_t x[n-hh+t] h_n[t]. */
int pam_nsconv(void* stream, int forward, const void* x, void* y,
               const void* hs, int64_t batch, int64_t d, int64_t m,
               int64_t nf, int64_t hsize, double oh, double dh, int dtype);

/* Stationary 1-D convolution along axis d of [batch, d, m] with nh real
 * taps h, 0 <= offset < nh the tap at lag zero (pylops Convolve1D; with
 * deriv the implicit pylops PoststackLinearModelling, one pass, no
 * intermediate in HBM):
 *   adjoint == 0: y[b,n,j] = sum_k h[k] * v[b, n-k+offset, j]
 *   adjoint != 0: y[b,n,j] = sum_k h[k] * x[b, n+k-offset, j]
 * terms whose sample index leaves [0, d) are skipped (zero padding, no
 * wrap-around).  acc starts at 0, k ascends, every tap is one rounded
 * multiply and one rounded add in the block's real type, the result is
 * stored unscaled.
 * deriv: 0 none (v = x); 1 centered, 2 forward first derivative with
 * edge = 0, coeff = 1 — pam_fd_serial ops 4/5 and 0/1.  Forward is C(Dx)
 * (v = Dx), adjoint D^T(C^T x), bit for bit what pam_fd_serial and
 * pam_conv1d(deriv = 0) give in that order.
 * x and y must not alias (every output reads nh inputs).  dtype PAM_F64 or
 * PAM_F32; a complex block with real taps runs as its real view (m -> 2m).
 * PAM_EARG: batch, d, m or nh <= 0, offset outside [0, nh), a NULL
 * pointer; PAM_EOP: deriv outside 0..2; PAM_EDTYPE otherwise; all checked
 * before anything is launched.
 *
 * pam_conv1d_variant: the kernel pam_conv1d runs for that block (host-side
 * query): 0 plain (one thread per output), 1 trace (a run of flattened
 * (n, j) outputs and its halo staged in LDS; m small), 2 column (rows x
 * columns tile in LDS, a register window along d; m large).
 * PAM_CONV_VARIANT=0|1|2, re-read per call, forces a variant where it is
 * valid; a tiled variant whose halo ((nh + 1) * m samples for 1, nh + 1
 * rows for 2) does not fit the LDS budget falls back to 0, and the query
 * says so.
 * pam_conv1d_tile_d / _tile_m: what one workgroup owns — variant 2:
 * tile_d rows of tile_m columns; variant 1: tile_d consecutive flattened
 * outputs of one batch (tile_d rows when m == 1; tile_m is 1, a run is
 * not aligned to columns); 0 for variant 0 and where variant 2 does not
 * fit. */
int pam_conv1d(void* stream, int adjoint, const void* x, void* y,
               const void* h, int64_t batch, int64_t d, int64_t m,
               int64_t nh, int64_t offset, int deriv, int dtype);
int pam_conv1d_variant(int dtype, int64_t d, int64_t m, int64_t nh);
int64_t pam_conv1d_tile_d(int variant, int dtype, int64_t nh);
int64_t pam_conv1d_tile_m(int variant, int dtype);

/* Kinematic Kirchhoff demigration / migration: the traveltime spread and
 * gather of pylops Kirchhoff with dynamic = False and wavfilter = False
 * (what pylops LSM(..., mode = "analytic") builds; the per-rank operator of
 * the reference's tutorials/lsm.py).  pylops' Kirchhoff is
 *   Convolve1D((ns * nr, nt), wav, offset = wavcenter, axis = -1) o spread;
 * the wavelet stage is pam_conv1d, this entry point is the spread and its
 * adjoint.
 *
 * Model m: ni image points, (nx, nz) or (ny, nx, nz) flattened in C order.
 * Data d: [ns, nr, nt], trace k = is * nr + ir, time axis starting at 0.
 * Tables qs [ns, ni] and qr [nr, ni]: source-to-point and point-to-receiver
 * traveltimes in units of SAMPLES, trace-major (lanes run over i and the
 * loads coalesce): qs[is, i] = trav_srcs[i, is] / dt for pylops' tables
 * trav_srcs (ni, ns) in seconds, qr likewise.  Adding two tables that were
 * divided by dt once, instead of dividing the sum per pair as pylops'
 * (ts + tr) / dt does, is a deliberate deviation by one rounding of q; it
 * is harmless because linear interpolation is continuous across a sample
 * boundary: a q that lands an ulp on the other side of an integer moves a
 * weight of about one ulp between two neighbouring samples.
 *
 * Per pair (k, i), everything in the block's type T:
 *   q = qs[is, i] + qr[ir, i],  it = floor(q),  w = q - it
 * the pair contributes iff 0 <= it < nt - 1; a NaN, infinite or negative q
 * fails that test, is skipped and indexes nothing.
 *   adjoint == 0 (spread, demigration):
 *     d[k, it] += m[i] * (1 - w);  d[k, it + 1] += m[i] * w
 *     every sample that receives nothing is written as 0: d needs no
 *     zeroing by the caller.
 *   adjoint != 0 (gather, migration):
 *     mig[i] = sum_k ((1 - w) * d[k, it]) + (w * d[k, it + 1]), written
 *     to m.
 *
 * Reproducibility.  The adjoint is pinned: acc = 0, traces ascending,
 * term = ((1 - w) * d0) + (w * d1) with each operation rounded once,
 * acc += term; where the launch splits the traces, every run of
 * pam_kirch_chunk consecutive traces is summed so from 0 and the partial
 * sums are added in ascending order — a NumPy loop given that chunk
 * reproduces every bit.  The forward is NOT: a workgroup sums a trace
 * window in LDS (in float64 for either T) with float adds whose order
 * depends on the schedule, so a sample is the sum of its n products
 * m[i] * (1 - w) or m[i] * w, each rounded in T, in SOME order, rounded to
 * T when written: within (n + 2) eps_T sum |m[i]| weight of the exact
 * value.  It is the first entry point of this library that is not
 * reproducible bit for bit; two runs of one launch were seen to differ in
 * the last bits on MI355X.  No float atomic reaches global memory and no
 * two workgroups add to one destination.
 *
 * ws: device scratch of pam_kirch_ws_elems elements of T (0: may be NULL).
 * m and d must not share memory.  dtype PAM_F64 or PAM_F32.
 * PAM_EARG: ns, nr or ni <= 0, nt < 2, a NULL m / d / qs / qr, ws NULL
 * where elements are needed, m and d overlapping; PAM_EDTYPE otherwise;
 * all checked before anything is launched.
 *
 * Host-side queries (no GPU work; each honours the environment exactly as
 * the launch does, re-read per call):
 * pam_kirch_points: image points one workgroup of the adjoint owns.
 * pam_kirch_chunk: traces per partial sum of the adjoint for that block —
 *   a fixed count where the traces are split over workgroups (few image
 *   points), ns * nr where they are not.  PAM_KIRCH_SPLIT=0|1 forces
 *   either.
 * pam_kirch_variant: the adjoint's body, 0 samples gathered from global
 *   memory, 1 each trace staged in LDS first (0 where a trace does not fit
 *   the LDS budget).  PAM_KIRCH_STAGE=0|1 forces either.
 * pam_kirch_window: samples W of the time window one workgroup of the
 *   forward owns: nt where the traces alone fill the chip, shorter with
 *   few traces, at most the LDS budget (8192 samples: the window is kept
 *   in float64).  PAM_KIRCH_WINDOW=W forces it (1 <= W <= budget; nt if
 *   smaller). */
int pam_kirch(void* stream, int adjoint, void* m, void* d, const void* qs,
              const void* qr, void* ws, int64_t ns, int64_t nr, int64_t ni,
              int64_t nt, int dtype);
int64_t pam_kirch_ws_elems(int adjoint, int64_t ns, int64_t nr, int64_t ni,
                           int64_t nt, int dtype);
int64_t pam_kirch_points(void);
int64_t pam_kirch_chunk(int64_t ns, int64_t nr, int64_t ni, int64_t nt,
                        int dtype);
int pam_kirch_variant(int64_t ns, int64_t nr, int64_t ni, int64_t nt,
                      int dtype);
int64_t pam_kirch_window(int64_t ns, int64_t nr, int64_t ni, int64_t nt,
                         int dtype);

/* Serial (single-rank) stencil along an arbitrary axis: the block is
 * viewed as [batch, d, m] with the derivative along d.  The local
 * operators inside MPIBlockDiag for Gradient/Laplacian axes >= 1
 * (ref basicoperators/Gradient.py:101-118, Laplacian.py:98-126, which
 * wrap serial pylops First/SecondDerivative). */
int pam_fd_serial(void* stream, int op, int edge, const void* x, void* y,
                  int64_t batch, int64_t d, int64_t m, double coeff,
                  int dtype);

/* ------------------------------------------------------------------ *
 * Dense GEMV: y = A @ x (trans=0) or y = A^T @ x (trans=1) for a
 * row-major [nr, nc] matrix resident in HBM.
 *
 * The local apply of a dense operator inside MPIBlockDiag
 * (ref basicoperators/BlockDiag.py:122-144 calling a serial dense
 * MatrixMult per rank, as in examples/plot_cgls.py:30-33) — HBM-bound
 * matrix read, wave-per-row (trans=0) or column-tile partials with a
 * deterministic chunk combine (trans=1; `ws` is a float64 device scratch
 * of pam_gemv_ws_elems(nr, nc) elements, unused for trans=0).
 * ------------------------------------------------------------------ */
int64_t pam_gemv_ws_elems(int64_t nr, int64_t nc);
int pam_gemv(void* stream, int trans, const void* A, const void* x, void* y,
             int64_t nr, int64_t nc, void* ws, int dtype);

/* ------------------------------------------------------------------ *
 * Panel GEMM: C = A @ B (accumulate != 0: C += A @ B) for row-major
 * A [M,K] (lda), B [K,N] (ldb), C [M,N] (ldc).  The leading dimensions
 * count elements between the starts of consecutive rows: lda >= K,
 * ldb >= N and ldc >= N are required (PAM_EARG otherwise, nothing is
 * launched); the ld - row padding is never read and never written.
 * K == 0 is an empty sum: C is zeroed, or with accumulate left as it is.
 * PAM_EARG also for M <= 0, N <= 0, K < 0 or a NULL pointer.
 *
 * The local panel product of MPIMatrixMult — block kind
 * (ref basicoperators/MatrixMult.py:369-372 `ncp.matmul(A_local,
 * X_local)`) and the SUMMA accumulation step (ref :661-668
 * `Y_local += ncp.dot(Atemp, Xtemp)`) — on MFMA matrix cores:
 * v_mfma_f32_32x32x2_f32 (exact f32) / v_mfma_f64_16x16x4_f64.
 *
 * pam_transpose materializes A^T for the adjoint panels
 * (ref MatrixMult.py:416,737 `A.T.conj()`; real dtypes).
 * ------------------------------------------------------------------ */
int pam_gemm(void* stream, const void* A, const void* B, void* C, int64_t M,
             int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc,
             int accumulate, int dtype);
int pam_transpose(void* stream, const void* A, void* At, int64_t nr,
                  int64_t nc, int dtype);

/* Batched complex GEMM: for b in [0, batch):
 *   C_b (+)= op(A_b) @ B_b  with op = N (opa=0) or conjugate-transpose
 *   (opa=1; then A_b is [K, M]); accumulate != 0 adds into C.
 * A_b = A + b*strideA etc. (strides in ELEMENTS = complex pairs); each
 * A_b, B_b, C_b is dense (leading dimension = its row length).  The
 * strides of the inputs may be 0 (one A, or one B, for every batch) or
 * leave a gap between batches; strideC must be at least M * N, and the
 * gaps are never read and never written.
 * K == 0 is an empty sum: every C_b is zeroed, or with accumulate left
 * as it is.  PAM_EARG for batch, M or N <= 0, K < 0 or a NULL pointer.
 * The Fredholm1 batched integral kernel (ref signalprocessing/
 * Fredholm1.py:123 `ncp.matmul(G, x)` and :149-156 adjoint), and —
 * with batch=1 — the complex MatrixMult panel product
 * (ref MatrixMult.py:341-427,610-765 complex dtypes). */
int pam_cgemm_batched(void* stream, const void* A, const void* B, void* C,
                      int64_t batch, int64_t M, int64_t N, int64_t K,
                      int64_t strideA, int64_t strideB, int64_t strideC,
                      int opa, int accumulate, int dtype);

/* Batched REAL GEMM: the single-plane analogue of pam_cgemm_batched
 * (op = N or transpose; accumulate != 0 adds into C; strides in
 * elements, K == 0 and the argument errors as there).  The Fredholm1
 * path for float32/float64 kernels (ref Fredholm1.py:123 on a real G)
 * — one z-batched launch instead of a per-slice host loop. */
int pam_gemm_batched(void* stream, const void* A, const void* B, void* C,
                     int64_t batch, int64_t M, int64_t N, int64_t K,
                     int64_t strideA, int64_t strideB, int64_t strideC,
                     int opa, int accumulate, int dtype);

/* Complex <-> real (de)interleave (the MDC chain's real extraction and
 * complex output carrier, ref waveeqprocessing/MDC.py:55-69): unzip
 * writes the n real parts of an interleaved complex array; zip writes n
 * (re, 0) pairs from a real array.  dtype names the COMPLEX type. */
int pam_unzip(void* stream, void* dst_real, const void* src_cplx, int64_t n,
              int dtype);
int pam_zip(void* stream, void* dst_cplx, const void* src_real, int64_t n,
            int dtype);

/* Strided-batched real FFTs along dim 0 of a row-major (nt, m) array
 * (rocFFT native layout — no permute copies; UNSCALED; the MDC chain
 * folds the ortho norms into its kernel).  dtype is the REAL element
 * type.  pam_irfft_strided may clobber its input (rocFFT scratch). */
int pam_rfft_strided(void* stream, const void* in_real, void* out_cplx,
                     int64_t nt, int64_t m, int dtype);
int pam_irfft_strided(void* stream, void* in_cplx, void* out_real,
                      int64_t nt, int64_t m, int dtype);

/* Contiguous-batch variants ((m, nt) layout, transform along the last
 * dim) — the MDC chain transposes itself (pam_unzip_t / pam_zip_t /
 * pam_ctranspose) because rocFFT's strided real plans insert full
 * pack/unpack copies. */
int pam_rfft_contig(void* stream, const void* in_real, void* out_cplx,
                    int64_t nt, int64_t m, int dtype);
int pam_irfft_contig(void* stream, void* in_cplx, void* out_real,
                     int64_t nt, int64_t m, int dtype);

/* Transpose-fused (de)interleave: unzip_t = complex (nt, m) -> real
 * (m, nt) (real parts); zip_t = real (m, nt) -> complex (nt, m) with
 * zero imag.  dtype names the COMPLEX type. */
int pam_unzip_t(void* stream, void* dst_real, const void* src_cplx,
                int64_t nt, int64_t m, int dtype);
int pam_zip_t(void* stream, void* dst_cplx, const void* src_real,
              int64_t nt, int64_t m, int dtype);

/* 256^2-tile f32 GEMM with async global->LDS staging (glds deep
 * pipeline): C (+)= At^T @ B for a K-MAJOR A (At = A^T, [K, M]
 * row-major) and row-major B [K, N], C [M, N].  Fast path only:
 * returns PAM_EARG unless M,N % 256 == 0, K % 32 == 0 and pointers are
 * 16-B aligned — callers fall back to pam_gemm. */
int pam_gemm_kt(void* stream, const void* At, const void* B, void* C,
                int64_t M, int64_t N, int64_t K, int accumulate,
                int dtype);

/* Complex (conj-)transpose on interleaved (re,im) pairs: At = A^T
 * (conj=0) or A^H (conj=1) — the complex MatrixMult adjoint panels
 * (ref MatrixMult.py:416,737 `A.T.conj()`). */
int pam_ctranspose(void* stream, const void* A, void* At, int64_t nr,
                   int64_t nc, int conj, int dtype);

#ifdef __cplusplus
}
#endif
#endif /* PAM_H */

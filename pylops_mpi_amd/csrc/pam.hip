// pam — pylops-mpi hot path, MI355X-native (gfx950/CDNA4) kernels.
//
// Design notes:
//  * Every kernel is HBM-bound (stencils: 16 B/pt algorithmic fp64;
//    axpy: 24 B/pt; dot: 16 B/pt): coalesced 16-byte vector accesses
//    (double2 / float4), block = 256 threads (4 waves of 64).  Launch
//    shapes differ by family: element-wise kernels run one block per 256
//    vector items with no stride loop (grid_1d), reductions a fixed grid of
//    at most NPARTIAL grid-stride blocks, stencils the grid fd_plan picks.
//  * The vector primitives launch through three shared pieces: the
//    dispatchers of launch.h turn dtype, op, kind, ncomp and flags into
//    template arguments, vec_launch is the one "16-byte aligned -> V =
//    VecW<T>, else V = 1" fork, and reduce_launch is the one two-stage
//    deterministic reduction (dot, cdot, norms, group norm).
//  * The finite-difference stencils are FUSED: one pass, reading the
//    neighbour halo planes directly from small exchange buffers instead of
//    materializing a concatenated ghosted copy the way the reference does
//    (ref DistributedArray.py:974,992-994,1028 — an extra full read+write
//    per apply there).
//  * Stencil math is table-driven: each (operator, kind, direction) is a
//    compile-time list of (row offset, coefficient, global-row interval)
//    terms — the closed forms of the reference's slice algebra
//    (ref basicoperators/FirstDerivative.py:141-318,
//     SecondDerivative.py:124-256), verified against the oracle's
//    rank-simulated restatement and dense-transpose adjoints.
//  * Reductions accumulate in float64 with a fixed tree shape for a given
//    n (grid-stride per-thread accumulation -> 64-lane __shfl_down wave
//    reduction -> LDS tree -> fixed-size partial buffer -> one-block
//    deterministic combine), so CGLS traces are reproducible run-to-run.
//    An empty reduction (n == 0) is the combine over zero partials: the
//    result is written by a kernel on the caller's stream, never by a
//    host copy.
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off
//        -fPIC -shared pam.hip -o ../libpam.so
// (-ffp-contract=off: keep mul+add roundings separate so results track the
//  reference NumPy op-for-op at the ulp level.)

#include <math.h>

#include <initializer_list>

#include "launch.h"
#include "fd_defs.h"

#define PAM_ABI_VERSION 1
#define NPARTIAL 1024  // fixed stage-1 partial count cap (determinism)

extern "C" int64_t pam_version(void) { return PAM_ABI_VERSION; }
extern "C" int64_t pam_reduce_ws_elems(void) { return NPARTIAL; }

// ---------------------------------------------------------------------------
// helpers
// ---------------------------------------------------------------------------
static inline int64_t grid_1d(int64_t work) {
  // One block per BLK work items — NO grid-stride looping by default.
  // A/B at the bench size (fp64 axpy, single box): cap=4096 (the old
  // default) 4.52 TB/s, 32768 4.98, 65536 5.14, uncapped 5.78 TB/s
  // (+28%) — the stride loop was the bottleneck, not launch width.
  // (The deterministic dot/norm reductions are unaffected: their
  // stage-1 grid is the fixed NPARTIAL tree, not grid_1d.)
  // PAM_EW_CAP (read once per process) restores a cap for A/Bs.
  static const int64_t cap = env_int("PAM_EW_CAP", 0x7FFFFFFF);
  int64_t g = (work + BLK - 1) / BLK;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return g;
}

// The one vector-or-scalar fork.  Calls f(std::integral_constant<int, V>{})
// with V = VecW<T> (one 16-byte vector per item) when `ok` holds and every
// pointer of `ptrs` is 16-byte aligned (NULL is), else with V = 1; f
// launches and the launch's error code is returned.  The grid is f's to
// choose: the families derive theirs from V in different ways.
template <typename T, typename F>
static int vec_launch(bool ok, std::initializer_list<const void*> ptrs,
                      F&& f) {
  for (const void* p : ptrs) ok = ok && (uintptr_t)p % 16 == 0;
  if (ok) f(std::integral_constant<int, VecW<T>::value>{});
  else f(std::integral_constant<int, 1>{});
  return check(hipGetLastError());
}

// ---------------------------------------------------------------------------
// element-wise kernels (ref DistributedArray.py:605-683 local math)
// EW op codes: 0 fill, 1 neg, 2 add, 3 sub, 4 mul, 5 scale, 6 axpy, 7 xpby
// ---------------------------------------------------------------------------
// one work item: V elements at offset off (a 16-byte vector, or one element)
template <typename T, int OP, int V>
__device__ __forceinline__ void ew_item(T* y, const T* a, const T* b,
                                        T alpha, int64_t off) {
  T va[V], vb[V], vy[V];
  if constexpr (OP != 0) loadv<T, V>(a + off, va);            // all but fill
  if constexpr (OP >= 2 && OP <= 4) loadv<T, V>(b + off, vb);  // binary a,b
  if constexpr (OP >= 6) loadv<T, V>(y + off, vy);             // y & a
#pragma unroll
  for (int k = 0; k < V; ++k) {
    if constexpr (OP == 0) vy[k] = alpha;
    else if constexpr (OP == 1) vy[k] = -va[k];
    else if constexpr (OP == 2) vy[k] = va[k] + vb[k];
    else if constexpr (OP == 3) vy[k] = va[k] - vb[k];
    else if constexpr (OP == 4) vy[k] = va[k] * vb[k];
    else if constexpr (OP == 5) vy[k] = alpha * va[k];
    else if constexpr (OP == 6) vy[k] = vy[k] + alpha * va[k];
    else if constexpr (OP == 7) vy[k] = va[k] + alpha * vy[k];
  }
  storev<T, V>(y + off, vy);
}

template <typename T, int OP, int V>
__device__ __forceinline__ void ew_body(T* __restrict__ y,
                                        const T* __restrict__ a,
                                        const T* __restrict__ b,
                                        T alpha, int64_t n) {
  const int64_t nv = n / V;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = gid; i < nv; i += stride)
    ew_item<T, OP, V>(y, a, b, alpha, i * V);
  for (int64_t i = nv * V + gid; i < n; i += stride)  // scalar tail
    ew_item<T, OP, 1>(y, a, b, alpha, i);
}

template <typename T, int OP, int V>
__global__ void __launch_bounds__(BLK) ew_kernel(T* __restrict__ y,
                                                 const T* __restrict__ a,
                                                 const T* __restrict__ b,
                                                 T alpha, int64_t n) {
  ew_body<T, OP, V>(y, a, b, alpha, n);
}

// device-scalar variant: alpha lives in HBM (1-elem f64 written by a prior
// reduction / pam_scalar_* kernel on the same stream) so the CG/CGLS
// recurrence (ref cls_basic.py:370-404) runs with no host round-trip per
// update.  scale is a host constant (+-1.0): (T)(scale * *ap) is exact for
// sign flips, so results are bit-identical to the host-scalar kernels.
template <typename T, int OP, int V>
__global__ void __launch_bounds__(BLK) ewd_kernel(T* __restrict__ y,
                                                  const T* __restrict__ a,
                                                  const double* __restrict__ ap,
                                                  double scale, int64_t n) {
  ew_body<T, OP, V>(y, a, nullptr, (T)(scale * ap[0]), n);
}

// Every element-wise entry point.  DEV: alpha = scale * *ap with ap on the
// device (ewd_kernel), and y, a, ap must not be NULL once n > 0 (an empty
// block has no storage: its pointers may be NULL).
template <int OP, bool DEV = false>
static int ew_launch(int dtype, void* stream, void* y, const void* a,
                     const void* b, const void* ap, double alpha, int64_t n) {
  return with_real(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    if (n < 0) return PAM_EARG;
    if (n == 0) return 0;
    if (DEV && (!y || !a || !ap)) return PAM_EARG;
    return vec_launch<T>(true, {y, a, b}, [&](auto v) {
      constexpr int V = decltype(v)::value;
      const dim3 grid((uint32_t)grid_1d(n / V + 1));
      if constexpr (DEV)
        hipLaunchKernelGGL((ewd_kernel<T, OP, V>), grid, dim3(BLK), 0,
                           (hipStream_t)stream, (T*)y, (const T*)a,
                           (const double*)ap, alpha, n);
      else
        hipLaunchKernelGGL((ew_kernel<T, OP, V>), grid, dim3(BLK), 0,
                           (hipStream_t)stream, (T*)y, (const T*)a,
                           (const T*)b, (T)alpha, n);
    });
  });
}

extern "C" int pam_fill(void* stream, void* y, int64_t n, double value,
                        int dtype) {
  return ew_launch<0>(dtype, stream, y, nullptr, nullptr, nullptr, value, n);
}
extern "C" int pam_neg(void* stream, void* y, const void* x, int64_t n,
                       int dtype) {
  return ew_launch<1>(dtype, stream, y, x, nullptr, nullptr, 0.0, n);
}
extern "C" int pam_add(void* stream, void* y, const void* a, const void* b,
                       int64_t n, int dtype) {
  return ew_launch<2>(dtype, stream, y, a, b, nullptr, 0.0, n);
}
extern "C" int pam_sub(void* stream, void* y, const void* a, const void* b,
                       int64_t n, int dtype) {
  return ew_launch<3>(dtype, stream, y, a, b, nullptr, 0.0, n);
}
extern "C" int pam_mul(void* stream, void* y, const void* a, const void* b,
                       int64_t n, int dtype) {
  return ew_launch<4>(dtype, stream, y, a, b, nullptr, 0.0, n);
}
extern "C" int pam_scale(void* stream, void* y, const void* x, double alpha,
                         int64_t n, int dtype) {
  return ew_launch<5>(dtype, stream, y, x, nullptr, nullptr, alpha, n);
}
extern "C" int pam_axpy(void* stream, void* y, const void* x, double alpha,
                        int64_t n, int dtype) {
  return ew_launch<6>(dtype, stream, y, x, nullptr, nullptr, alpha, n);
}
extern "C" int pam_xpby(void* stream, void* y, const void* x, double beta,
                        int64_t n, int dtype) {
  return ew_launch<7>(dtype, stream, y, x, nullptr, nullptr, beta, n);
}

// ---------------------------------------------------------------------------
// device-scalar solver fast path (ref optimization/cls_basic.py:370-404):
// axpy/xpby whose scalar is read from device memory, plus the two tiny
// recurrence-scalar kernels.  Together these let a whole CG/CGLS iteration
// be launched with a single host synchronization (the stop-test readback).
// ---------------------------------------------------------------------------
// y += scale * (*alpha) * x
extern "C" int pam_axpy_d(void* stream, void* y, const void* x,
                          const void* alpha, double scale, int64_t n,
                          int dtype) {
  return ew_launch<6, true>(dtype, stream, y, x, nullptr, alpha, scale, n);
}

// y = x + scale * (*beta) * y
extern "C" int pam_xpby_d(void* stream, void* y, const void* x,
                          const void* beta, double scale, int64_t n,
                          int dtype) {
  return ew_launch<7, true>(dtype, stream, y, x, nullptr, beta, scale, n);
}

// *out = |num[0] / (den[0] + damp * den[1])| — the CG/CGLS step scalars
// a = |kold / (q.q + damp^2 c.c)| (ref cls_basic.py:379-383; CG a with
// damp==0, ref :121-123).  |x/y| == |x|/|y| in IEEE, so this matches the
// reference's np.abs placement for the non-negative numerators involved.
__global__ void scalar_alpha_kernel(double* __restrict__ out,
                                    const double* __restrict__ num,
                                    const double* __restrict__ den,
                                    double damp) {
  out[0] = fabs(num[0] / (den[0] + damp * den[1]));
}

// *out = |num[0] / den[0]| — b = k/kold (ref cls_basic.py:394-395)
__global__ void scalar_div_kernel(double* __restrict__ out,
                                  const double* __restrict__ num,
                                  const double* __restrict__ den) {
  out[0] = fabs(num[0] / den[0]);
}

extern "C" int pam_scalar_alpha(void* stream, void* out, const void* num,
                                const void* den, double damp) {
  if (!out || !num || !den) return PAM_EARG;
  hipLaunchKernelGGL(scalar_alpha_kernel, dim3(1), dim3(1), 0,
                     (hipStream_t)stream, (double*)out, (const double*)num,
                     (const double*)den, damp);
  return check(hipGetLastError());
}

extern "C" int pam_scalar_div(void* stream, void* out, const void* num,
                              const void* den) {
  if (!out || !num || !den) return PAM_EARG;
  hipLaunchKernelGGL(scalar_div_kernel, dim3(1), dim3(1), 0,
                     (hipStream_t)stream, (double*)out, (const double*)num,
                     (const double*)den);
  return check(hipGetLastError());
}

// ---------------------------------------------------------------------------
// complex element-wise (interleaved re,im).  EWC op: 0 cmul, 1 cscale, 2 conj
// (ref DistributedArray.py:661-683, :840-854).  add/neg/real-axpy on complex
// arrays reuse the real kernels on the 2n view (solver scalars are real).
// ---------------------------------------------------------------------------
template <typename T, int OP>
__global__ void __launch_bounds__(BLK) ewc_kernel(T* __restrict__ y,
                                                  const T* __restrict__ a,
                                                  const T* __restrict__ b,
                                                  T ar, T ai, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    const T xr = a[2 * i], xi = a[2 * i + 1];
    T zr, zi;
    if constexpr (OP == 0) {
      const T br = b[2 * i], bi = b[2 * i + 1];
      zr = xr * br - xi * bi;
      zi = xr * bi + xi * br;
    } else if constexpr (OP == 1) {
      zr = xr * ar - xi * ai;
      zi = xr * ai + xi * ar;
    } else {
      zr = xr;
      zi = -xi;
    }
    y[2 * i] = zr;
    y[2 * i + 1] = zi;
  }
}

template <int OP>
static int ewc_launch(int dtype, void* stream, void* y, const void* a,
                      const void* b, double ar, double ai, int64_t n) {
  return with_cplx(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    if (n < 0) return PAM_EARG;
    if (n == 0) return 0;
    hipLaunchKernelGGL((ewc_kernel<T, OP>), dim3(grid_1d(n)), dim3(BLK), 0,
                       (hipStream_t)stream, (T*)y, (const T*)a, (const T*)b,
                       (T)ar, (T)ai, n);
    return check(hipGetLastError());
  });
}

extern "C" int pam_cmul(void* stream, void* y, const void* a, const void* b,
                        int64_t n, int dtype) {
  return ewc_launch<0>(dtype, stream, y, a, b, 0.0, 0.0, n);
}
extern "C" int pam_cscale(void* stream, void* y, const void* a,
                          double alpha_re, double alpha_im, int64_t n,
                          int dtype) {
  return ewc_launch<1>(dtype, stream, y, a, nullptr, alpha_re, alpha_im, n);
}
extern "C" int pam_conj(void* stream, void* y, const void* a, int64_t n,
                        int dtype) {
  return ewc_launch<2>(dtype, stream, y, a, nullptr, 0.0, 0.0, n);
}

// ---------------------------------------------------------------------------
// complex <-> real (de)interleave: the MDC chain's real extraction
// feeding rfft (ref MDC.py:55-69 — pylops' real FFT discards imag) and
// the real->complex(0 imag) output carrier.  torch's strided
// elementwise copies run these at ~3.7 TB/s (r02 MDC kernel trace); the
// vectorized forms below stream at the plain copy rate.  unzip reads V
// complex pairs per lane and writes V reals; zip the reverse.
// ---------------------------------------------------------------------------
template <typename T, int V>
__global__ void __launch_bounds__(BLK) unzip_kernel(
    T* __restrict__ dst, const T* __restrict__ src, int64_t n) {
  const int64_t nv = n / V;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t iv = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; iv < nv;
       iv += stride) {
    T pair[2 * V], out[V];
    loadv<T, V>(src + 2 * iv * V, pair);
    loadv<T, V>(src + 2 * iv * V + V, pair + V);
#pragma unroll
    for (int k = 0; k < V; ++k) out[k] = pair[2 * k];
    storev<T, V>(dst + iv * V, out);
  }
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = nv * V + gid; i < n; i += stride)
    dst[i] = src[2 * i];
}

template <typename T, int V>
__global__ void __launch_bounds__(BLK) zip_kernel(
    T* __restrict__ dst, const T* __restrict__ src, int64_t n) {
  const int64_t nv = n / V;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t iv = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; iv < nv;
       iv += stride) {
    T in[V], pair[2 * V];
    loadv<T, V>(src + iv * V, in);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      pair[2 * k] = in[k];
      pair[2 * k + 1] = (T)0;
    }
    storev<T, V>(dst + 2 * iv * V, pair);
    storev<T, V>(dst + 2 * iv * V + V, pair + V);
  }
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = nv * V + gid; i < n; i += stride) {
    dst[2 * i] = src[i];
    dst[2 * i + 1] = (T)0;
  }
}

static int zip_launch(int dtype, void* stream, void* dst, const void* src,
                      int64_t n, bool unzip) {
  return with_cplx(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    if (n < 0) return PAM_EARG;
    if (n == 0) return 0;  // empty arrays have no storage (NULL)
    if (!dst || !src) return PAM_EARG;
    return vec_launch<T>(true, {dst, src}, [&](auto v) {
      constexpr int V = decltype(v)::value;
      hipLaunchKernelGGL((unzip ? unzip_kernel<T, V> : zip_kernel<T, V>),
                         dim3((uint32_t)grid_1d(n / V + 1)), dim3(BLK), 0,
                         (hipStream_t)stream, (T*)dst, (const T*)src, n);
    });
  });
}

extern "C" int pam_unzip(void* stream, void* dst_real, const void* src_cplx,
                         int64_t n, int dtype) {
  return zip_launch(dtype, stream, dst_real, src_cplx, n, true);
}

extern "C" int pam_zip(void* stream, void* dst_cplx, const void* src_real,
                       int64_t n, int dtype) {
  return zip_launch(dtype, stream, dst_cplx, src_real, n, false);
}

// ---------------------------------------------------------------------------
// transpose-fused (de)interleave for the MDC chain's FFT layout (r02):
// rocFFT's strided real plans insert their own full pack/unpack copy
// kernels (~500 us/direction at the cfg5 shape, r02 trace), so the
// chain transposes to the time-contiguous layout itself — fused with
// the complex<->real conversion it already needs, at the LDS-tiled
// transpose rate.  unzipT: complex (nt, m) -> real (m, nt) (real parts
// only).  zipT: real (m, nt) -> complex (nt, m) with zero imag.
// 32x32 LDS tiles (+1 pad), 256 threads as 8x32.
// ---------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(BLK) unzipT_kernel(
    T* __restrict__ dst, const T* __restrict__ src, int64_t nt, int64_t m) {
  __shared__ T tile[32][33];
  const int64_t k0 = (int64_t)blockIdx.y * 32;  // time rows
  const int64_t j0 = (int64_t)blockIdx.x * 32;  // columns
  const int tr = threadIdx.x / 32;
  const int tc = threadIdx.x % 32;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t k = k0 + tr + 8 * i;
    if (k < nt && j0 + tc < m)
      tile[tr + 8 * i][tc] = src[2 * (k * m + j0 + tc)];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t j = j0 + tr + 8 * i;
    if (j < m && k0 + tc < nt)
      dst[j * nt + k0 + tc] = tile[tc][tr + 8 * i];
  }
}

template <typename T>
__global__ void __launch_bounds__(BLK) zipT_kernel(
    T* __restrict__ dst, const T* __restrict__ src, int64_t nt, int64_t m) {
  __shared__ T tile[32][33];
  const int64_t j0 = (int64_t)blockIdx.y * 32;  // columns (src rows)
  const int64_t k0 = (int64_t)blockIdx.x * 32;  // time
  const int tr = threadIdx.x / 32;
  const int tc = threadIdx.x % 32;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t j = j0 + tr + 8 * i;
    if (j < m && k0 + tc < nt)
      tile[tr + 8 * i][tc] = src[j * nt + k0 + tc];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t k = k0 + tr + 8 * i;
    if (k < nt && j0 + tc < m) {
      const int64_t off = 2 * (k * m + j0 + tc);
      dst[off] = tile[tc][tr + 8 * i];
      dst[off + 1] = (T)0;
    }
  }
}

// both directions: the tiles of the complex side's columns run along grid.x
// for unzipT and along grid.y for zipT
static int zip_t_launch(int dtype, void* stream, void* dst, const void* src,
                        int64_t nt, int64_t m, bool unzip) {
  if (nt <= 0 || m <= 0 || !dst || !src) return PAM_EARG;
  const uint32_t gm = (uint32_t)((m + 31) / 32);
  const uint32_t gt = (uint32_t)((nt + 31) / 32);
  const dim3 grid = unzip ? dim3(gm, gt) : dim3(gt, gm);
  return with_cplx(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((unzip ? unzipT_kernel<T> : zipT_kernel<T>), grid,
                       dim3(BLK), 0, (hipStream_t)stream, (T*)dst,
                       (const T*)src, nt, m);
    return check(hipGetLastError());
  });
}

extern "C" int pam_unzip_t(void* stream, void* dst_real,
                           const void* src_cplx, int64_t nt, int64_t m,
                           int dtype) {
  return zip_t_launch(dtype, stream, dst_real, src_cplx, nt, m, true);
}

extern "C" int pam_zip_t(void* stream, void* dst_cplx, const void* src_real,
                         int64_t nt, int64_t m, int dtype) {
  return zip_t_launch(dtype, stream, dst_cplx, src_real, nt, m, false);
}

// ---------------------------------------------------------------------------
// thresholding for ISTA/FISTA (the pylops _softthreshold/_hardthreshold
// formulas the reference imports, ref optimization/cls_sparsity.py:10):
//   soft real   : sign(x) * max(|x|-t, 0)
//   soft complex: z * max(|z|-t, 0)/|z|
//   hard        : x * (|x| >= sqrt(2 t))
//   half        : L1/2 prox (Xu et al. 2012, the published formula pylops'
//                 _halfthreshold implements — the EXACT prox of
//                 (t/2)|v|^(1/2), matching ISTA's thresh = eps*alpha*0.5):
//                 for |x| > (54^(1/3)/4) t^(2/3),
//                 y = (2/3) x (1 + cos(2pi/3 - (2/3) acos((t/8)(|x|/3)^-1.5)))
//                 else 0; complex by the magnitude rule.  Pinned by the prox
//                 optimality property test (tests/test_oracle_proximal.py) —
//                 pylops itself is absent from /root/reference.
// kind: 0 soft, 1 hard, 2 half.  In-place safe (y may alias x).
// ---------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T half_factor(T a_, T thresh_) {
  // multiplicative factor of the L1/2 prox at magnitude a (>= 0).
  // Always evaluated in double so the cutoff decision (a discontinuity)
  // and the acos/pow chain agree with the f64 oracle for every dtype.
  const double a = (double)a_, thresh = (double)thresh_;
  const double cut = 0.9449407874211548 * pow(thresh, 2.0 / 3.0);
  if (!(a > cut)) return (T)0;  // 54^(1/3)/4 = 0.944940787421...
  const double phi = acos((thresh / 8.0) * pow(a / 3.0, -1.5));
  return (T)((2.0 / 3.0) *
             (1.0 + cos(2.0 * M_PI / 3.0 - (2.0 / 3.0) * phi)));
}

template <typename T, bool CPLX, int KIND>
__global__ void __launch_bounds__(BLK) thresh_kernel(T* __restrict__ y,
                                                     const T* __restrict__ x,
                                                     T thresh, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    if constexpr (!CPLX) {
      const T v = x[i];
      if constexpr (KIND == 0) {
        const T m = fabs(v) - thresh;
        // NaN in, NaN out (sign(x) * max(|x| - t, 0) in NumPy): m is NaN
        y[i] = m > (T)0 ? copysign(m, v) : (m != m ? m : (T)0);
      } else if constexpr (KIND == 1) {
        y[i] = fabs(v) >= sqrt((T)2 * thresh) ? v : (T)0;
      } else {
        y[i] = v * half_factor(fabs(v), thresh);
      }
    } else {
      const T zr = x[2 * i], zi = x[2 * i + 1];
      const T a = hypot(zr, zi);
      T s;
      if constexpr (KIND == 0) {
        const T m = a - thresh;
        s = (m > (T)0 && a > (T)0) ? m / a : (T)0;
      } else if constexpr (KIND == 1) {
        s = a >= sqrt((T)2 * thresh) ? (T)1 : (T)0;
      } else {
        s = half_factor(a, thresh);
      }
      y[2 * i] = zr * s;
      y[2 * i + 1] = zi * s;
    }
  }
}

extern "C" int pam_thresh(void* stream, void* y, const void* x, int64_t n,
                          int kind, double thresh, int dtype) {
  return with_dtype(dtype, [&](auto t, auto cplx) {
    using T = typename decltype(t)::type;
    constexpr bool CPLX = decltype(cplx)::value;
    if (n < 0) return PAM_EARG;
    if (n == 0) return 0;
    return with_int<0, 2>(kind, PAM_EOP, [&](auto k) {
      hipLaunchKernelGGL((thresh_kernel<T, CPLX, decltype(k)::value>),
                         dim3(grid_1d(n)), dim3(BLK), 0, (hipStream_t)stream,
                         (T*)y, (const T*)x, (T)thresh, n);
      return check(hipGetLastError());
    });
  });
}

// ---------------------------------------------------------------------------
// reductions (ref DistributedArray.py:685-717 dot, :719-838 norms)
// RED codes: 0 dot, 1 powsum |x^p|, 2 max|x|, 3 min|x|, 4 count_nonzero
// ---------------------------------------------------------------------------
// max / min propagate NaN, as np.max(np.abs(x)) does (fmax / fmin return
// the non-NaN operand: a diverged iterate would report a finite inf-norm);
// on |x| >= +0 without NaN they return what fmax / fmin return.
template <int RED>
__device__ __forceinline__ double red_combine(double u, double v) {
  if constexpr (RED == 2) return u != u ? u : ((v != v || v > u) ? v : u);
  else if constexpr (RED == 3) return u != u ? u : ((v != v || v < u) ? v : u);
  else return u + v;
}

// the value of an empty reduction: 0, 0, +inf, 0 for the norm ops
template <int RED> __device__ __forceinline__ double red_init() {
  if constexpr (RED == 2) return 0.0;          // max over |x| >= 0
  else if constexpr (RED == 3) return INFINITY;
  else return 0.0;
}

// 64-lane __shfl_down tree of one wave; the result is valid in lane 0
template <int RED>
__device__ __forceinline__ double wave_reduce(double acc) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    acc = red_combine<RED>(acc, __shfl_down(acc, off, 64));
  return acc;
}

// The fixed tail of every deterministic reduction: wave_reduce -> one LDS
// slot per wave -> thread 0 combines the BLK/64 slots in order.  The result
// is valid in thread 0 only.  All calls in one kernel share the LDS slots:
// a second call needs a __syncthreads() before it.
template <int RED>
__device__ __forceinline__ double block_reduce(double acc) {
  acc = wave_reduce<RED>(acc);
  __shared__ double lds[BLK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    acc = lds[0];
#pragma unroll
    for (int w = 1; w < BLK / 64; ++w) acc = red_combine<RED>(acc, lds[w]);
  }
  return acc;
}

template <typename T, int RED, bool CPLX = false>
__global__ void __launch_bounds__(BLK) reduce_stage1(
    const T* __restrict__ x, const T* __restrict__ y, int64_t n, double p,
    double* __restrict__ partials) {
  double acc = red_init<RED>();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    double v;
    if constexpr (CPLX) {
      // reduce over |z| (norms only; |z^p| == |z|^p for real p)
      const double zr = (double)x[2 * i], zi = (double)x[2 * i + 1];
      if constexpr (RED == 1) {
        // fast paths: pow with a runtime exponent is transcendental-bound
        // (measured 3.4x a dot pass); p==2/p==1 cover every solver norm
        if (p == 2.0) v = zr * zr + zi * zi;
        else if (p == 1.0) v = hypot(zr, zi);
        else v = pow(hypot(zr, zi), p);
      }
      else if constexpr (RED == 2 || RED == 3) v = hypot(zr, zi);
      else v = (zr != 0.0 || zi != 0.0) ? 1.0 : 0.0;
    } else {
      const double xv = (double)x[i];
      if constexpr (RED == 0) v = xv * (double)y[i];
      else if constexpr (RED == 1) {
        // ref :786 float_power; pow(x,2) is correctly rounded == x*x and
        // |pow(x,1)| == |x|, so the fast paths are bit-identical
        if (p == 2.0) v = xv * xv;
        else if (p == 1.0) v = fabs(xv);
        else v = fabs(pow(xv, p));
      }
      else if constexpr (RED == 2 || RED == 3) v = fabs(xv);
      else v = (xv != 0.0) ? 1.0 : 0.0;
    }
    acc = red_combine<RED>(acc, v);
  }
  const double r = block_reduce<RED>(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = r;
}

// One block combines the np stage-1 partials of each of LANES result lanes
// (lane l's partials start at partials + l * NPARTIAL) into out[l].  np == 0
// leaves red_init<RED>(): the empty result.
template <int RED, int LANES>
__global__ void __launch_bounds__(BLK) reduce_stage2(
    const double* __restrict__ partials, int64_t np, double* __restrict__ out) {
  double acc[LANES], r[LANES];
#pragma unroll
  for (int l = 0; l < LANES; ++l) acc[l] = red_init<RED>();
  for (int64_t i = threadIdx.x; i < np; i += BLK) {
#pragma unroll
    for (int l = 0; l < LANES; ++l)
      acc[l] = red_combine<RED>(acc[l], partials[l * NPARTIAL + i]);
  }
#pragma unroll
  for (int l = 0; l < LANES; ++l) {
    if (l > 0) __syncthreads();
    r[l] = block_reduce<RED>(acc[l]);
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int l = 0; l < LANES; ++l) out[l] = r[l];
  }
}

// The one two-stage deterministic reduction.  stage1(grid, s) launches the
// family's stage-1 kernel on min(ceil(n / BLK), NPARTIAL) blocks, each
// writing one partial per result lane into ws; stage 2 combines them into
// out[0..LANES).  n == 0 launches stage 2 alone, which writes the empty
// result: no array is read and nothing blocks the host.  The caller has
// checked its arguments.
template <int RED, int LANES, typename F>
static int reduce_launch(void* stream, int64_t n, void* ws, void* out,
                         F&& stage1) {
  hipStream_t s = (hipStream_t)stream;
  int64_t nb = (n + BLK - 1) / BLK;
  if (nb > NPARTIAL) nb = NPARTIAL;
  if (nb > 0) {
    stage1(dim3((uint32_t)nb), s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL((reduce_stage2<RED, LANES>), dim3(1), dim3(BLK), 0, s,
                     (const double*)ws, nb, (double*)out);
  return check(hipGetLastError());
}

// dot and the norms; x (and y of the dot) may be NULL when n == 0
template <typename T, int RED, bool CPLX>
static int norm_launch(void* stream, const void* x, const void* y, int64_t n,
                       double p, void* ws, void* out) {
  if (n < 0 || !ws || !out) return PAM_EARG;
  if (n > 0 && (!x || (RED == 0 && !y))) return PAM_EARG;
  return reduce_launch<RED, 1>(stream, n, ws, out, [&](dim3 grid,
                                                       hipStream_t s) {
    hipLaunchKernelGGL((reduce_stage1<T, RED, CPLX>), grid, dim3(BLK), 0, s,
                       (const T*)x, (const T*)y, n, p, (double*)ws);
  });
}

// ---- complex dot (out = sum x*y or sum conj(x)*y; 2-double result)
template <typename T, bool CONJX>
__global__ void __launch_bounds__(BLK) cdot_stage1(
    const T* __restrict__ x, const T* __restrict__ y, int64_t n,
    double* __restrict__ pre, double* __restrict__ pim) {
  double ar = 0.0, ai = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    const double xr = (double)x[2 * i];
    const double xi = CONJX ? -(double)x[2 * i + 1] : (double)x[2 * i + 1];
    const double yr = (double)y[2 * i], yi = (double)y[2 * i + 1];
    ar += xr * yr - xi * yi;
    ai += xr * yi + xi * yr;
  }
  const double sr = block_reduce<0>(ar);
  __syncthreads();
  const double si = block_reduce<0>(ai);
  if (threadIdx.x == 0) {
    pre[blockIdx.x] = sr;
    pim[blockIdx.x] = si;
  }
}

extern "C" int pam_cdot(void* stream, const void* x, const void* y, int64_t n,
                        int conjx, void* ws, void* out, int dtype) {
  return with_cplx(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    if (n < 0 || !ws || !out) return PAM_EARG;
    if (n > 0 && (!x || !y)) return PAM_EARG;
    double* pre = (double*)ws;  // re partials; im partials NPARTIAL further
    return reduce_launch<0, 2>(stream, n, ws, out, [&](dim3 grid,
                                                       hipStream_t s) {
      with_bool(conjx != 0, [&](auto cj) {
        hipLaunchKernelGGL((cdot_stage1<T, decltype(cj)::value>), grid,
                           dim3(BLK), 0, s, (const T*)x, (const T*)y, n, pre,
                           pre + NPARTIAL);
      });
    });
  });
}

extern "C" int pam_dot(void* stream, const void* x, const void* y, int64_t n,
                       void* ws, void* out, int dtype) {
  return with_real(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return norm_launch<T, 0, false>(stream, x, y, n, 0.0, ws, out);
  });
}

extern "C" int pam_norm_local(void* stream, const void* x, int64_t n, int op,
                              double p, void* ws, void* out, int dtype) {
  return with_int<0, 3>(op, PAM_EOP, [&](auto o) {  // RED = op + 1
    return with_dtype(dtype, [&](auto t, auto cplx) {
      using T = typename decltype(t)::type;
      return norm_launch<T, decltype(o)::value + 1, decltype(cplx)::value>(
          stream, x, nullptr, n, p, ws, out);
    });
  });
}

// ---------------------------------------------------------------------------
// L2,1 group kernels (isotropic TV): the prox couples the NC component
// arrays of a stacked array at each grid point, so every lane reads the
// same index of up to PAM_GROUP_MAX arrays — one pass, 16 B per
// component-point (24 B with the fused shift), nothing materialized.
//   v_c = a_c (+ beta * b_c),  rho = sqrt(sum_c |v_c|^2),  y_c = v_c * s
//   mode 0 (prox of thresh*||.||_{2,1}): s = rho > thresh ? (rho-thresh)/rho : 0
//   mode 1 (projection on the L2 ball) : s = rho > thresh ? thresh/rho     : 1
// A zero group has rho == 0 <= thresh: s is 0 or 1, never 0/0.
// NC is a template parameter: the component loops unroll, the pointer
// arrays stay in SGPRs and all loads issue before the math.  Complex groups
// span the (re, im) of one element, so complex arrays are NOT launched as
// their real view (cf. thresh_kernel's CPLX branch); a 16-B vector holds
// one complex128 or two complex64.  y_c may alias a_c (no __restrict__: an
// item loads everything it needs before it stores).
// ---------------------------------------------------------------------------
template <typename T, int NC>
struct GroupArgs {
  T* y[NC];
  const T* a[NC];
  const T* b[NC];
};

template <typename T, int V, bool VEC>
__device__ __forceinline__ void group_load(const T* p, T* v) {
  if constexpr (VEC) {
    loadv<T, V>(p, v);
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = p[k];
  }
}

template <typename T, int V, bool VEC>
__device__ __forceinline__ void group_store(T* p, const T* v) {
  if constexpr (VEC) {
    storev<T, V>(p, v);
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k) p[k] = v[k];
  }
}

// one work item: V reals (V / E groups) of every component at real offset off
template <typename T, int NC, int E, int V, bool SHIFT, bool VEC>
__device__ __forceinline__ void group_shrink_item(const GroupArgs<T, NC>& P,
                                                  int64_t off, T beta,
                                                  T thresh, int mode) {
  T v[NC][V];
#pragma unroll
  for (int c = 0; c < NC; ++c) group_load<T, V, VEC>(P.a[c] + off, v[c]);
  if constexpr (SHIFT) {
    T w[NC][V];
#pragma unroll
    for (int c = 0; c < NC; ++c) group_load<T, V, VEC>(P.b[c] + off, w[c]);
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const T t = beta * w[c][k];  // pam_scale's rounding ...
        v[c][k] = v[c][k] + t;       // ... then pam_add's
      }
  }
#pragma unroll
  for (int g = 0; g < V / E; ++g) {
    T acc = (T)0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if constexpr (E == 2)
        acc += v[c][2 * g] * v[c][2 * g] + v[c][2 * g + 1] * v[c][2 * g + 1];
      else
        acc += v[c][g] * v[c][g];
    }
    const T rho = sqrt(acc);
    T s;
    if (rho > thresh)
      s = mode ? thresh / rho : (rho - thresh) / rho;
    else
      s = mode ? (T)1 : (T)0;
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int e = 0; e < E; ++e) v[c][g * E + e] = v[c][g * E + e] * s;
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) group_store<T, V, VEC>(P.y[c] + off, v[c]);
}

template <typename T, int NC, bool CPLX, bool SHIFT, bool VEC>
__global__ void __launch_bounds__(BLK) group_shrink_kernel(
    GroupArgs<T, NC> P, T beta, T thresh, int mode, int64_t n) {
  constexpr int E = CPLX ? 2 : 1;                  // reals per element
  constexpr int V = VEC ? VecW<T>::value : E;      // reals per work item
  const int64_t nv = (n * E) / V;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = gid; i < nv; i += stride)
    group_shrink_item<T, NC, E, V, SHIFT, VEC>(P, i * V, beta, thresh, mode);
  if constexpr (V > E) {  // scalar tail: elements the vectors do not cover
    for (int64_t i = nv * (V / E) + gid; i < n; i += stride)
      group_shrink_item<T, NC, E, E, SHIFT, false>(P, i * E, beta, thresh,
                                                   mode);
  }
}

// the arguments are checked and n > 0; b is all NULL (no shift) or all set
template <typename T, bool CPLX, int NC>
static int group_shrink_launch(void* stream, int mode, void* const* y,
                               const void* const* a, const void* const* b,
                               double beta, int64_t n, double thresh) {
  GroupArgs<T, NC> P;
  const bool shift = b[0] != nullptr;
  bool aligned = true;
  for (int c = 0; c < NC; ++c) {
    P.y[c] = (T*)y[c];
    P.a[c] = (const T*)a[c];
    P.b[c] = shift ? (const T*)b[c] : nullptr;
    aligned = aligned && ((uintptr_t)y[c] % 16 == 0) &&
              ((uintptr_t)a[c] % 16 == 0) &&
              (!shift || (uintptr_t)b[c] % 16 == 0);
  }
  return vec_launch<T>(aligned, {}, [&](auto v) {
    constexpr int E = CPLX ? 2 : 1;
    constexpr bool VEC = decltype(v)::value > 1;
    const int64_t grid = grid_1d(VEC ? (n * E) / decltype(v)::value + 1 : n);
    with_bool(shift, [&](auto sh) {
      hipLaunchKernelGGL(
          (group_shrink_kernel<T, NC, CPLX, decltype(sh)::value, VEC>),
          dim3((uint32_t)grid), dim3(BLK), 0, (hipStream_t)stream, P, (T)beta,
          (T)thresh, mode, n);
    });
  });
}

extern "C" int pam_group_shrink(void* stream, int mode, int64_t ncomp,
                                void* y0, void* y1, void* y2, void* y3,
                                const void* a0, const void* a1,
                                const void* a2, const void* a3,
                                const void* b0, const void* b1,
                                const void* b2, const void* b3, double beta,
                                int64_t n, double thresh, int dtype) {
  void* const y[PAM_GROUP_MAX] = {y0, y1, y2, y3};
  const void* const a[PAM_GROUP_MAX] = {a0, a1, a2, a3};
  const void* const b[PAM_GROUP_MAX] = {b0, b1, b2, b3};
  // every argument check precedes the first HIP call
  if (ncomp < 1 || ncomp > PAM_GROUP_MAX) return PAM_EARG;
  for (int64_t c = 0; c < ncomp; ++c) {
    if (!y[c] || !a[c]) return PAM_EARG;
    if ((b[c] == nullptr) != (b[0] == nullptr)) return PAM_EARG;
  }
  if (n < 0 || !(thresh >= 0.0)) return PAM_EARG;
  if (mode != 0 && mode != 1) return PAM_EOP;
  return with_dtype(dtype, [&](auto t, auto cplx) {
    using T = typename decltype(t)::type;
    constexpr bool CPLX = decltype(cplx)::value;
    if (n == 0) return 0;
    return with_int<1, PAM_GROUP_MAX>(ncomp, PAM_EARG, [&](auto nc) {
      return group_shrink_launch<T, CPLX, decltype(nc)::value>(
          stream, mode, y, a, b, beta, n, thresh);
    });
  });
}

// out = sum_i sqrt(sum_c |x_c[i]|^2) in float64: stage 1 is pam_dot's fixed
// tree (<= NPARTIAL blocks, grid-stride, wave shuffle, LDS), stage 2 the
// shared deterministic combine.
template <typename T, int NC>
struct GroupIn {
  const T* x[NC];
};

template <typename T, int NC, bool CPLX>
__global__ void __launch_bounds__(BLK) group_norm_stage1(
    GroupIn<T, NC> P, int64_t n, double* __restrict__ partials) {
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    double q = 0.0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if constexpr (CPLX) {
        const double zr = (double)P.x[c][2 * i];
        const double zi = (double)P.x[c][2 * i + 1];
        q += zr * zr + zi * zi;
      } else {
        const double xv = (double)P.x[c][i];
        q += xv * xv;
      }
    }
    acc += sqrt(q);
  }
  const double r = block_reduce<0>(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = r;
}

extern "C" int pam_group_norm(void* stream, int64_t ncomp, const void* x0,
                              const void* x1, const void* x2, const void* x3,
                              int64_t n, void* ws, void* out, int dtype) {
  const void* const x[PAM_GROUP_MAX] = {x0, x1, x2, x3};
  if (ncomp < 1 || ncomp > PAM_GROUP_MAX) return PAM_EARG;
  for (int64_t c = 0; c < ncomp; ++c)
    if (!x[c]) return PAM_EARG;
  if (n < 0 || !ws || !out) return PAM_EARG;
  return with_dtype(dtype, [&](auto t, auto cplx) {
    using T = typename decltype(t)::type;
    constexpr bool CPLX = decltype(cplx)::value;
    return with_int<1, PAM_GROUP_MAX>(ncomp, PAM_EARG, [&](auto nc) {
      constexpr int NC = decltype(nc)::value;
      GroupIn<T, NC> P;
      for (int c = 0; c < NC; ++c) P.x[c] = (const T*)x[c];
      return reduce_launch<0, 1>(stream, n, ws, out, [&](dim3 grid,
                                                         hipStream_t s) {
        hipLaunchKernelGGL((group_norm_stage1<T, NC, CPLX>), grid, dim3(BLK),
                           0, s, P, n, (double*)ws);
      });
    });
  });
}

// ---------------------------------------------------------------------------
// dense GEMV (local apply of MPIBlockDiag dense operators,
// ref basicoperators/BlockDiag.py:122-144).  HBM-bound: the matrix read
// dominates (nr*nc elements, read once).
// ---------------------------------------------------------------------------
#define GEMV_CHUNKS 64  // deterministic row-chunk count for the trans path

extern "C" int64_t pam_gemv_ws_elems(int64_t nr, int64_t nc) {
  (void)nr;
  return GEMV_CHUNKS * nc;
}

// y = A @ x: one 64-lane wave per output row, lanes stride the row with
// 16-B vector loads, wavefront shuffle reduction.
template <typename T, int V>
__global__ void __launch_bounds__(BLK) gemv_n_kernel(
    const T* __restrict__ A, const T* __restrict__ x, T* __restrict__ y,
    int64_t nr, int64_t nc) {
  const int64_t wave = ((int64_t)blockIdx.x * (BLK / 64))
                       + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (BLK / 64);
  const int64_t ncv = nc / V;
  for (int64_t r = wave; r < nr; r += nwaves) {
    const T* __restrict__ row = A + r * nc;
    double acc = 0.0;
    for (int64_t cv = lane; cv < ncv; cv += 64) {
      T a[V], b[V];
      loadv<T, V>(row + cv * V, a);
      loadv<T, V>(x + cv * V, b);
#pragma unroll
      for (int k = 0; k < V; ++k) acc += (double)a[k] * (double)b[k];
    }
    for (int64_t c = ncv * V + lane; c < nc; c += 64)
      acc += (double)row[c] * (double)x[c];
    acc = wave_reduce<0>(acc);
    if (lane == 0) y[r] = (T)acc;
  }
}

// y = A^T @ x, stage 1: block (cb, chunk) accumulates its row chunk into
// partials[chunk*nc + c] — fixed chunk count => deterministic combine.
template <typename T, int V>
__global__ void __launch_bounds__(BLK) gemv_t_stage1(
    const T* __restrict__ A, const T* __restrict__ x,
    double* __restrict__ partials, int64_t nr, int64_t nc) {
  // V consecutive columns per lane => 16-B row reads.  Measured: NO rate
  // change vs the scalar form (4096: 4.59 TB/s either way) — the t-path's
  // gap to the n-kernel is the fixed ~8 us two-stage cost (stage-2 launch
  // + 2 MB of partials), not access width.  Kept: same bits, wider loads.
  const int64_t c0 = ((int64_t)blockIdx.x * BLK + threadIdx.x) * V;
  const int chunk = blockIdx.y;
  const int64_t r0 = (nr * chunk) / GEMV_CHUNKS;
  const int64_t r1 = (nr * (chunk + 1)) / GEMV_CHUNKS;
  if (c0 >= nc) return;
  double acc[V] = {};
  for (int64_t r = r0; r < r1; ++r) {
    T v[V];
    loadv<T, V>(A + r * nc + c0, v);
#pragma unroll
    for (int j = 0; j < V; ++j)
      acc[j] += (double)v[j] * (double)x[r];
  }
#pragma unroll
  for (int j = 0; j < V; ++j)
    partials[(int64_t)chunk * nc + c0 + j] = acc[j];
}

template <typename T>
__global__ void __launch_bounds__(BLK) gemv_t_stage2(
    const double* __restrict__ partials, T* __restrict__ y, int64_t nc) {
  const int64_t c = (int64_t)blockIdx.x * BLK + threadIdx.x;
  if (c >= nc) return;
  double acc = 0.0;
  for (int ch = 0; ch < GEMV_CHUNKS; ++ch)
    acc += partials[(int64_t)ch * nc + c];
  y[c] = (T)acc;
}

// the vector kernels also need whole rows of vectors: nc % VecW<T> == 0
template <typename T>
static int gemv_launch(void* stream, int trans, const void* A, const void* x,
                       void* y, int64_t nr, int64_t nc, void* ws) {
  if (nr <= 0 || nc <= 0 || !A || !x || !y) return PAM_EARG;
  hipStream_t s = (hipStream_t)stream;
  const bool rows_ok = nc % VecW<T>::value == 0;
  if (!trans) {
    int64_t nb = (nr + (BLK / 64) - 1) / (BLK / 64);
    if (nb > 4096) nb = 4096;
    return vec_launch<T>(rows_ok, {A, x}, [&](auto v) {
      hipLaunchKernelGGL((gemv_n_kernel<T, decltype(v)::value>),
                         dim3((uint32_t)nb), dim3(BLK), 0, s, (const T*)A,
                         (const T*)x, (T*)y, nr, nc);
    });
  }
  if (!ws) return PAM_EARG;
  const int rc = vec_launch<T>(rows_ok, {A}, [&](auto v) {
    constexpr int V = decltype(v)::value;
    dim3 g1((uint32_t)((nc / V + BLK - 1) / BLK), GEMV_CHUNKS);
    hipLaunchKernelGGL((gemv_t_stage1<T, V>), g1, dim3(BLK), 0, s,
                       (const T*)A, (const T*)x, (double*)ws, nr, nc);
  });
  if (rc != 0) return rc;
  hipLaunchKernelGGL((gemv_t_stage2<T>),
                     dim3((uint32_t)((nc + BLK - 1) / BLK)), dim3(BLK), 0, s,
                     (const double*)ws, (T*)y, nc);
  return check(hipGetLastError());
}

extern "C" int pam_gemv(void* stream, int trans, const void* A, const void* x,
                        void* y, int64_t nr, int64_t nc, void* ws, int dtype) {
  return with_real(dtype, [&](auto t) {
    return gemv_launch<typename decltype(t)::type>(stream, trans, A, x, y, nr,
                                                   nc, ws);
  });
}

// ---------------------------------------------------------------------------
// fused finite-difference stencils
// (ref FirstDerivative.py:141-318, SecondDerivative.py:124-256 — closed
//  forms of the slice algebra; masks are global-row intervals)
//
// Three kernels, one arithmetic (fd_defs.h fd_row_masked / fd_row_interior),
// chosen per launch by fd_plan: row-parallel (fd_kernel), rolling window
// (fd_roll_kernel, long rows) and row band (fd_band_kernel, mid-size ragged
// shapes).  Measurements behind the rules: DESIGN.md §3 and §8.
// ---------------------------------------------------------------------------

extern "C" int64_t pam_fd_halo_width(int op) {
  switch (op) {
    case 0: case 1: case 2: case 3: case 4: case 5: return 1;
    case 6: case 7: case 8: case 9: case 10: case 11: case 12: case 13:
      return 2;
    default: return PAM_EOP;
  }
}

// rows from either global end that are NOT interior: some term masked
// (lo/hi) or touched by fd_edge (which reaches rows 0..2 / N-3..N-1)
template <int OP>
constexpr int fd_margin() {
  int mg = 3;
  for (int t = 0; t < FDDef<OP>::NT; ++t) {
    if (FDDef<OP>::TERMS[t].lo > mg) mg = FDDef<OP>::TERMS[t].lo;
    if (FDDef<OP>::TERMS[t].hi > mg) mg = FDDef<OP>::TERMS[t].hi;
  }
  return mg;
}

// Interior column trips of one row: U column vectors per trip while U fit,
// all U*NT loads issued before the first store (U*NT 16-B loads in flight
// per thread instead of NT).  Advances jv past what it stored.
template <typename T, int OP, int V, int U>
__device__ __forceinline__ void fd_interior_trips(
    const T* __restrict__ xrow, T* __restrict__ yrow, int64_t m, int64_t mv,
    int64_t cstride, T c, int64_t& jv) {
  constexpr int NR = 2 * FDDef<OP>::W + 1;
  for (; jv + (U - 1) * cstride < mv; jv += U * cstride) {
    T win[U][NR][V];
#pragma unroll
    for (int u = 0; u < U; ++u)
      fd_load_terms<T, OP, V>(xrow + (jv + u * cstride) * V, m, win[u]);
#pragma unroll
    for (int u = 0; u < U; ++u)
      fd_row_interior<T, OP, V, NR>(win[u], c, yrow + (jv + u * cstride) * V,
                                    m);
  }
}

// Row-parallel stencil: one block-row per local row, a grid-stride loop
// over the row's column vectors.  Interior rows — every input row a local
// row of x, every term active, no edge fixup; uniform per block — take the
// unmasked trips (U per trip, then singly); every other row, and the columns
// the trips left, take the masked body.
template <typename T, int OP, int V, int U>
__global__ void __launch_bounds__(BLK) fd_kernel(Rows<T> R, T* __restrict__ y,
                                                 int64_t row0, int64_t N, T c,
                                                 int edge, int64_t rbegin,
                                                 int64_t rend) {
  constexpr int W = FDDef<OP>::W, MG = fd_margin<OP>();
  const int64_t bcol = blockIdx.x;
  const int64_t m = R.m, mv = m / V;
  const int64_t cstride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = rbegin + blockIdx.y; i < rend; i += gridDim.y) {
    const int64_t g = row0 + i;
    T* __restrict__ yrow = y + i * m;
    int64_t jv = (int64_t)bcol * blockDim.x + threadIdx.x;
    if (i >= W && i + W < R.nloc && g >= MG && g <= N - 1 - MG) {
      const T* __restrict__ xrow = R.x + i * m;
      if constexpr (U > 1)
        fd_interior_trips<T, OP, V, U>(xrow, yrow, m, mv, cstride, c, jv);
      fd_interior_trips<T, OP, V, 1>(xrow, yrow, m, mv, cstride, c, jv);
    }
    for (; jv < mv; jv += cstride)
      fd_row_masked<T, OP, V>(R, i, jv * V, g, N, c, edge, yrow);
    // scalar tail columns (m not divisible by V)
    if constexpr (V > 1) {
      for (int64_t j = mv * V + (int64_t)bcol * blockDim.x + threadIdx.x;
           j < m; j += cstride)
        fd_row_masked<T, OP, 1>(R, i, j, g, N, c, edge, yrow);
    }
  }
}

// Row-band stencil: each thread produces RT consecutive rows of ONE 16-B
// column vector from RT+2W input rows loaded up front, fully unrolled —
// (RT+2W loads + RT stores) per RT outputs where fd_kernel issues
// (2..4 loads + 1 store) per output, RT+2W independent loads in flight per
// thread, no loop-carried window (fd_roll_kernel) and 1/RT the workgroups.
// The path is chosen per block from uniform values only:
//   interior — all RT+2W rows are local rows of x, every row has every
//     term active and sits outside the rows fd_edge touches: one base
//     pointer + compile-time multiples of m, the unmasked body per row;
//   general — everything else (first/last band of the global array, bands
//     reaching into gf/gb, the partial last band): the masked body, row by
//     row, rows >= rend never stored.
// RT is compile-time and one value is instantiated (choice: DESIGN.md §3).
#ifndef PAM_FD_BAND_RT
#define PAM_FD_BAND_RT 4
#endif

template <typename T, int OP, int V, int RT>
__global__ void __launch_bounds__(BLK) fd_band_kernel(
    Rows<T> R, T* __restrict__ y, int64_t row0, int64_t N, T c, int edge,
    int64_t rbegin, int64_t rend, uint32_t ncb) {
  constexpr int W = FDDef<OP>::W;
  constexpr int MG = fd_margin<OP>();
  // 1-D grid, column blocks fastest: a band sweeps its rows end to end
  const uint32_t band = blockIdx.x / ncb, cb = blockIdx.x - band * ncb;
  const int64_t m = R.m;
  const int64_t jv = (int64_t)cb * BLK + threadIdx.x;
  if (jv >= m / V) return;
  const int64_t j = jv * V;
  const int64_t i0 = rbegin + (int64_t)band * RT;
  const int64_t g0 = row0 + i0;
  const bool interior = i0 - W >= 0 && i0 + RT - 1 + W < R.nloc &&
                        i0 + RT <= rend && g0 >= MG &&
                        g0 + RT - 1 <= N - 1 - MG;
  if (interior) {
    const T* __restrict__ p = R.x + (i0 - W) * m + j;
    T in[RT + 2 * W][V];
#pragma unroll
    for (int k = 0; k < RT + 2 * W; ++k) loadv<T, V>(p + k * m, in[k]);
    T* __restrict__ q = y + i0 * m + j;
    fd_unroll<RT>([&](auto rc) {
      constexpr int r = decltype(rc)::value;
      fd_row_interior<T, OP, V, RT + 2 * W, r>(in, c, q, m);
    });
    return;
  }
  for (int64_t i = i0; i < i0 + RT && i < rend; ++i)
    fd_row_masked<T, OP, V>(R, i, j, row0 + i, N, c, edge, y + i * m);
}

// Rolling-window stencil: each block walks a row range carrying the 2W+1
// input rows of its column vectors in registers, so every x element is
// loaded from HBM exactly once — the row-parallel kernel relies on L2
// absorbing its neighbour-row re-reads, which fades once a row outgrows it.
// CV independent column vectors per thread (separate windows) give CV
// outstanding loads per row step; a single chain is latency-bound (one
// dependent load per row).  Chains are BLOCK-interleaved (chain q of lane t
// at column block*BLK*CV + q*BLK + t) so each chain's wave accesses stay
// coalesced.  CV = 8 is the swept optimum.
// Guards: load indices are clamped to existing rows (halo planes included)
// and columns; term/edge masks ignore the clamped garbage and an invalid
// chain stores nothing.
#define PAM_FD_ROLL_CV 8

// masked accumulate over the window win[k] = row i-W+k.  The window index
// is a compile-time constant per term: with a runtime index the windows go
// to scratch (measured 2.0 TB/s instead of 5.2).
template <typename T, int OP, int V>
__device__ __forceinline__ void roll_terms(
    const T (&win)[2 * FDDef<OP>::W + 1][V], T (&acc)[V], int64_t g,
    int64_t N) {
  fd_unroll<FDDef<OP>::NT>([&](auto tc) {
    constexpr Term tm = FDDef<OP>::TERMS[decltype(tc)::value];
    if (g >= tm.lo && g <= N - 1 - tm.hi) {
#pragma unroll
      for (int k = 0; k < V; ++k)
        acc[k] += (T)tm.coeff * win[tm.off + FDDef<OP>::W][k];
    }
  });
}

template <typename T, int OP, int V>
__global__ void __launch_bounds__(BLK) fd_roll_kernel(
    Rows<T> R, T* __restrict__ y, int64_t row0, int64_t N, T c, int edge,
    int64_t rbegin, int64_t rend) {
  constexpr int W = FDDef<OP>::W, CV = PAM_FD_ROLL_CV;
  constexpr int NROLL = 2 * W + 1;
  const int64_t m = R.m, mv = m / V;
  const int64_t base = (int64_t)blockIdx.x * blockDim.x * CV + threadIdx.x;
  const int64_t nr = rend - rbegin;
  const int64_t c0 = rbegin + (nr * blockIdx.y) / gridDim.y;
  const int64_t c1 = rbegin + (nr * (blockIdx.y + 1)) / gridDim.y;
  if (c1 <= c0 || base >= mv) return;
  const int64_t lo = R.gf ? -(int64_t)R.w : 0;
  const int64_t hi = R.nloc - 1 + (R.gb ? R.w : 0);
  auto clamp_row = [&](int64_t i) {
    return i < lo ? lo : (i > hi ? hi : i);
  };
  // constant-indexed per-chain state (a runtime-compacted chain array
  // made the windows spill to scratch: 5.2 -> 1.9 TB/s)
  int64_t js[CV];
  bool vq[CV];
#pragma unroll
  for (int q = 0; q < CV; ++q) {
    const int64_t jq = base + (int64_t)q * blockDim.x;
    vq[q] = jq < mv;
    js[q] = (vq[q] ? jq : mv - 1) * V;  // clamped: loads stay in range
  }
  T buf[CV][NROLL][V];  // rows i-W .. i+W of each owned column vector
#pragma unroll
  for (int q = 0; q < CV; ++q)
#pragma unroll
    for (int k = 0; k < NROLL; ++k)
      loadv<T, V>(R.row(clamp_row(c0 - W + k)) + js[q], buf[q][k]);
  for (int64_t i = c0; i < c1; ++i) {
    const int64_t g = row0 + i;
    // issue ALL next-row loads first (CV independent chains)
    T nxt[CV][V];
    const int64_t rn = clamp_row(i + 1 + W);
#pragma unroll
    for (int q = 0; q < CV; ++q) loadv<T, V>(R.row(rn) + js[q], nxt[q]);
#pragma unroll
    for (int q = 0; q < CV; ++q) {
      T acc[V];
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] = (T)0;
      roll_terms<T, OP, V>(buf[q], acc, g, N);
      if (edge) fd_edge<T, OP, V>(R, i, js[q], g, N, acc);
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] *= c;
      if (vq[q]) storev<T, V>(y + i * m + js[q], acc);
#pragma unroll
      for (int k = 0; k < NROLL - 1; ++k)
#pragma unroll
        for (int v = 0; v < V; ++v) buf[q][k][v] = buf[q][k + 1][v];
#pragma unroll
      for (int v = 0; v < V; ++v) buf[q][NROLL - 1][v] = nxt[q][v];
    }
  }
}

// ---- launch plan: which kernel, which lane width, which grid -------------

enum { FD_ROW = 0, FD_ROLL = 1, FD_BAND = 2 };  // pam_fd_variant's codes

struct FdPlan {
  int variant;     // FD_ROW / FD_ROLL / FD_BAND
  int V;           // elements per lane the launch really uses
  bool u4;         // FD_ROW: the 4x-unrolled interior trips
  int64_t gx, gy;  // grid; FD_BAND: column blocks x bands, launched 1-D
};

// The launch of nrows = rend - rbegin rows of m elements of tsize bytes.
// Pure host: fd_launch dispatches on it and pam_fd_variant reports it.
//   PAM_FD_BAND  (read on EVERY call, tests flip it in-process) unset =
//                auto, 1 = band wherever eligible, -1 = never
//   PAM_FD_ROLL  unset = auto, -1 = never rolling, > 0 = rolling wherever
//                eligible;  PAM_FD_LONGROW  the long-row threshold, bytes
//   PAM_FD_GY / PAM_FD_CAP  row-parallel grid caps;  PAM_FD_ROLL_TGT
//                rolling target block count
// Every kernel but the V = 1 row-parallel one needs 16-B lanes: 16-B
// aligned pointers and m a multiple of 16 / tsize.
static FdPlan fd_plan(int tsize, int64_t m, int64_t nrows, bool align16) {
  static const int64_t rollov = env_int("PAM_FD_ROLL", 0);
  static const int64_t longrow = env_int("PAM_FD_LONGROW", 4 << 20);
  static const int64_t gycap = env_int("PAM_FD_GY", 65535);
  static const int64_t totcap = env_int("PAM_FD_CAP", 262144);
  static const int64_t rolltgt = env_int("PAM_FD_ROLL_TGT", 2048);
  const int64_t bandov = env_int("PAM_FD_BAND", 0);
  const int vw = 16 / tsize;
  const bool lanes16 = align16 && m % vw == 0;
  const int64_t rowbytes = m * (int64_t)tsize;
  // Auto rules (12-shape crossover sweep).  Rolling wins
  // above longrow (strict: the 4 MiB power-of-two shape prefers
  // row-parallel) and on "ragged" shapes — rows of at least 5/8 longrow
  // (2.5 MiB) with a row count that is no multiple of 1024, which the
  // row-parallel grid maps unevenly across the 8 XCDs.  The band kernel
  // takes the ragged shapes up to longrow from 4 bands of rows on; fewer
  // (the overlap path's 1-2-row boundary launches) stay rolling.
  const bool ragged = rowbytes * 8 >= longrow * 5 && (nrows % 1024) != 0;
  const bool band_auto = bandov == 0 && rollov == 0 && ragged &&
                         rowbytes <= longrow && nrows >= 4 * PAM_FD_BAND_RT;
  const bool roll_auto = rollov == 0 && (rowbytes > longrow || ragged);
  FdPlan P{FD_ROW, lanes16 ? vw : 1, false, 1, 1};
  if (lanes16 && ((bandov > 0 && nrows >= 1) || band_auto)) {
    P.variant = FD_BAND;
    P.gx = (m / vw + BLK - 1) / BLK;
    P.gy = (nrows + PAM_FD_BAND_RT - 1) / PAM_FD_BAND_RT;
  } else if (lanes16 && (rollov > 0 || roll_auto)) {
    P.variant = FD_ROLL;
    // 32-B lanes where they divide the row: the rolling form's swept
    // optimum (the row-parallel kernel's stays 16 B)
    if (m % 4 == 0) P.V = 4;
    P.gx = (m / P.V + BLK * PAM_FD_ROLL_CV - 1) / (BLK * PAM_FD_ROLL_CV);
    // at least 16 rows per chunk, to amortize the 2W+1-row preload
    const int64_t maxgy = (nrows + 15) / 16;
    P.gy = rolltgt / P.gx;
    if (P.gy > maxgy) P.gy = maxgy;
    if (P.gy < 1) P.gy = 1;
    if (P.gy > 65535) P.gy = 65535;
  } else {
    // one block-row per row; column blocks capped so that a block runs ~4
    // column iterations at large launches.  262144 blocks in all is the
    // measured peak between too few blocks and no loop at all (bench shape,
    // pairs/s by cap: 16384 295.8, 131072 316.6, 262144 332.0, 524288
    // 319.6, 1048576 = no loop 216.6)
    const int64_t nb = (m / P.V + BLK - 1) / BLK;
    P.gy = nrows < gycap ? nrows : gycap;
    if (P.gy < 1) P.gy = 1;
    int64_t cap = totcap / P.gy;
    if (cap < 1) cap = 1;
    P.gx = nb < cap ? nb : cap;
    // the unrolled trips need >= 4 iterations per block: with a single
    // iteration the unrolled kernel is slower than the plain one
    P.u4 = lanes16 && nb >= 4 * P.gx;
  }
  return P;
}

extern "C" int pam_fd_variant(int dtype, int64_t m, int64_t nrows,
                              int aligned16) {
  if (dtype != PAM_F64 && dtype != PAM_F32) return PAM_EDTYPE;
  if (m <= 0 || nrows < 0) return PAM_EARG;
  return fd_plan(dtype == PAM_F64 ? 8 : 4, m, nrows, aligned16 != 0).variant;
}

extern "C" int64_t pam_fd_band_rows(void) { return PAM_FD_BAND_RT; }

// ---- launchers -------------------------------------------------------------

template <typename T>
struct FdCall {  // the arguments every stencil kernel takes
  hipStream_t s;
  Rows<T> R;
  T* y;
  int64_t row0, nglob;
  T c;
  int edge;
  int64_t rbegin, rend;
};

template <typename K, typename T, typename... Extra>
static int fd_go(K kernel, dim3 grid, const FdCall<T>& a, Extra... extra) {
  hipLaunchKernelGGL(kernel, grid, dim3(BLK), 0, a.s, a.R, a.y, a.row0,
                     a.nglob, a.c, a.edge, a.rbegin, a.rend, extra...);
  return check(hipGetLastError());
}

template <typename T, int OP>
static int fd_launch_row(const FdPlan& P, const FdCall<T>& a) {
  constexpr int VW = VecW<T>::value;
  const dim3 grid((uint32_t)P.gx, (uint32_t)P.gy);
  if (P.V == 1) return fd_go(fd_kernel<T, OP, 1, 1>, grid, a);
  if (P.u4) return fd_go(fd_kernel<T, OP, VW, 4>, grid, a);
  return fd_go(fd_kernel<T, OP, VW, 1>, grid, a);
}

template <typename T, int OP>
static int fd_launch_roll(const FdPlan& P, const FdCall<T>& a) {
  const dim3 grid((uint32_t)P.gx, (uint32_t)P.gy);
  if constexpr (VecW<T>::value == 2)
    if (P.V == 2) return fd_go(fd_roll_kernel<T, OP, 2>, grid, a);
  return fd_go(fd_roll_kernel<T, OP, 4>, grid, a);
}

template <typename T, int OP>
static int fd_launch_band(const FdPlan& P, const FdCall<T>& a) {
  if (P.gx * P.gy > 0x7fffffffLL) return PAM_EARG;
  return fd_go(fd_band_kernel<T, OP, VecW<T>::value, PAM_FD_BAND_RT>,
               dim3((uint32_t)(P.gx * P.gy)), a, (uint32_t)P.gx);
}

template <typename T, int OP>
static int fd_launch(void* stream, int edge, const void* x, const void* gf,
                     const void* gb, void* y, int64_t nloc, int64_t m,
                     int64_t row0, int64_t nglob, int64_t rbegin,
                     int64_t rend, double coeff) {
  if (nloc < 0 || m <= 0 || rbegin < 0 || rend > nloc) return PAM_EARG;
  if (nglob < fd_min_rows(OP, edge)) return PAM_EARG;
  const int64_t nrows = rend - rbegin;
  if (nloc == 0 || nrows <= 0) return 0;
  const bool align16 = ((uintptr_t)x % 16 == 0) && ((uintptr_t)y % 16 == 0) &&
                       (gf == nullptr || (uintptr_t)gf % 16 == 0) &&
                       (gb == nullptr || (uintptr_t)gb % 16 == 0);
  const FdPlan P = fd_plan((int)sizeof(T), m, nrows, align16);
  const FdCall<T> a{(hipStream_t)stream,
                    {(const T*)x, (const T*)gf, (const T*)gb, nloc, m,
                     FDDef<OP>::W},
                    (T*)y, row0, nglob, (T)coeff, edge, rbegin, rend};
  switch (P.variant) {
    case FD_BAND: return fd_launch_band<T, OP>(P, a);
    case FD_ROLL: return fd_launch_roll<T, OP>(P, a);
    default: return fd_launch_row<T, OP>(P, a);
  }
}

extern "C" int pam_fd_apply(void* stream, int op, int edge, const void* x,
                            const void* gf, const void* gb, void* y,
                            int64_t nloc, int64_t m, int64_t row0,
                            int64_t nglob, int64_t rbegin, int64_t rend,
                            double coeff, int dtype) {
  if (dtype != PAM_F64 && dtype != PAM_F32) return PAM_EDTYPE;
  return fd_dispatch_op(op, [&](auto opc) {
    constexpr int OP = decltype(opc)::value;
    return dtype == PAM_F64
               ? fd_launch<double, OP>(stream, edge, x, gf, gb, y, nloc, m,
                                       row0, nglob, rbegin, rend, coeff)
               : fd_launch<float, OP>(stream, edge, x, gf, gb, y, nloc, m,
                                      row0, nglob, rbegin, rend, coeff);
  });
}

// pam — kinematic Kirchhoff demigration (spread) and migration (gather):
// the traveltime stage of pylops' Kirchhoff with dynamic = False,
// wavfilter = False, the per-rank operator of the reference's
// least-squares-migration tutorial.  The wavelet stage is pam_conv1d.
//
// Tables in SAMPLES, trace-major: qs [ns, ni], qr [nr, ni].  Per pair of
// trace k = is * nr + ir and image point i, all in T:
//   q = qs[is, i] + qr[ir, i],  f = floor(q),  w = q - f,  it = (int) f
// the pair contributes iff 0 <= it < nt - 1; a NaN, infinite or negative q
// fails `q >= 0 && q < nt` and is dropped before it is converted.
//   forward  d[k, it] += m[i] * (1 - w);  d[k, it + 1] += m[i] * w
//   adjoint  mig[i] = sum_k ((1 - w) * d[k, it]) + (w * d[k, it + 1])
//
// Adjoint (gather) — pinned arithmetic, a NumPy loop reproduces every bit:
// a thread owns KIRCH_R image points (lanes run over i: the table loads
// coalesce), acc = 0, traces ascending, term = ((1 - w) * d0) + (w * d1)
// with each operation rounded once, acc += term.  A workgroup takes
// KIRCH_P = 256 * KIRCH_R points.  When the point tiles alone cannot fill
// the chip the traces are cut into chunks of KIRCH_CHUNK traces; every
// (tile, chunk) writes its partial to the workspace and a second kernel
// adds the partials in ascending chunk order.  Two bodies: 0 gathers d0, d1
// straight from global memory (neighbouring points hit neighbouring
// samples, so a wave's gather touches a few lines that L2 / the vector L1
// already hold), 1 stages the whole trace in LDS first (2 barriers per
// trace).  Measured on MI355X (profiles/kirchhoff.log): see
// KIRCH_STAGE_AUTO below.  Splitting matters far more than the body: the
// 32 point tiles of the 32768-point shape took 5.1 ms unsplit and 0.19 ms
// in 128 chunks.
//
// Forward (spread) — a scatter.  A workgroup owns the window [t0, t0 + W)
// of one trace in LDS (as float64, whatever T), zeroes it, loops over ALL
// image points (256 per step), adds the contributions that land in the
// window with LDS float adds (it and it + 1 are tested separately, so a
// pair may straddle the window edge) and writes the window with plain
// stores: no global atomics, no two workgroups on one destination, no
// pre-zeroed output.  W is the whole trace when traces alone fill the
// chip; fewer traces get shorter windows (more workgroups, each dropping
// the pairs outside its window), and a trace beyond the LDS budget gets
// windows of the budget's size.  Every window scans all image points, so
// windows multiply the table reads: with 4096 traces a forced W = 512 took
// 1.8x and W = 128 7x the time of W = nt = 1024 (float64); with 110 traces
// W = 128 ... 651 ran within 10 % of each other (9 us, launch-bound).
// The ORDER in which the LDS adds of one sample happen depends on the
// schedule, so the forward is not pinned bit for bit: a sample is the sum of
// its n rounded products in some order.

#include "launch.h"

#pragma clang fp contract(off)

#define KIRCH_R 4                    // image points per thread, adjoint
#define KIRCH_P (BLK * KIRCH_R)     // image points per workgroup, adjoint
#define KIRCH_CHUNK 32               // traces per partial when traces split
#define KIRCH_LDS_BYTES 65536        // LDS budget of one workgroup
#define KIRCH_FILL 512               // workgroups that fill the chip (2 / CU)
#define KIRCH_W_MIN 128              // shortest automatic window
#define KIRCH_WS_MAX ((int64_t)1 << 25)  // partials the split may ask for
// automatic choice of the adjoint body, measured on MI355X
// (profiles/kirchhoff.log): the staged body ran BEHIND the plain gather at
// both shapes measured and in both dtypes — 0.224 against 0.190 ms
// (float32) and 0.241 against 0.228 ms (float64) at 4096 traces x 32768
// points x 1024 samples with the traces split, 0.046 / 0.049 against
// 0.040 / 0.042 ms at the tutorial's 110 x 4860 x 651, and by 17-50 %
// unsplit — so the plan never takes it by itself; PAM_KIRCH_STAGE=1
// selects it for measuring other shapes.
#define KIRCH_STAGE_AUTO 0

// ---------------------------------------------------------------- adjoint
template <typename T, bool STAGE>
__global__ void __launch_bounds__(BLK) kirch_gather_kernel(
    const T* __restrict__ d, T* __restrict__ out, const T* __restrict__ qs,
    const T* __restrict__ qr, int64_t nr, int64_t ntr, int64_t ni,
    int64_t nt, int64_t chunk, int64_t ntile, int64_t nitems) {
  extern __shared__ __align__(16) unsigned char kirch_smem[];
  T* lds = reinterpret_cast<T*>(kirch_smem);
  const int tid = threadIdx.x;
  const T tmax = (T)nt;
  for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int64_t c = item / ntile;
    const int64_t i0 = (item - c * ntile) * KIRCH_P + tid;
    const int64_t k0 = c * chunk;
    const int64_t k1 = k0 + chunk < ntr ? k0 + chunk : ntr;
    T acc[KIRCH_R];
#pragma unroll
    for (int r = 0; r < KIRCH_R; ++r) acc[r] = (T)0;
    int64_t is = k0 / nr, ir = k0 - is * nr;
    for (int64_t k = k0; k < k1; ++k) {
      const T* dk = d + k * nt;
      if constexpr (STAGE) {
        __syncthreads();      // the previous trace has been read
        for (int64_t j = tid; j < nt; j += BLK) lds[j] = dk[j];
        __syncthreads();
      }
      const T* qsk = qs + is * ni;
      const T* qrk = qr + ir * ni;
#pragma unroll
      for (int r = 0; r < KIRCH_R; ++r) {
        const int64_t i = i0 + (int64_t)r * BLK;
        if (i < ni) {
          const T q = qsk[i] + qrk[i];
          if (q >= (T)0 && q < tmax) {
            const T f = floor(q);
            const int64_t it = (int64_t)f;
            if (it < nt - 1) {
              const T w = q - f;
              T d0, d1;
              if constexpr (STAGE) {
                d0 = lds[it];
                d1 = lds[it + 1];
              } else {
                d0 = dk[it];
                d1 = dk[it + 1];
              }
              const T term = (((T)1 - w) * d0) + (w * d1);
              acc[r] += term;
            }
          }
        }
      }
      if (++ir == nr) {
        ir = 0;
        ++is;
      }
    }
    T* o = out + c * ni;    // the image itself when there is one chunk
#pragma unroll
    for (int r = 0; r < KIRCH_R; ++r) {
      const int64_t i = i0 + (int64_t)r * BLK;
      if (i < ni) o[i] = acc[r];
    }
  }
}

// mig[i] = ws[0, i] + ws[1, i] + ... in ascending chunk order
template <typename T>
__global__ void __launch_bounds__(BLK) kirch_combine_kernel(
    const T* __restrict__ ws, T* __restrict__ mig, int64_t ni,
    int64_t nchunk) {
  const int64_t stride = (int64_t)gridDim.x * BLK;
  for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < ni;
       i += stride) {
    T acc = ws[i];
    for (int64_t c = 1; c < nchunk; ++c) acc += ws[c * ni + i];
    mig[i] = acc;
  }
}

// ---------------------------------------------------------------- forward
// The window is kept in float64 for float32 traces too: on MI355X colliding
// ds_add_f32 ran 6x slower than ds_add_f64 (1.37 against 0.22 ms on the
// 134 Mpair shape of profiles/kirchhoff.log).  The products are rounded in
// T; the sum is rounded to T once, when the window is written.
template <typename T>
__global__ void __launch_bounds__(BLK) kirch_spread_kernel(
    const T* __restrict__ m, T* __restrict__ d, const T* __restrict__ qs,
    const T* __restrict__ qr, int64_t nr, int64_t ni, int64_t nt, int64_t W,
    int64_t nwin, int64_t nitems) {
  extern __shared__ __align__(16) unsigned char kirch_smem[];
  double* lds = reinterpret_cast<double*>(kirch_smem);
  const int tid = threadIdx.x;
  const T tmax = (T)nt;
  for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int64_t k = item / nwin;
    const int64_t t0 = (item - k * nwin) * W;
    const int64_t wl = t0 + W < nt ? W : nt - t0;   // samples of this window
    const int64_t is = k / nr, ir = k - is * nr;
    const T* qsk = qs + is * ni;
    const T* qrk = qr + ir * ni;
    for (int64_t j = tid; j < wl; j += BLK) lds[j] = 0.0;
    __syncthreads();
    for (int64_t i = tid; i < ni; i += BLK) {
      const T q = qsk[i] + qrk[i];
      if (q >= (T)0 && q < tmax) {
        const T f = floor(q);
        const int64_t it = (int64_t)f;
        if (it < nt - 1) {
          const T w = q - f;
          const T mi = m[i];
          const int64_t j = it - t0;     // in [-t0, nt - 1 - t0)
          if (j >= 0 && j < wl) atomicAdd(lds + j, (double)(mi * ((T)1 - w)));
          if (j + 1 >= 0 && j + 1 < wl)
            atomicAdd(lds + j + 1, (double)(mi * w));
        }
      }
    }
    __syncthreads();
    T* dk = d + k * nt + t0;
    for (int64_t j = tid; j < wl; j += BLK) dk[j] = (T)lds[j];
    __syncthreads();        // the window is reused by the next item
  }
}

// ------------------------------------------------------------ launch plan
// (the PAM_KIRCH_* knobs are read on EVERY call)
static int64_t kirch_tsize(int dtype) { return dtype == PAM_F64 ? 8 : 4; }

// forward window: PAM_KIRCH_WINDOW = W in [1, budget] forces it; else the
// trace is cut until ntr * nwin workgroups fill the chip, windows of at
// least KIRCH_W_MIN and at most the LDS budget; never longer than nt
static int64_t kirch_window_of(int64_t ntr, int64_t nt) {
  const int64_t wmax = KIRCH_LDS_BYTES / (int64_t)sizeof(double);
  int64_t W = env_int("PAM_KIRCH_WINDOW", -1);
  if (W < 1 || W > wmax) {
    const int64_t want = ntr >= KIRCH_FILL ? 1 : (KIRCH_FILL + ntr - 1) / ntr;
    W = (nt + want - 1) / want;
    W = (W + 63) / 64 * 64;
    if (W < KIRCH_W_MIN) W = KIRCH_W_MIN;
    if (W > wmax) W = wmax;
  }
  return W < nt ? W : nt;
}

struct KirchAdjPlan {
  int stage;        // 0 gather from global memory, 1 trace staged in LDS
  int64_t chunk;    // traces per partial: KIRCH_CHUNK, or ntr (no split)
  int64_t nchunk;
  int64_t ntile;
};

// adjoint: split the traces iff the point tiles do not fill the chip, there
// is more than one chunk and the partials stay below KIRCH_WS_MAX elements;
// PAM_KIRCH_SPLIT = 0 | 1 forces the answer (1 still needs > 1 chunk).
// PAM_KIRCH_STAGE = 0 | 1 forces the body; staging needs the trace to fit.
static KirchAdjPlan kirch_adj_plan(int dtype, int64_t ntr, int64_t ni,
                                   int64_t nt) {
  KirchAdjPlan P;
  P.ntile = (ni + KIRCH_P - 1) / KIRCH_P;
  const int64_t nck = (ntr + KIRCH_CHUNK - 1) / KIRCH_CHUNK;
  const int64_t forced = env_int("PAM_KIRCH_SPLIT", -1);
  bool split = P.ntile < KIRCH_FILL && nck <= KIRCH_WS_MAX / ni;
  if (forced == 0 || forced == 1) split = forced == 1;
  split = split && nck > 1;
  P.chunk = split ? KIRCH_CHUNK : ntr;
  P.nchunk = split ? nck : 1;
  const int64_t st = env_int("PAM_KIRCH_STAGE", -1);
  P.stage = (st == 0 || st == 1) ? (int)st : KIRCH_STAGE_AUTO;
  if (nt > KIRCH_LDS_BYTES / kirch_tsize(dtype)) P.stage = 0;
  return P;
}

static bool kirch_sizes_ok(int64_t ns, int64_t nr, int64_t ni, int64_t nt) {
  const int64_t big = (int64_t)1 << 62;
  return ns > 0 && nr > 0 && ni > 0 && nt >= 2 && ns <= big / nr &&
         ns * nr <= big / nt && ns <= big / ni && nr <= big / ni;
}

extern "C" int64_t pam_kirch_points(void) { return KIRCH_P; }

extern "C" int64_t pam_kirch_chunk(int64_t ns, int64_t nr, int64_t ni,
                                   int64_t nt, int dtype) {
  if (!kirch_sizes_ok(ns, nr, ni, nt)) return PAM_EARG;
  if (dtype != PAM_F64 && dtype != PAM_F32) return PAM_EDTYPE;
  return kirch_adj_plan(dtype, ns * nr, ni, nt).chunk;
}

extern "C" int pam_kirch_variant(int64_t ns, int64_t nr, int64_t ni,
                                 int64_t nt, int dtype) {
  if (!kirch_sizes_ok(ns, nr, ni, nt)) return PAM_EARG;
  if (dtype != PAM_F64 && dtype != PAM_F32) return PAM_EDTYPE;
  return kirch_adj_plan(dtype, ns * nr, ni, nt).stage;
}

extern "C" int64_t pam_kirch_window(int64_t ns, int64_t nr, int64_t ni,
                                    int64_t nt, int dtype) {
  if (!kirch_sizes_ok(ns, nr, ni, nt)) return PAM_EARG;
  if (dtype != PAM_F64 && dtype != PAM_F32) return PAM_EDTYPE;
  return kirch_window_of(ns * nr, nt);
}

extern "C" int64_t pam_kirch_ws_elems(int adjoint, int64_t ns, int64_t nr,
                                      int64_t ni, int64_t nt, int dtype) {
  if (!kirch_sizes_ok(ns, nr, ni, nt)) return PAM_EARG;
  if (dtype != PAM_F64 && dtype != PAM_F32) return PAM_EDTYPE;
  if (!adjoint) return 0;
  const KirchAdjPlan P = kirch_adj_plan(dtype, ns * nr, ni, nt);
  return P.nchunk > 1 ? P.nchunk * ni : 0;
}

static unsigned kirch_grid(int64_t nitems) {
  return (unsigned)(nitems < 0x7FFFFFFF ? nitems : 0x7FFFFFFF);
}

template <typename T>
static int kirch_launch(hipStream_t s, int adjoint, void* m, void* d,
                        const void* qs, const void* qr, void* ws, int64_t nr,
                        int64_t ntr, int64_t ni, int64_t nt, int dtype) {
  const T* qsp = (const T*)qs;
  const T* qrp = (const T*)qr;
  if (!adjoint) {
    const int64_t W = kirch_window_of(ntr, nt);
    const int64_t nwin = (nt + W - 1) / W;
    const int64_t nitems = ntr * nwin;
    hipLaunchKernelGGL((kirch_spread_kernel<T>), dim3(kirch_grid(nitems)),
                       dim3(BLK), (size_t)(W * sizeof(double)), s, (const T*)m,
                       (T*)d, qsp, qrp, nr, ni, nt, W, nwin, nitems);
    return (int)hipGetLastError();
  }
  const KirchAdjPlan P = kirch_adj_plan(dtype, ntr, ni, nt);
  const int64_t nitems = P.ntile * P.nchunk;
  T* out = P.nchunk > 1 ? (T*)ws : (T*)m;
  if (P.stage)
    hipLaunchKernelGGL((kirch_gather_kernel<T, true>),
                       dim3(kirch_grid(nitems)), dim3(BLK),
                       (size_t)(nt * sizeof(T)), s, (const T*)d, out, qsp,
                       qrp, nr, ntr, ni, nt, P.chunk, P.ntile, nitems);
  else
    hipLaunchKernelGGL((kirch_gather_kernel<T, false>),
                       dim3(kirch_grid(nitems)), dim3(BLK), 0, s,
                       (const T*)d, out, qsp, qrp, nr, ntr, ni, nt, P.chunk,
                       P.ntile, nitems);
  int rc = (int)hipGetLastError();
  if (rc || P.nchunk == 1) return rc;
  int64_t g = (ni + BLK - 1) / BLK;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL((kirch_combine_kernel<T>), dim3((unsigned)g),
                     dim3(BLK), 0, s, (const T*)ws, (T*)m, ni, P.nchunk);
  return (int)hipGetLastError();
}

extern "C" int pam_kirch(void* stream, int adjoint, void* m, void* d,
                         const void* qs, const void* qr, void* ws,
                         int64_t ns, int64_t nr, int64_t ni, int64_t nt,
                         int dtype) {
  if (!kirch_sizes_ok(ns, nr, ni, nt) || !m || !d || !qs || !qr)
    return PAM_EARG;
  if (dtype != PAM_F64 && dtype != PAM_F32) return PAM_EDTYPE;
  const int64_t ts = kirch_tsize(dtype), ntr = ns * nr;
  const uintptr_t mb = (uintptr_t)m, db = (uintptr_t)d;
  if (mb < db + (uintptr_t)(ntr * nt * ts) && db < mb + (uintptr_t)(ni * ts))
    return PAM_EARG;      // m and d share memory
  if (!ws && pam_kirch_ws_elems(adjoint, ns, nr, ni, nt, dtype) > 0)
    return PAM_EARG;
  hipStream_t s = (hipStream_t)stream;
  return dtype == PAM_F64
             ? kirch_launch<double>(s, adjoint, m, d, qs, qr, ws, nr, ntr, ni,
                                    nt, dtype)
             : kirch_launch<float>(s, adjoint, m, d, qs, qr, ws, nr, ntr, ni,
                                   nt, dtype);
}

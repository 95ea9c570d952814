// pam — stationary 1-D convolution along axis d of a [batch, d, m] block,
// with an optionally fused first derivative (the post-stack model
// C(Dx) / D^T(C^T x) in one pass).  The local operator of pylops'
// Convolve1D / PoststackLinearModelling inside MPIBlockDiag.
//
//   forward  y[b,n,j] = sum_k h[k] * v[b, n-k+offset, j]
//   adjoint  y[b,n,j] = sum_k h[k] * x[b, n+k-offset, j]
// terms whose sample index leaves [0, d) are skipped (zero padding).
//
// Pinned arithmetic: acc = 0, k ascending, one rounded multiply and one
// rounded add per tap in T, stored unscaled — a NumPy loop in the same
// dtype reproduces every bit.  The derivative stages use FDDef<OP>::TERMS
// of fd_defs.h in their order with edge = 0, coeff = 1, so the fused result
// is what pam_fd_serial and pam_conv1d(deriv = 0) give one after the other.
//
// Three kernels:
//   0 plain   one thread per output, taps and samples from global memory
//   1 trace   (m small) a workgroup owns a run of consecutive flattened
//             (n, j) outputs of one batch; the run plus its (nh-1)*m halo is
//             staged in LDS once; lane l reads LDS word base + l: no bank
//             conflict.  A tap shifts the flat index by m, and "row inside
//             [0, d)" is "flat index inside [0, d*m)", so no row / column
//             is ever formed.
//   2 column  (m large) a workgroup owns tile_d rows of tile_m columns;
//             tile_d + nh - 1 rows are staged, lanes run across columns and
//             a thread produces CONV_R consecutive rows from a rotating
//             register window: one LDS read per tap feeds CONV_R
//             multiply-adds.
// The tiled kernels pad with zeros instead of skipping: h[k] * 0 = +-0
// leaves acc unchanged (at most the sign of a zero result differs) for
// finite taps.  The taps are wave-uniform and come in as scalar loads.

#include "fd_defs.h"

#pragma clang fp contract(off)

#define CONV_R 8          // rows per thread, column kernel
#define CONV_TM 64        // columns per workgroup, column kernel
#define CONV_TD_MAX 128   // rows per workgroup, column kernel (at most)
#define CONV_CHUNK 2048   // flattened outputs per workgroup, trace kernel
#define CONV_LDS_BYTES 65536   // LDS budget of one workgroup
#define CONV_IDX_MAX (1 << 30) // d*m bound of the 32-bit tiled kernels
// automatic dispatch, measured on MI355X (profiles/conv1d_variants.log): a
// tiled kernel is chosen only where it ran ahead of the plain one there.
// trace: its cost depends on nh and on halo / run only; ahead from nh = 3
// at a negligible halo and, at nh = 41, up to a halo of 2.6 runs.
// column: ahead from 24 columns at nh = 41 and, at 1024 columns, from
// nh = 9 (float32) / nh = 21 (float64; 9 is a 17 % lead, 3 a loss).
#define CONV_TRACE_NH_MIN 3
#define CONV_COL_M_MIN 24
#define CONV_COL_NH_MIN_F32 9
#define CONV_COL_NH_MIN_F64 21

// the serial stencil a derivative stage fuses: centered 4/5, forward 0/1
template <bool ADJ, int DERIV> struct ConvFD {
  static constexpr int OP = (DERIV == 1 ? 4 : 0) + (ADJ ? 1 : 0);
};

// v = (D x) at flat position f of one batch (row f / m), pam_fd_serial's
// arithmetic; I is the index type.  g >= lo <=> f >= lo*m and
// g <= d-1-hi <=> f < (d-hi)*m, so the row is never formed.
template <typename T, int OP, typename I>
__device__ __forceinline__ T conv_fd_at(const T* __restrict__ xb, I f, I d,
                                        I m) {
  T acc = (T)0;
#pragma unroll
  for (int t = 0; t < FDDef<OP>::NT; ++t) {
    const Term tm = FDDef<OP>::TERMS[t];
    if (f >= (I)tm.lo * m && f < (d - (I)tm.hi) * m)
      acc += (T)tm.coeff * xb[f + (I)tm.off * m];
  }
  return acc;
}

// ------------------------------------------------------------------ plain
// w(n) = sum_k h[k] * s[n -+ k +- offset], s = x or (forward, DERIV) D x
template <typename T, bool ADJ, int DERIV>
__device__ __forceinline__ T conv_plain_at(const T* __restrict__ xb,
                                           const T* __restrict__ h,
                                           int64_t n, int64_t j, int64_t d,
                                           int64_t m, int64_t nh,
                                           int64_t off) {
  T acc = (T)0;
  for (int64_t k = 0; k < nh; ++k) {
    const int64_t g = ADJ ? n + k - off : n - k + off;
    if (g < 0 || g >= d) continue;
    T s;
    if constexpr (!ADJ && DERIV != 0)
      s = conv_fd_at<T, ConvFD<false, DERIV>::OP, int64_t>(xb, g * m + j, d,
                                                          m);
    else
      s = xb[g * m + j];
    acc += h[k] * s;
  }
  return acc;
}

template <typename T, bool ADJ, int DERIV>
__global__ void __launch_bounds__(BLK) conv_plain_kernel(
    const T* __restrict__ x, T* __restrict__ y, const T* __restrict__ h,
    int64_t batch, int64_t d, int64_t m, int64_t nh, int64_t off) {
  const int64_t total = batch * d * m;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total; idx += stride) {
    const int64_t j = idx % m;
    const int64_t rem = idx / m;
    const int64_t n = rem % d;
    const T* xb = x + (rem - n) * m;
    if constexpr (ADJ && DERIV != 0) {
      constexpr int OP = ConvFD<true, DERIV>::OP;
      T acc = (T)0;
#pragma unroll
      for (int t = 0; t < FDDef<OP>::NT; ++t) {
        const Term tm = FDDef<OP>::TERMS[t];
        if (n >= tm.lo && n <= d - 1 - tm.hi)
          acc += (T)tm.coeff * conv_plain_at<T, true, 0>(xb, h, n + tm.off, j,
                                                         d, m, nh, off);
      }
      y[idx] = acc;
    } else {
      y[idx] = conv_plain_at<T, ADJ, DERIV>(xb, h, n, j, d, m, nh, off);
    }
  }
}

// ------------------------------------------------------------------ tiled
// TM > 0: column kernel (LDS pitch TM, R rows per thread); TM == 0: trace
// kernel (flat run, LDS "pitch" m, R == 1).  td = rows (column) or flat
// outputs (trace) per workgroup.  LDS word 0 is sample row
// first_output_row - E - HL, HL the taps' reach below an output.
template <typename T, int R, int TM, bool ADJ, int DERIV>
__global__ void __launch_bounds__(BLK) conv_tiled_kernel(
    const T* __restrict__ x, T* __restrict__ y, const T* __restrict__ h,
    int d, int m, int nh, int off, int td, int ntile_d, int ntile_m) {
  extern __shared__ __align__(16) unsigned char conv_smem[];
  T* lds = reinterpret_cast<T*>(conv_smem);
  static_assert(TM > 0 || R == 1, "the trace kernel has one row per thread");
  constexpr bool COL = TM > 0;
  constexpr int E = (ADJ && DERIV != 0) ? 1 : 0;  // extra w rows per side
  constexpr int NW = R + 2 * E;                   // window / accumulators
  const int tid = threadIdx.x;
  const int HL = ADJ ? off : nh - 1 - off;
  const int dm = d * m;

  int64_t bi = blockIdx.x;
  const int tmi = (int)(bi % ntile_m);
  bi /= ntile_m;
  const int tdi = (int)(bi % ntile_d);
  const int64_t b = bi / ntile_d;
  const T* xb = x + b * (int64_t)dm;
  T* yb = y + b * (int64_t)dm;

  const int S = COL ? TM : m;      // LDS distance of one row
  const int o0 = tdi * td;         // first output row (column) / flat (trace)
  const int c0 = tmi * TM;
  // outputs this workgroup really owns (the last tile may be short)
  const int nout = min(td, (COL ? d : dm) - o0);

  // ---- stage: samples (or D x) with zeros outside the block ----
  if constexpr (COL) {
    // whole row groups: the window of a short last group reads them
    const int nrows = (nout + R - 1) / R * R + 2 * E + nh - 1;
    const int g0 = o0 - E - HL;
    for (int i = tid; i < nrows * TM; i += BLK) {
      const int lr = i / TM, lc = i % TM;
      const int g = g0 + lr, c = c0 + lc;
      T v = (T)0;
      if (g >= 0 && g < d && c < m) {
        const int f = g * m + c;
        if constexpr (!ADJ && DERIV != 0)
          v = conv_fd_at<T, ConvFD<false, DERIV>::OP, int>(xb, f, d, m);
        else
          v = xb[f];
      }
      lds[i] = v;
    }
  } else {
    const int nst = nout + (2 * E + nh - 1) * m;
    const int f0 = o0 - (E + HL) * m;
    for (int i = tid; i < nst; i += BLK) {
      const int f = f0 + i;
      T v = (T)0;
      if (f >= 0 && f < dm) {
        if constexpr (!ADJ && DERIV != 0)
          v = conv_fd_at<T, ConvFD<false, DERIV>::OP, int>(xb, f, d, m);
        else
          v = xb[f];
      }
      lds[i] = v;
    }
  }
  __syncthreads();

  // ---- items: (row group, column) or one flat output ----
  const int nitems = COL ? ((nout + R - 1) / R) * TM : nout;
  for (int it = tid; it < nitems; it += BLK) {
    int ib, fo;        // LDS word of window row 0 at tap row 0; output flat
    int rows = R;      // output rows of this item inside the block
    if constexpr (COL) {
      const int lc = it % TM, grp = it / TM;
      const int c = c0 + lc;
      if (c >= m) continue;
      ib = grp * R * TM + lc;
      fo = (o0 + grp * R) * m + c;
      rows = min(R, nout - grp * R);
    } else {
      ib = it;
      fo = o0 + it;
    }

    // rotating window: logical row q of the window sits in win[(q +- u)
    // % NW] at step u of an unrolled group of NW taps; each tap loads the
    // one row that enters (top for the adjoint, bottom for the forward).
    T win[NW], acc[NW];
#pragma unroll
    for (int q = 0; q < NW; ++q) acc[q] = (T)0;
    if constexpr (ADJ) {
#pragma unroll
      for (int q = 0; q < NW - 1; ++q) win[q] = lds[ib + q * S];
    } else {
#pragma unroll
      for (int q = 1; q < NW; ++q) win[q] = lds[ib + (q + nh - 1) * S];
    }
    for (int k0 = 0; k0 < nh; k0 += NW) {
      fd_unroll<NW>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const int k = k0 + u;
        if (k < nh) {
          const T hk = h[k];
          if constexpr (ADJ)
            win[(NW - 1 + u) % NW] = lds[ib + (NW - 1 + k) * S];
          else
            win[(NW - u) % NW] = lds[ib + (nh - 1 - k) * S];
          fd_unroll<NW>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            constexpr int p = ADJ ? (q + u) % NW : (q - u + NW) % NW;
            acc[q] += hk * win[p];
          });
        }
      });
    }

    // ---- out: w itself, or D^T w from the neighbours in registers ----
    fd_unroll<R>([&](auto rc) {
      constexpr int r = decltype(rc)::value;
      if (r < rows) {
        const int f = fo + r * m;
        if constexpr (E == 0) {
          yb[f] = acc[r];
        } else {
          constexpr int OP = ConvFD<true, DERIV>::OP;
          T a = (T)0;
          fd_unroll<FDDef<OP>::NT>([&](auto tc) {
            constexpr Term tm = FDDef<OP>::TERMS[decltype(tc)::value];
            if (f >= tm.lo * m && f < (d - tm.hi) * m)
              a += (T)tm.coeff * acc[r + E + tm.off];
          });
          yb[f] = a;
        }
      }
    });
  }
}

// ------------------------------------------------------------ launch plan
struct ConvPlan {
  int variant;          // 0 plain, 1 trace, 2 column
  int64_t td;           // rows (column) / flat outputs (trace) per workgroup
  int64_t ntd, ntm;     // tiles along d (or the flat run) and along m
  size_t lds;           // dynamic LDS bytes
};

// rows per workgroup of the column kernel for nh taps: what the LDS budget
// leaves after the nh - 1 halo rows and the derivative's 2, a multiple of
// CONV_R, at most CONV_TD_MAX; 0 = does not fit
static int64_t conv_col_td(int64_t tsize, int64_t nh) {
  const int64_t rows = CONV_LDS_BYTES / (CONV_TM * tsize) - (nh + 1);
  if (rows < CONV_R) return 0;
  const int64_t td = rows / CONV_R * CONV_R;
  return td > CONV_TD_MAX ? CONV_TD_MAX : td;
}

static bool conv_trace_fits(int64_t tsize, int64_t m, int64_t nh) {
  // (nh + 1) * m halo words next to the run; nh, m < 2^31 each
  if (nh > CONV_LDS_BYTES || m > CONV_LDS_BYTES) return false;
  return (CONV_CHUNK + (nh + 1) * m) * tsize <= CONV_LDS_BYTES;
}

// Pure host: pam_conv1d launches what this says, pam_conv1d_variant
// reports it.  Automatic choice: trace while the halo is small next to the
// run (m <= 2 nh and (nh + 1) m <= 2 runs), else column from
// CONV_COL_M_MIN columns and CONV_COL_NH_MIN_* taps, else plain.
static ConvPlan conv_plan(int dtype, int64_t batch, int64_t d, int64_t m,
                          int64_t nh) {
  const int64_t tsize = dtype == PAM_F64 ? 8 : 4;
  ConvPlan P = {0, 0, 0, 0, 0};
  const bool idx32 = d <= CONV_IDX_MAX / m;  // d * m <= 2^30
  const int64_t td2 = conv_col_td(tsize, nh);
  const bool ok1 = idx32 && conv_trace_fits(tsize, m, nh);
  const bool ok2 = idx32 && td2 > 0;
  const int64_t forced = env_int("PAM_CONV_VARIANT", -1);  // on EVERY call
  int want;
  if (forced >= 0 && forced <= 2) {
    want = (int)forced;
  } else if (ok1 && nh >= CONV_TRACE_NH_MIN && m <= 2 * nh &&
             (nh + 1) * m <= 2 * CONV_CHUNK) {
    want = 1;
  } else if (ok2 && m >= CONV_COL_M_MIN &&
             nh >= (dtype == PAM_F64 ? CONV_COL_NH_MIN_F64
                                     : CONV_COL_NH_MIN_F32)) {
    want = 2;
  } else {
    want = 0;
  }
  if (want == 1 && ok1) {
    P.variant = 1;
    P.td = CONV_CHUNK;
    P.ntd = (d * m + P.td - 1) / P.td;
    P.ntm = 1;
    const int64_t run = d * m < P.td ? d * m : P.td;
    P.lds = (size_t)((run + (nh + 1) * m) * tsize);
  } else if (want == 2 && ok2) {
    P.variant = 2;
    P.td = td2;
    P.ntd = (d + td2 - 1) / td2;
    P.ntm = (m + CONV_TM - 1) / CONV_TM;
    const int64_t rows = d < td2 ? (d + CONV_R - 1) / CONV_R * CONV_R : td2;
    P.lds = (size_t)((rows + nh + 1) * CONV_TM * tsize);
  }
  // the tiled kernels decode a 1-D grid
  if (P.variant && batch > 0 &&
      P.ntd * P.ntm > (int64_t)0x7FFFFFFF / batch) {
    P = {0, 0, 0, 0, 0};
  }
  return P;
}

extern "C" int pam_conv1d_variant(int dtype, int64_t d, int64_t m,
                                  int64_t nh) {
  if (dtype != PAM_F64 && dtype != PAM_F32) return PAM_EDTYPE;
  if (d <= 0 || m <= 0 || nh <= 0) return PAM_EARG;
  return conv_plan(dtype, 1, d, m, nh).variant;
}

extern "C" int64_t pam_conv1d_tile_d(int variant, int dtype, int64_t nh) {
  if (dtype != PAM_F64 && dtype != PAM_F32) return PAM_EDTYPE;
  if (nh <= 0) return PAM_EARG;
  if (variant == 1) return CONV_CHUNK;
  if (variant == 2) return conv_col_td(dtype == PAM_F64 ? 8 : 4, nh);
  return 0;
}

extern "C" int64_t pam_conv1d_tile_m(int variant, int dtype) {
  if (dtype != PAM_F64 && dtype != PAM_F32) return PAM_EDTYPE;
  if (variant == 1) return 1;
  if (variant == 2) return CONV_TM;
  return 0;
}

template <typename T, bool ADJ, int DERIV>
static int conv_launch(hipStream_t s, const ConvPlan& P, const void* x,
                       void* y, const void* h, int64_t batch, int64_t d,
                       int64_t m, int64_t nh, int64_t off) {
  const T* xp = (const T*)x;
  const T* hp = (const T*)h;
  T* yp = (T*)y;
  if (P.variant == 0) {
    int64_t g = (batch * d * m + BLK - 1) / BLK;
    if (g > 0x7FFFFFFF) g = 0x7FFFFFFF;
    hipLaunchKernelGGL((conv_plain_kernel<T, ADJ, DERIV>), dim3((unsigned)g),
                       dim3(BLK), 0, s, xp, yp, hp, batch, d, m, nh, off);
  } else {
    const dim3 grid((unsigned)(batch * P.ntd * P.ntm));
    if (P.variant == 1)
      hipLaunchKernelGGL((conv_tiled_kernel<T, 1, 0, ADJ, DERIV>), grid,
                         dim3(BLK), P.lds, s, xp, yp, hp, (int)d, (int)m,
                         (int)nh, (int)off, (int)P.td, (int)P.ntd,
                         (int)P.ntm);
    else
      hipLaunchKernelGGL((conv_tiled_kernel<T, CONV_R, CONV_TM, ADJ, DERIV>),
                         grid, dim3(BLK), P.lds, s, xp, yp, hp, (int)d,
                         (int)m, (int)nh, (int)off, (int)P.td, (int)P.ntd,
                         (int)P.ntm);
  }
  return (int)hipGetLastError();
}

template <typename T>
static int conv_dispatch(hipStream_t s, const ConvPlan& P, int adjoint,
                         int deriv, const void* x, void* y, const void* h,
                         int64_t batch, int64_t d, int64_t m, int64_t nh,
                         int64_t off) {
#define CONV_CASE(A, D)                                                 \
  if ((adjoint != 0) == A && deriv == D)                                \
    return conv_launch<T, A, D>(s, P, x, y, h, batch, d, m, nh, off)
  CONV_CASE(false, 0);
  CONV_CASE(false, 1);
  CONV_CASE(false, 2);
  CONV_CASE(true, 0);
  CONV_CASE(true, 1);
  CONV_CASE(true, 2);
#undef CONV_CASE
  return PAM_EOP;
}

extern "C" int pam_conv1d(void* stream, int adjoint, const void* x, void* y,
                          const void* h, int64_t batch, int64_t d, int64_t m,
                          int64_t nh, int64_t offset, int deriv, int dtype) {
  if (batch <= 0 || d <= 0 || m <= 0 || nh <= 0 || offset < 0 ||
      offset >= nh || !x || !y || !h)
    return PAM_EARG;
  if (deriv < 0 || deriv > 2) return PAM_EOP;
  if (dtype != PAM_F64 && dtype != PAM_F32) return PAM_EDTYPE;
  const ConvPlan P = conv_plan(dtype, batch, d, m, nh);
  hipStream_t s = (hipStream_t)stream;
  return dtype == PAM_F64
             ? conv_dispatch<double>(s, P, adjoint, deriv, x, y, h, batch, d,
                                     m, nh, offset)
             : conv_dispatch<float>(s, P, adjoint, deriv, x, y, h, batch, d,
                                    m, nh, offset);
}

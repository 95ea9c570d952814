// pam — MFMA GEMM + transpose for the MatrixMult path (gfx950/CDNA4).
//
// Y = A @ B (optionally += onto C) for row-major matrices, used by
// MPIMatrixMult block/SUMMA local products
// (ref basicoperators/MatrixMult.py:341-427, :610-765: the reference calls
// ncp.matmul on CuPy; here the panels run on hand-written MFMA kernels).
//
// Shapes (cdna_hip_programming.md §3/§5 canonical anatomy):
//   f32: v_mfma_f32_32x32x2_f32  — exact f32 at the 157 TF vector-rate peak
//        (no xf32/TF32 on gfx950); 128x128 block tile, BK=32, 4 waves as
//        2x2, each wave 2x2 MFMA tiles of 32x32 (64 acc VGPRs/lane).
//   f64: v_mfma_f64_16x16x4_f64  — 128x64 block tile, BK=16, 4 waves as
//        2x2, each wave 4x2 MFMA tiles of 16x16.
// A is staged to LDS TRANSPOSED ([k][row], +1 element row pad so the
// k-major writes and the row-major fragment reads are conflict-free);
// B is staged linear [k][col] (coalesced both ways).
// Arbitrary M/N/K via zero-padded loads + guarded stores.
//
// gemm_kernel and gemm_batched_kernel differ in their staging (how a
// K-panel gets from global memory into LDS) only: the K-panel pipeline,
// the fragment loop and the C/D walk below are shared.

#include "launch.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

template <typename T> struct GemmCfg;
template <> struct GemmCfg<float> {
  static constexpr int TM = 32;   // MFMA tile edge (square)
  static constexpr int TK = 2;    // K per MFMA
  static constexpr int BM = 128, BN = 128, BK = 32;
  // Pipeline A/Bs at 8192^3 (all NEGATIVE for f32, kept single-buffered):
  //   BK=32 NBUF=2: 135.4 -> 123.0 TF (66 KB LDS halves occupancy)
  //   BK=16 NBUF=2: 135.4 -> 131.7 TF (4 WG/CU kept, but the shallower
  //   panels double the barrier count).  f64's 128x64/BK16 panels DID
  //   gain from NBUF=2 (57.2 -> 65.1, see GemmCfg<double>).
  static constexpr int NBUF = 1;        // LDS K-panel buffers (k_pipeline)
  using acc_t = f32x16;
  using vec_t = f32x4;            // 16-B staging vector
  static constexpr int VW = 4;
  __device__ static acc_t mfma(float a, float b, acc_t c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
  }
  // C/D lane mapping for 32x32 shapes (dtype-independent on gfx950):
  // col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
  __device__ static int crow(int lane, int reg) {
    return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
  }
  static constexpr int NREG = 16;
};
template <> struct GemmCfg<double> {
  static constexpr int TM = 16;
  static constexpr int TK = 4;
  // 128x64 block tile (A/B-measured vs the earlier 64x64: the bigger M
  // tile cuts B-panel HBM traffic 25% and lifted the 8192^3 rate)
  static constexpr int BM = 128, BN = 64, BK = 16;
  static constexpr int NBUF = 2;
  using acc_t = f64x4;
  using vec_t = f64x2;
  static constexpr int VW = 2;
  __device__ static acc_t mfma(double a, double b, acc_t c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  // v_mfma_f64_16x16x4f64 C/D: col = lane&15, row = (lane>>4) + 4*reg
  // (probed empirically on gfx950 — scripts/probe_f64_mfma.hip; NOTE this
  // differs from the bf16 16x16 mapping (lane>>4)*4 + reg)
  __device__ static int crow(int lane, int reg) {
    return (lane >> 4) + 4 * reg;
  }
  static constexpr int NREG = 4;
};

// ---------------------------------------------------------------------------
// Shared by every kernel of 4 waves as 2x2 over a BM x BN block tile, each
// wave MI x NJ MFMA tiles.  LDS holds NPL planes (1 real; 2 complex: re,
// im) of NB K-panels, k-major: As[NPL][NB][BK][>= BM], Bs[..][>= BN].
// ---------------------------------------------------------------------------
struct Lane {
  int tid, lane;
  int wr, wc;   // wave row / column in the 2x2
  int li, lk;   // fragment row/col within the MFMA tile, fragment k
};

template <typename T>
__device__ __forceinline__ Lane lane_coords() {
  constexpr int TM = GemmCfg<T>::TM;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  return {tid, lane, wave >> 1, wave & 1, lane & (TM - 1), lane / TM};
}

// MFMA loop on K-panel `cur`, rows from arow of A and columns from bcol of
// B.  LDS fragments are prefetched one k-step ahead so their latency
// hides under the MFMAs (the naive form serializes ds_read -> lgkmcnt(0)
// -> MFMA per step — seen in the ISA dump).  Chain c multiplies plane
// c & 1 of A with plane (c ^ c >> 1) & 1 of B: one real chain, or the four
// of a complex product in the order rr, ii, ri, ir — independent sums, so
// no operand is negated here (the epilogue combines them).
template <typename T, int NPL, int NB, int BK, int LA, int LB, int MI, int NJ>
__device__ __forceinline__ void mma_panel(
    const T (&As)[NPL][NB][BK][LA], const T (&Bs)[NPL][NB][BK][LB], int cur,
    int arow, int bcol, const Lane& ln,
    typename GemmCfg<T>::acc_t (&acc)[NPL * NPL][MI][NJ]) {
  using CFG = GemmCfg<T>;
  constexpr int TM = CFG::TM, TK = CFG::TK;
  T a[2][MI][NPL], b[2][NJ][NPL];
  auto fetch = [&](int f, int krow) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl)
        a[f][mi][pl] = As[pl][cur][krow][arow + mi * TM + ln.li];
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl)
        b[f][nj][pl] = Bs[pl][cur][krow][bcol + nj * TM + ln.li];
  };
  fetch(0, ln.lk);
#pragma unroll
  for (int kk = 0; kk < BK / TK; ++kk) {
    const int cf = kk & 1, nf = (kk + 1) & 1;
    if (kk + 1 < BK / TK) fetch(nf, (kk + 1) * TK + ln.lk);
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int c = 0; c < NPL * NPL; ++c)
          acc[c][mi][nj] = CFG::mfma(a[cf][mi][c & 1],
                                     b[cf][nj][(c ^ (c >> 1)) & 1],
                                     acc[c][mi][nj]);
  }
}

// K-panel pipeline over NP panels of depth BK: load(k0) reads a panel from
// global memory into registers, store(buf) writes them to LDS panel buf.
// The next panel's global loads are issued BEFORE the MFMA loop on the
// current panel and parked in registers, so the HBM latency hides under
// compute.  NB=2: the LDS store goes to the other buffer, one barrier per
// panel.  NB=1 keeps the classic 2-barrier structure (f32 gemm_kernel:
// doubling LDS would halve occupancy; measured best single-buffered).
template <typename T, int NPL, int NB, int BK, int LA, int LB, int MI, int NJ,
          typename Load, typename Store>
__device__ __forceinline__ void k_pipeline(
    int64_t NP, Load&& load, Store&& store, T (&As)[NPL][NB][BK][LA],
    T (&Bs)[NPL][NB][BK][LB], int arow, int bcol, const Lane& ln,
    typename GemmCfg<T>::acc_t (&acc)[NPL * NPL][MI][NJ]) {
  // K = 0: no panel.  (A block, not an early return: with `return` the
  // real f32 transposed-A kernels came out 4 VGPRs, one wave/SIMD, worse.)
  if (NP > 0) {
    load(0);
    store(0);
    __syncthreads();
    for (int64_t p = 0; p < NP; ++p) {
      if (p + 1 < NP) load((p + 1) * BK);
      mma_panel(As, Bs, (int)(p % NB), arow, bcol, ln, acc);
      if (p + 1 < NP) {
        if (NB == 1) __syncthreads();  // readers done before overwrite
        store((int)((p + 1) % NB));
        __syncthreads();
      }
    }
  }
}

// C/D fragment layout -> put(row, col, mi, nj, reg) for every element of
// the wave's tiles (origin r0, c0) that lies inside M x N.
template <typename T, int MI, int NJ, bool GUARD, typename Put>
__device__ __forceinline__ void for_each_c(const Lane& ln, int64_t r0,
                                           int64_t c0, int64_t M, int64_t N,
                                           Put&& put) {
  using CFG = GemmCfg<T>;
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) {
      const int64_t cc = c0 + nj * CFG::TM + ln.li;
      if (GUARD && cc >= N) continue;
#pragma unroll
      for (int reg = 0; reg < CFG::NREG; ++reg) {
        const int64_t rr = r0 + mi * CFG::TM + CFG::crow(ln.lane, reg);
        if (!GUARD || rr < M) put(rr, cc, mi, nj, reg);
      }
    }
}

template <bool ACC, typename T>
__device__ __forceinline__ void emit(T& dst, T v) {
  if constexpr (ACC) dst += v;
  else dst = v;
}

// C = A@B (+C when ACC), A [M,K] lda, B [K,N] ldb, C [M,N] ldc, row-major.
// Staging: 16-byte vector loads (scalar, zero-padded at the edges when
// GUARD); A is transposed on its way into LDS.
template <typename T, bool ACC, bool GUARD>
__global__ void __launch_bounds__(BLK) gemm_kernel(
    const T* __restrict__ A, const T* __restrict__ B, T* __restrict__ C,
    int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc) {
  using CFG = GemmCfg<T>;
  constexpr int BM = CFG::BM, BN = CFG::BN, BK = CFG::BK;
  constexpr int TM = CFG::TM, VW = CFG::VW;
  constexpr int MI = (BM / 2) / TM, NJ = (BN / 2) / TM;
  using vec_t = typename CFG::vec_t;

  __shared__ T As[1][CFG::NBUF][BK][BM + 1];  // transposed, padded
  __shared__ T Bs[1][CFG::NBUF][BK][BN];       // linear

  const Lane ln = lane_coords<T>();
  const int tid = ln.tid;

  // NOTE: an XCD-aware bijective tile remap (T1) was measured and
  // REGRESSED this kernel (f32 4096^3: 97->83 TF; 8192^3: 110->101 TF;
  // f64: 49.7->46.7) — the 128^2-tile structure is MFMA-issue-bound here,
  // not HBM-bound, so the remap only disturbed dispatch locality.
  const int64_t brow = (int64_t)blockIdx.y * BM;
  const int64_t bcol = (int64_t)blockIdx.x * BN;

  typename CFG::acc_t acc[1][MI][NJ] = {};

  constexpr int AV = (BM * BK) / VW / BLK;  // A vector loads per thread
  constexpr int BV = (BK * BN) / VW / BLK;  // B vector loads per thread
  vec_t areg[AV], breg[BV];

  auto load_panel = [&](int64_t k0) {
#pragma unroll
    for (int e = 0; e < AV; ++e) {
      const int vi = tid + BLK * e;
      const int row = vi / (BK / VW);
      const int kv = vi % (BK / VW);
      const int64_t gr = brow + row;
      if (!GUARD || (gr < M && k0 + (int64_t)kv * VW + VW <= K)) {
        areg[e] = *reinterpret_cast<const vec_t*>(A + gr * lda + k0
                                                  + (int64_t)kv * VW);
      } else {
#pragma unroll
        for (int j = 0; j < VW; ++j) {
          const int64_t gk = k0 + kv * VW + j;
          areg[e][j] = (gr < M && gk < K) ? A[gr * lda + gk] : (T)0;
        }
      }
    }
#pragma unroll
    for (int e = 0; e < BV; ++e) {
      const int vi = tid + BLK * e;
      const int kb = vi / (BN / VW);
      const int nv = vi % (BN / VW);
      const int64_t gk = k0 + kb;
      const int64_t gn = bcol + (int64_t)nv * VW;
      if (!GUARD || (gk < K && gn + VW <= N)) {
        breg[e] = *reinterpret_cast<const vec_t*>(B + gk * ldb + gn);
      } else {
#pragma unroll
        for (int j = 0; j < VW; ++j)
          breg[e][j] = (gk < K && gn + j < N) ? B[gk * ldb + gn + j] : (T)0;
      }
    }
  };

  auto store_panel = [&](int buf) {
#pragma unroll
    for (int e = 0; e < AV; ++e) {
      const int vi = tid + BLK * e;
      const int row = vi / (BK / VW);
      const int kv = vi % (BK / VW);
#pragma unroll
      for (int j = 0; j < VW; ++j) As[0][buf][kv * VW + j][row] = areg[e][j];
    }
#pragma unroll
    for (int e = 0; e < BV; ++e) {
      const int vi = tid + BLK * e;
      const int kb = vi / (BN / VW);
      const int nv = vi % (BN / VW);
      *reinterpret_cast<vec_t*>(&Bs[0][buf][kb][nv * VW]) = breg[e];
    }
  };

  k_pipeline(GUARD ? (K + BK - 1) / BK : K / BK, load_panel, store_panel, As,
             Bs, ln.wr * (BM / 2), ln.wc * (BN / 2), ln, acc);

  for_each_c<T, MI, NJ, GUARD>(
      ln, brow + ln.wr * (BM / 2), bcol + ln.wc * (BN / 2), M, N,
      [&](int64_t rr, int64_t cc, int mi, int nj, int reg) {
        emit<ACC>(C[rr * ldc + cc], acc[0][mi][nj][reg]);
      });
}

template <typename T>
static int gemm_launch(void* stream, const void* A, const void* B, void* C,
                       int64_t M, int64_t N, int64_t K, int64_t lda,
                       int64_t ldb, int64_t ldc, int accumulate) {
  using CFG = GemmCfg<T>;
  if (M <= 0 || N <= 0 || K < 0 || !A || !B || !C) return PAM_EARG;
  // a leading dimension shorter than its row would read the wrong rows
  if (lda < K || ldb < N || ldc < N) return PAM_EARG;
  dim3 grid((uint32_t)((N + CFG::BN - 1) / CFG::BN),
            (uint32_t)((M + CFG::BM - 1) / CFG::BM));
  const bool aligned = (M % CFG::BM == 0) && (N % CFG::BN == 0) &&
                       (K % CFG::BK == 0);
  with_bool(accumulate, [&](auto acc) {
    with_bool(!aligned, [&](auto guard) {
      hipLaunchKernelGGL((gemm_kernel<T, acc(), guard()>), grid, dim3(BLK),
                         0, (hipStream_t)stream, (const T*)A, (const T*)B,
                         (T*)C, M, N, K, lda, ldb, ldc);
    });
  });
  return check(hipGetLastError());
}

extern "C" int pam_gemm(void* stream, const void* A, const void* B, void* C,
                        int64_t M, int64_t N, int64_t K, int64_t lda,
                        int64_t ldb, int64_t ldc, int accumulate, int dtype) {
  if (dtype == PAM_F64)
    return gemm_launch<double>(stream, A, B, C, M, N, K, lda, ldb, ldc,
                               accumulate);
  if (dtype == PAM_F32)
    return gemm_launch<float>(stream, A, B, C, M, N, K, lda, ldb, ldc,
                              accumulate);
  return PAM_EDTYPE;
}

// ---------------------------------------------------------------------------
// batched GEMM: C_b (+)= op(A_b) @ B_b over blockIdx.z, dense row-major
// matrices of NPL values per element: 1 real (op = N or transpose), 2
// interleaved (re,im) complex (op = N or conj-transpose).  The Fredholm1
// batched integral kernel (ref signalprocessing/Fredholm1.py:123,149-156
// `ncp.matmul(G, x)` on a 3-D G); the z-batched grid fills the chip where
// a pam_gemm per slice from Python left it empty (513 launches of 4
// workgroups each at the cfg5 shape, plus the ctypes overhead).
//
// Complex MFMA formulation: four independent accumulation chains per
// output tile (ar*br, ai*bi, ar*bi, ai*br) over separate re/im LDS planes;
// the epilogue combines Cr = S_rr - S_ii, Ci = S_ri + S_ir.  This replaced
// a VALU outer-product kernel (r01 A/B at the judged cfg5 shape
// 513x(64x256x256) c64: VALU 24.6 TF real-flops = 63% of the ~39 TF VALU
// ceiling; the MFMA version's numbers are in DESIGN.md) — the batch
// dimension fills the chip either way, but only MFMA reaches the
// matrix-core rate.
// ---------------------------------------------------------------------------
template <typename T, int NPL, bool CT, bool ACC, int BK>
__global__ void __launch_bounds__(BLK) gemm_batched_kernel(
    const T* __restrict__ A, const T* __restrict__ B, T* __restrict__ C,
    int64_t M, int64_t N, int64_t K, int64_t strideA, int64_t strideB,
    int64_t strideC) {
  using CFG = GemmCfg<T>;
  // 64x64 block tile, double-buffered BK-deep panels (BK: see cgemm_bk).
  // A/B'd alternatives, all NEGATIVE at cfg5 complex:
  //   BK=32 (49.5 -> 37.2 TF), BK=64 single-panel (0.432 -> 0.518 ms
  //   rmatvec: the 133 KB LDS footprint drops occupancy to 2 WG/CU, which
  //   costs more than the three extra barriers it saves), f32 BN=128 wide
  //   tile (69.2 -> 66.2 TF: halving the WG count costs more latency
  //   hiding than the doubled fragment reuse gains), 128x64 tile for the
  //   shallow-K adjoint (-15% rmatvec; its double kernels spilled),
  //   single-buffered panels (-5%).
  constexpr int BM = 64, BN = 64, NB = 2;
  constexpr int MI = (BM / 2) / CFG::TM, NJ = (BN / 2) / CFG::TM;

  __shared__ T As[NPL][NB][BK][BM + 1];  // k-major
  __shared__ T Bs[NPL][NB][BK][BN + 1];
  const int64_t b = blockIdx.z;
  const T* __restrict__ Ab = A + NPL * b * strideA;
  const T* __restrict__ Bb = B + NPL * b * strideB;
  T* __restrict__ Cb = C + NPL * b * strideC;
  const int64_t m0 = (int64_t)blockIdx.y * BM;
  const int64_t n0 = (int64_t)blockIdx.x * BN;
  const Lane ln = lane_coords<T>();

  typename CFG::acc_t acc[NPL * NPL][MI][NJ] = {};

  constexpr int AE = (BM * BK) / BLK;
  constexpr int BE = (BK * BN) / BLK;
  T areg[AE][NPL], breg[BE][NPL];

  // element e of this thread in the A panel -> (k, m); consecutive threads
  // follow the contiguous direction of A: m when A is [K, M] (CT), else k
  auto a_km = [&](int e, int& kk, int& mm) {
    const int v = ln.tid + BLK * e;
    if constexpr (CT) {
      mm = v & (BM - 1);
      kk = v / BM;
    } else {
      kk = v & (BK - 1);
      mm = v / BK;
    }
  };

  auto load_panel = [&](int64_t k0) {
#pragma unroll
    for (int e = 0; e < AE; ++e) {
      int kk, mm;
      a_km(e, kk, mm);
      const int64_t gm = m0 + mm;
      const int64_t gk = k0 + kk;
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) {
        T v = 0;
        if (gm < M && gk < K) {
          v = Ab[NPL * (CT ? gk * M + gm : gm * K + gk) + pl];
          // op(A)[m][k] = conj(A[k][m]); a real transpose has no plane 1
          if (CT && pl == 1) v = -v;
        }
        areg[e][pl] = v;
      }
    }
#pragma unroll
    for (int e = 0; e < BE; ++e) {
      const int v = ln.tid + BLK * e;
      const int64_t gk = k0 + v / BN;
      const int64_t gn = n0 + (v & (BN - 1));
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl)
        breg[e][pl] =
            (gk < K && gn < N) ? Bb[NPL * (gk * N + gn) + pl] : (T)0;
    }
  };

  auto store_panel = [&](int buf) {
#pragma unroll
    for (int e = 0; e < AE; ++e) {
      int kk, mm;
      a_km(e, kk, mm);
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) As[pl][buf][kk][mm] = areg[e][pl];
    }
#pragma unroll
    for (int e = 0; e < BE; ++e) {
      const int v = ln.tid + BLK * e;
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl)
        Bs[pl][buf][v / BN][v & (BN - 1)] = breg[e][pl];
    }
  };

  k_pipeline((K + BK - 1) / BK, load_panel, store_panel, As, Bs,
             ln.wr * (BM / 2), ln.wc * (BN / 2), ln, acc);

  for_each_c<T, MI, NJ, true>(
      ln, m0 + ln.wr * (BM / 2), n0 + ln.wc * (BN / 2), M, N,
      [&](int64_t rr, int64_t cc, int mi, int nj, int reg) {
        const int64_t off = NPL * (rr * N + cc);
        if constexpr (NPL == 1) {
          emit<ACC>(Cb[off], acc[0][mi][nj][reg]);
        } else {  // Cr = S_rr - S_ii, Ci = S_ri + S_ir
          emit<ACC>(Cb[off], acc[0][mi][nj][reg] - acc[1][mi][nj][reg]);
          emit<ACC>(Cb[off + 1], acc[2][mi][nj][reg] + acc[3][mi][nj][reg]);
        }
      });
}

// Panel depth of the complex kernel without accumulate (with accumulate,
// and for real data, 16).  r02 sweep at the cfg5 shapes
// (profiles/r02s5/sweep.log): BK=8 wins the shallow-K adjoint (K=64:
// 0.262->0.240 ms saveGt=off, 0.206->0.200 on) and loses the K=256 matvec
// (0.207->0.218), so K<=64 auto-selects BK=8; PAM_CGEMM_BK=8 / 16 (read
// once per process) forces the shallow / the deep panel.
static int cgemm_bk(int64_t K) {
  static const int bkov = (int)env_int("PAM_CGEMM_BK", 0);
  return (bkov == 8 || (bkov == 0 && K <= 64)) ? 8 : 16;
}

template <typename T, int NPL>
static int batched_launch(void* stream, const void* A, const void* B, void* C,
                          int64_t batch, int64_t M, int64_t N, int64_t K,
                          int64_t sA, int64_t sB, int64_t sC, int opa,
                          int acc) {
  if (batch <= 0 || M <= 0 || N <= 0 || K < 0 || !A || !B || !C)
    return PAM_EARG;
  dim3 grid((uint32_t)((N + 63) / 64), (uint32_t)((M + 63) / 64),
            (uint32_t)batch);
  auto launch = [&](auto ct, auto ac, auto bk) {
    hipLaunchKernelGGL((gemm_batched_kernel<T, NPL, ct(), ac(), bk()>), grid,
                       dim3(BLK), 0, (hipStream_t)stream, (const T*)A,
                       (const T*)B, (T*)C, M, N, K, sA, sB, sC);
  };
  using BK8 = std::integral_constant<int, 8>;
  using BK16 = std::integral_constant<int, 16>;
  with_bool(opa, [&](auto ct) {
    if constexpr (NPL == 2) {
      if (!acc && cgemm_bk(K) == 8) {
        launch(ct, std::false_type{}, BK8{});
        return;
      }
    }
    with_bool(acc, [&](auto ac) { launch(ct, ac, BK16{}); });
  });
  return check(hipGetLastError());
}

extern "C" int pam_cgemm_batched(void* stream, const void* A, const void* B,
                                 void* C, int64_t batch, int64_t M, int64_t N,
                                 int64_t K, int64_t strideA, int64_t strideB,
                                 int64_t strideC, int opa, int accumulate,
                                 int dtype) {
  if (dtype == PAM_C128)
    return batched_launch<double, 2>(stream, A, B, C, batch, M, N, K, strideA,
                                     strideB, strideC, opa, accumulate);
  if (dtype == PAM_C64)
    return batched_launch<float, 2>(stream, A, B, C, batch, M, N, K, strideA,
                                    strideB, strideC, opa, accumulate);
  return PAM_EDTYPE;
}

extern "C" int pam_gemm_batched(void* stream, const void* A, const void* B,
                                void* C, int64_t batch, int64_t M, int64_t N,
                                int64_t K, int64_t strideA, int64_t strideB,
                                int64_t strideC, int opa, int accumulate,
                                int dtype) {
  if (dtype == PAM_F64)
    return batched_launch<double, 1>(stream, A, B, C, batch, M, N, K, strideA,
                                     strideB, strideC, opa, accumulate);
  if (dtype == PAM_F32)
    return batched_launch<float, 1>(stream, A, B, C, batch, M, N, K, strideA,
                                    strideB, strideC, opa, accumulate);
  return PAM_EDTYPE;
}

// ---------------------------------------------------------------------------
// LDS-tiled transpose: At[c][r] = A[r][c] for elements of NV values — 1
// real; 2 an interleaved (re,im) pair, conjugated when CONJ.  Materializes
// the adjoint's A^T / A^H panels (ref MatrixMult.py:416,737 "A.T.conj()").
// 32x32 tiles, +1 pad against bank conflicts.
// ---------------------------------------------------------------------------
template <typename T, int NV, bool CONJ>
__global__ void __launch_bounds__(BLK) transpose_kernel(
    const T* __restrict__ A, T* __restrict__ At, int64_t nr, int64_t nc) {
  __shared__ T tile[32][33][NV];
  const int64_t r0 = (int64_t)blockIdx.y * 32;
  const int64_t c0 = (int64_t)blockIdx.x * 32;
  const int tr = threadIdx.x / 32;   // 8 rows of 32 threads
  const int tc = threadIdx.x % 32;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t r = r0 + tr + 8 * i;
    if (r < nr && c0 + tc < nc) {
      const int64_t off = NV * (r * nc + c0 + tc);
#pragma unroll
      for (int v = 0; v < NV; ++v)
        tile[tr + 8 * i][tc][v] = (CONJ && v == 1) ? -A[off + v] : A[off + v];
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t c = c0 + tr + 8 * i;
    if (c < nc && r0 + tc < nr) {
      const int64_t off = NV * (c * nr + r0 + tc);
#pragma unroll
      for (int v = 0; v < NV; ++v) At[off + v] = tile[tc][tr + 8 * i][v];
    }
  }
}

template <typename T, int NV, bool CONJ = false>
static int transpose_launch(void* stream, const void* A, void* At, int64_t nr,
                            int64_t nc) {
  dim3 grid((uint32_t)((nc + 31) / 32), (uint32_t)((nr + 31) / 32));
  hipLaunchKernelGGL((transpose_kernel<T, NV, CONJ>), grid, dim3(BLK), 0,
                     (hipStream_t)stream, (const T*)A, (T*)At, nr, nc);
  return check(hipGetLastError());
}

extern "C" int pam_ctranspose(void* stream, const void* A, void* At,
                              int64_t nr, int64_t nc, int conj, int dtype) {
  if (nr <= 0 || nc <= 0 || !A || !At) return PAM_EARG;
  int rc = PAM_EDTYPE;
  with_bool(conj, [&](auto cj) {
    if (dtype == PAM_C128)
      rc = transpose_launch<double, 2, cj()>(stream, A, At, nr, nc);
    else if (dtype == PAM_C64)
      rc = transpose_launch<float, 2, cj()>(stream, A, At, nr, nc);
  });
  return rc;
}

extern "C" int pam_transpose(void* stream, const void* A, void* At,
                             int64_t nr, int64_t nc, int dtype) {
  if (nr <= 0 || nc <= 0 || !A || !At) return PAM_EARG;
  if (dtype == PAM_F64)
    return transpose_launch<double, 1>(stream, A, At, nr, nc);
  if (dtype == PAM_F32)
    return transpose_launch<float, 1>(stream, A, At, nr, nc);
  return PAM_EDTYPE;
}

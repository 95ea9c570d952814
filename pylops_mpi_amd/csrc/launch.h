// launch.h — the host-side launch helpers every .hip file shares: the error
// code, the block size, the environment reader and the runtime-value ->
// template-argument dispatchers.  Plain functions only.
#ifndef PAM_LAUNCH_H
#define PAM_LAUNCH_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>
#include <utility>

#include "../../include/pam.h"

#define BLK 256  // threads per block of every kernel (4 waves of 64)

static inline int check(hipError_t e) { return (int)e; }

// Integer knob from the environment; unset or empty gives dflt.  The caller
// decides how often to read: `static const` for once per process.
static inline int64_t env_int(const char* name, int64_t dflt) {
  const char* e = getenv(name);
  return (e && *e) ? atoll(e) : dflt;
}

// f(std::integral_constant<int, 0>{}) ... f(std::integral_constant<int,
// N-1>{}), in order: a loop whose index is a compile-time constant inside f.
template <typename F, int... Is>
__host__ __device__ __forceinline__ void fd_unroll_seq(
    F&& f, std::integer_sequence<int, Is...>) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, typename F>
__host__ __device__ __forceinline__ void fd_unroll(F&& f) {
  fd_unroll_seq(f, std::make_integer_sequence<int, N>{});
}

// Runtime flag -> template argument: f(std::true_type{}) or
// f(std::false_type{}); nest one call per flag.
template <typename F>
static inline void with_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

// Runtime integer -> template argument: returns
// f(std::integral_constant<int, v>{}) for v in [Lo, Hi], err otherwise.
template <int Lo, int Hi, typename F>
static inline int with_int(int64_t v, int err, F&& f) {
  int rc = err;
  fd_unroll<Hi - Lo + 1>([&](auto i) {
    if (v == Lo + decltype(i)::value)
      rc = f(std::integral_constant<int, Lo + decltype(i)::value>{});
  });
  return rc;
}

// dtype code -> element type: f(type_tag<T>{}) with T the real base type
// (`using T = typename decltype(t)::type;` inside f).  with_real takes the
// two real codes, with_cplx the two complex ones, with_dtype all four and
// passes std::bool_constant<CPLX> as well; PAM_EDTYPE for any other code.
template <typename T> struct type_tag { using type = T; };

template <typename F>
static inline int with_dtype(int dtype, F&& f) {
  switch (dtype) {
    case PAM_F64: return f(type_tag<double>{}, std::false_type{});
    case PAM_F32: return f(type_tag<float>{}, std::false_type{});
    case PAM_C128: return f(type_tag<double>{}, std::true_type{});
    case PAM_C64: return f(type_tag<float>{}, std::true_type{});
    default: return PAM_EDTYPE;
  }
}
template <typename F>
static inline int with_real(int dtype, F&& f) {
  if (dtype != PAM_F64 && dtype != PAM_F32) return PAM_EDTYPE;
  return with_dtype(dtype, [&](auto t, auto) { return f(t); });
}
template <typename F>
static inline int with_cplx(int dtype, F&& f) {
  if (dtype != PAM_C128 && dtype != PAM_C64) return PAM_EDTYPE;
  return with_dtype(dtype, [&](auto t, auto) { return f(t); });
}

#endif  // PAM_LAUNCH_H

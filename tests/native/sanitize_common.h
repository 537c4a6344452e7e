// sanitize_common.h — what the stand-alone sanitizer programs of this folder share: EXPECT with
// its failure counter, the dtype codes of a value / index type, and a seeded generator.  Each
// program sets its own seed and keeps what only it uses (a tolerance of its own, its data).
#ifndef OFX_TESTS_SANITIZE_COMMON_H_
#define OFX_TESTS_SANITIZE_COMMON_H_

#include <cstdint>
#include <cstdio>

#include "ofx_spmm.h"
#include "spmm_common.h"

inline int g_failures = 0;

#define EXPECT(cond, ...)                        \
  do {                                           \
    if (!(cond)) {                               \
      ++g_failures;                              \
      fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);              \
      fprintf(stderr, "\n");                     \
    }                                            \
  } while (0)

// The dtype code of T and the tolerance of a result of T against a naive double loop.
template <typename T>
struct Code;
template <>
struct Code<float> {
  static constexpr int dt = OFX_DT_FLOAT;
  static constexpr double tol = 1e-6;
};
template <>
struct Code<double> {
  static constexpr int dt = OFX_DT_DOUBLE;
  static constexpr double tol = 1e-14;
};
template <>
struct Code<ofx::bf16> {
  static constexpr int dt = OFX_DT_BFLOAT16;
  static constexpr double tol = 1e-2;
};
template <>
struct Code<ofx::f16> {
  static constexpr int dt = OFX_DT_FLOAT16;
  static constexpr double tol = 2e-3;
};
template <typename I>
constexpr int idx_code() {
  return sizeof(I) == 4 ? OFX_DT_INT32 : OFX_DT_INT64;
}

// splitmix64 from the seed a program sets before its first draw.
inline uint64_t g_rng = 0;
inline uint64_t next() { return g_rng = ofx::splitmix64(g_rng); }
inline double uniform() { return (double)(next() >> 11) / 9007199254740992.0; }  // [0, 1)

#endif  // OFX_TESTS_SANITIZE_COMMON_H_

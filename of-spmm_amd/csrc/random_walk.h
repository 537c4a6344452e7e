// random_walk.h — what the kCPU kernel (random_walk_cpu.cpp) and the HIP kernels (random_walk.hip)
// of the random walks share: the acceptance thresholds of node2vec's bias, the check of a row a
// walk stands on, the words of an attempt, the class of a candidate, the step in its sequential
// form and the argument checks of the C-ABI entries (contract in include/ofx_spmm.h, DESIGN.md
// §3n).  The generator is the neighbour sampler's (sample_neighbors.h).  Integers only.
//
// Walk i starts at starts[i].  Step t = 1..length stands on v = walks[i, t-1] and draws attempts
// a = 0, 1, ...: the words (w0, w1) of philox4x32-10 under counter (i lo, i hi, t, a) and the
// seed as key give the candidate position r = (w0 * deg(v)) >> 32 of row v and its acceptance
// word w1.  The candidate x is accepted iff w1 < thr[class of x], the class against the node
// u = walks[i, t-2] before v: return (x == u), common (x is a column of row u) or out.  Step 1 has
// no u and accepts attempt 0; attempt kMaxAttempts - 1 is accepted whatever its class.
//
// Bias: the multiply-shift draw is off by at most deg / 2^32 of itself, as the sampler's; forcing
// the last attempt moves at most (1 - min(thr) / 2^32)^256 of a step's probability, 7e-8 at a
// ratio of 16 between the largest and the smallest weight.
#ifndef OFX_RANDOM_WALK_H_
#define OFX_RANDOM_WALK_H_

#include <climits>
#include <cmath>

#include "ofx_internal.h"
#include "sample_neighbors.h"
#include "spmm_common.h"

namespace ofx {
namespace rw {

constexpr int kMaxAttempts = 256;
constexpr int kMaxLength = 65535;
constexpr uint64_t kAlways = 1ull << 32;  // above every 32-bit word: the class is always accepted
enum Class { kReturn = 0, kCommon = 1, kOut = 2 };

// thr[c] / 2^32 is the acceptance probability of class c: its weight over the largest weight.
struct Thresholds {
  uint64_t thr[3];
};

// The thresholds of (p, q), host; false for a p or q that is not finite and > 0.  The largest
// weight gets 2^32 itself; the others floor((w / max) * 2^32), the scaling being exact in double.
static inline bool thresholds_of(double p, double q, Thresholds* out) {
  if (!(std::isfinite(p) && std::isfinite(q) && p > 0.0 && q > 0.0)) return false;
  const double w[3] = {1.0 / p, 1.0, 1.0 / q};
  const double mx = std::fmax(w[0], std::fmax(w[1], w[2]));
  for (int c = 0; c < 3; ++c)
    out->thr[c] = w[c] == mx ? kAlways : (uint64_t)std::floor((w[c] / mx) * 4294967296.0);
  return true;
}

// thr[c] by selects: c differs between lanes, and an indexed read of the struct would spill it.
OFX_HD uint64_t threshold(const Thresholds& t, int c) {
  return c == kReturn ? t.thr[kReturn] : c == kCommon ? t.thr[kCommon] : t.thr[kOut];
}

// Every attempt 0 is accepted: the walk is a first-order one and needs no search.
OFX_HD bool first_order(const Thresholds& t) {
  return t.thr[kReturn] == kAlways && t.thr[kCommon] == kAlways && t.thr[kOut] == kAlways;
}

// The row a walk stands on.  ended: v is no row (-1, a column >= m of a non-square CSR) or its
// row is empty or bad; bad: the degree is outside [0, 2^31) or the entries leave [0, nnz).
// row_ptr is read only for v inside [0, m); [begin, end) is used only when !ended.
struct Row {
  int64_t begin;
  int64_t end;
  bool ended;
  bool bad;
};
template <typename I>
OFX_HD Row row_of(const I* __restrict__ row_ptr, int64_t m, int64_t nnz, int64_t v) {
  Row r{0, 0, true, false};
  if (v < 0 || v >= m) return r;
  const int64_t lo = (int64_t)row_ptr[v];
  const int64_t hi = (int64_t)row_ptr[v + 1];
  if (lo < 0 || hi < lo || hi > nnz || hi - lo > (int64_t)INT32_MAX) {
    r.bad = true;
    return r;
  }
  r.begin = lo;
  r.end = hi;
  r.ended = hi == lo;
  return r;
}

// The two words of attempt a of step t of walk i.
OFX_HD void attempt_words(uint64_t i, uint32_t t, uint32_t a, uint64_t seed, uint32_t* w0,
                          uint32_t* w1) {
  uint32_t c[4] = {(uint32_t)i, (uint32_t)(i >> 32), t, a};
  smp::philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  *w0 = c[0];
  *w1 = c[1];
}

// The candidate's entry: position (w0 * deg) >> 32 of the row.  0 < deg < 2^31.
OFX_HD int64_t candidate(int64_t begin, int64_t deg, uint32_t w0) {
  return begin + (int64_t)(((uint64_t)w0 * (uint64_t)deg) >> 32);
}

// Lower bound of x over [lo, hi) of col_idx, then the compare: whether row u holds column x (for
// ascending columns; on other rows still a function of the row alone, inside the row).
template <typename I>
OFX_HD bool row_has(const I* __restrict__ col_idx, int64_t lo, int64_t hi, int64_t x) {
  const int64_t end = hi;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if ((int64_t)col_idx[mid] < x)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < end && (int64_t)col_idx[lo] == x;
}

// The class of candidate x against the previous node u, whose row is [ub, ue).  The search is
// skipped where it cannot change the outcome (common and out share a threshold).
template <typename I>
OFX_HD int class_of(const I* __restrict__ col_idx, int64_t u, int64_t ub, int64_t ue, int64_t x,
                    bool search) {
  if (x == u) return kReturn;
  if (!search) return kOut;
  return row_has(col_idx, ub, ue, x) ? kCommon : kOut;
}

// One step, sequential: the accepted entry e of row [vb, ve) (not empty).  has_prev is t >= 2.
template <typename I>
OFX_HD int64_t step(const I* __restrict__ col_idx, uint64_t i, uint32_t t, uint64_t seed,
                    const Thresholds& th, int64_t vb, int64_t ve, bool has_prev, int64_t u,
                    int64_t ub, int64_t ue) {
  const bool search = th.thr[kCommon] != th.thr[kOut];
  for (uint32_t a = 0;; ++a) {
    uint32_t w0, w1;
    attempt_words(i, t, a, seed, &w0, &w1);
    const int64_t e = candidate(vb, ve - vb, w0);
    if (!has_prev || a == (uint32_t)(kMaxAttempts - 1)) return e;
    const int c = class_of(col_idx, u, ub, ue, (int64_t)col_idx[e], search);
    if ((uint64_t)w1 < threshold(th, c)) return e;
  }
}

// The checks every entry shares (host).
static inline int check_walk_args(const char* fn, int idx_dtype, int64_t m, int64_t nnz,
                                  int64_t num_walks, const void* row_ptr, const void* col_idx,
                                  const void* starts, int length, double p, double q,
                                  const void* out_walks, Thresholds* th) {
  OFX_REQUIRE(is_index_dtype(idx_dtype), OFX_EUNSUPPORTED, "%s: index dtype %d is not int32/int64",
              fn, idx_dtype);
  OFX_REQUIRE(length >= 1 && length <= kMaxLength, OFX_EINVAL, "%s: length %d outside [1, %d]", fn,
              length, kMaxLength);
  OFX_REQUIRE(m >= 0 && m <= (int64_t)INT32_MAX && nnz >= 0 && nnz <= (int64_t)INT32_MAX &&
                  num_walks >= 0 && num_walks <= (int64_t)INT32_MAX,
              OFX_EINVAL, "%s: m=%lld, nnz=%lld or num_walks=%lld is not in [0, 2^31)", fn,
              (long long)m, (long long)nnz, (long long)num_walks);
  OFX_REQUIRE(thresholds_of(p, q, th), OFX_EINVAL, "%s: p=%g and q=%g must be finite and > 0", fn,
              p, q);
  OFX_REQUIRE(row_ptr && (nnz == 0 || col_idx), OFX_EINVAL, "%s: NULL pointer", fn);
  OFX_REQUIRE(num_walks == 0 || (starts && out_walks), OFX_EINVAL, "%s: NULL pointer", fn);
  return OFX_OK;
}

}  // namespace rw
}  // namespace ofx

#endif  // OFX_RANDOM_WALK_H_

// sample_neighbors.h — what the kCPU kernel (sample_neighbors_cpu.cpp) and the HIP kernels
// (sample_neighbors.hip) of the neighbour sampler share: the counter-based generator, the draw of
// one Floyd step, the step itself, the row routine in its sequential form and the argument checks
// of the C-ABI entries (contract in include/ofx_spmm.h).
//
// A row v of degree deg > fanout keeps a uniform subset of `fanout` of its positions 0..deg-1,
// drawn without replacement by Floyd's algorithm and written in ascending order.  Step t
// (t = 0..fanout-1) draws r uniformly from [0, j], j = deg - fanout + t, and keeps r unless an
// earlier step kept it, in which case it keeps j (which no earlier step can have kept: every
// earlier pick is at most j - 1).  The draw is r = (u * (j + 1)) >> 32 from one 32-bit word u of
// philox4x32-10 whose counter is (v, t) and whose key is the caller's seed: it depends on the node
// and the step alone, so the `fanout` draws of a row are independent of each other (the HIP kernel
// computes them in parallel, one per lane) and of where, or how often, v stands among the seeds.
//
// Bias: the multiply-shift maps 2^32 values of u onto j + 1 <= deg results, so some results get
// one value more than others: the probability of a result is off by at most deg / 2^32 of itself,
// which is below 5e-6 for every degree up to 20000 and reaches one half only at the 2^31 limit.
#ifndef OFX_SAMPLE_NEIGHBORS_H_
#define OFX_SAMPLE_NEIGHBORS_H_

#include <climits>

#include "ofx_internal.h"
#include "spmm_common.h"

namespace ofx {
namespace smp {

constexpr int kMaxFanout = 64;

// philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
// SC'11): the published multipliers, Weyl constants and round count.  c is replaced by the output.
OFX_HD void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1;
    c[3] = (uint32_t)p0;
    c[0] = n0;
    c[2] = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// The draw of step t of node v: uniform in [0, j] up to the bias above.  j < 2^31.
OFX_HD uint32_t draw(uint64_t v, uint32_t t, uint64_t seed, uint32_t j) {
  uint32_t c[4] = {(uint32_t)v, (uint32_t)(v >> 32), t, 0u};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  return (uint32_t)(((uint64_t)c[0] * (uint64_t)(j + 1u)) >> 32);
}

// Floyd's step: r, or j when an earlier step already kept r.
OFX_HD uint32_t floyd_pick(uint32_t r, uint32_t j, bool r_taken) { return r_taken ? j : r; }

// What a seed gives before anything is drawn.  len = min(deg, fanout), 0 for a bad seed; bad: the
// seed is outside [0, m) or its row's degree is outside [0, 2^31).  row_ptr is read only for a
// seed inside [0, m).
struct RowOf {
  int64_t begin;
  int64_t deg;
  int len;
  bool bad;
};
template <typename I>
OFX_HD RowOf row_of(const I* __restrict__ row_ptr, int64_t m, int64_t v, int fanout) {
  RowOf r{0, 0, 0, true};
  if (v < 0 || v >= m) return r;
  r.begin = (int64_t)row_ptr[v];
  r.deg = (int64_t)row_ptr[v + 1] - r.begin;
  if (r.deg < 0 || r.deg > (int64_t)INT32_MAX) {
    r.deg = 0;
    return r;
  }
  r.bad = false;
  r.len = r.deg < (int64_t)fanout ? (int)r.deg : fanout;
  return r;
}

// The row routine, sequential: the ascending positions of row v (deg > fanout) into pos[0..fanout).
// Each pick is inserted where it belongs, so `pos` is the set and the sorted output at once.
OFX_HD void sample_positions(uint64_t v, uint32_t deg, int fanout, uint64_t seed, uint32_t* pos) {
  for (int t = 0; t < fanout; ++t) {
    const uint32_t j = deg - (uint32_t)fanout + (uint32_t)t;
    const uint32_t r = draw(v, (uint32_t)t, seed, j);
    bool taken = false;
    for (int s = 0; s < t; ++s) taken = taken || pos[s] == r;
    const uint32_t pick = floyd_pick(r, j, taken);
    int at = t;
    while (at > 0 && pos[at - 1] > pick) {
      pos[at] = pos[at - 1];
      --at;
    }
    pos[at] = pick;
  }
}

// The checks every entry shares (host).
static inline int check_sample_args(const char* fn, int idx_dtype, int64_t m, int64_t num_seeds,
                                    const void* row_ptr, const void* col_idx, const void* seeds,
                                    int fanout, const void* out_row_ptr, const void* out_col_idx,
                                    const void* out_nnz) {
  OFX_REQUIRE(is_index_dtype(idx_dtype), OFX_EUNSUPPORTED, "%s: index dtype %d is not int32/int64",
              fn, idx_dtype);
  OFX_REQUIRE(fanout >= 1 && fanout <= kMaxFanout, OFX_EINVAL, "%s: fanout %d outside [1, %d]", fn,
              fanout, kMaxFanout);
  OFX_REQUIRE(m >= 0 && num_seeds >= 0, OFX_EINVAL, "%s: negative size (m=%lld num_seeds=%lld)", fn,
              (long long)m, (long long)num_seeds);
  OFX_REQUIRE(idx_dtype == OFX_DT_INT64 ||
                  (m <= INT32_MAX && num_seeds <= INT32_MAX / (int64_t)fanout),
              OFX_EINVAL, "%s: int32 indices cannot address m=%lld or %lld seeds of fanout %d", fn,
              (long long)m, (long long)num_seeds, fanout);
  OFX_REQUIRE(row_ptr && out_row_ptr && out_nnz, OFX_EINVAL, "%s: NULL pointer", fn);
  OFX_REQUIRE(num_seeds == 0 || (seeds && col_idx && out_col_idx), OFX_EINVAL, "%s: NULL pointer",
              fn);
  return OFX_OK;
}

}  // namespace smp
}  // namespace ofx

#endif  // OFX_SAMPLE_NEIGHBORS_H_

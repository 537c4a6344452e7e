// segment_matmul.h — what the HIP kernels (segment_matmul.hip, segment_matmul_grad_w.hip) and the
// kCPU kernels (segment_matmul_cpu.cpp) of ops "segment_matmul" / "segment_matmul_grad_w" share:
// the tile sizes, the w-gradient's partition of the rows, the clamp of a segment bound and the
// argument checks of their C-ABI entries (contract in include/ofx_spmm.h).
#ifndef OFX_SEGMENT_MATMUL_H_
#define OFX_SEGMENT_MATMUL_H_

#include <climits>
#include <cstdint>

#include "gatv2_scores.h"     // extent
#include "graph_attention.h"  // ranges_overlap
#include "ofx_internal.h"
#include "spmm_common.h"

namespace ofx {
namespace segmm {

// The forward's block: kBM output rows x kBN output columns, four waves of 32 rows each.  The
// w-gradient's block: a kBN x kBN tile of dw[t], four waves of 64 x 64 each.  Both walk the
// contraction in slabs of kSlabBytes bytes of the dtype (BK = 64 elements of bf16 / f16, 32 of
// f32): one slab row is what a lane pair of an MFMA operand holds (2 x 64 bytes).
constexpr int kBM = 128;
constexpr int kBN = 128;
constexpr int kSlabBytes = 128;
constexpr int kThreads = 256;
constexpr int slab_elems(int elem_size) { return kSlabBytes / elem_size; }

// The most row parts a w-gradient launch is cut into when the caller leaves the choice open: about
// four blocks a compute unit of the 256 of an MI355X over all tiles of dw[t].
constexpr int64_t kAutoBlocks = 1024;
constexpr int64_t kMaxParts = 4096;

OFX_HD int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// The w-gradient's row parts: `parts` > 0 is the caller's (tests), else a function of the shapes
// alone, at least 256 rows a part.
OFX_HD int64_t grad_w_parts(int64_t s, int64_t f_in, int64_t f_out, int64_t parts) {
  if (parts > 0) return parts < kMaxParts ? parts : kMaxParts;
  const int64_t tiles = ceil_div(f_in, kBN) * ceil_div(f_out, kBN);
  int64_t cap = kAutoBlocks / (tiles > 0 ? tiles : 1);
  if (cap < 1) cap = 1;
  int64_t p = ceil_div(s, 256);
  if (p > cap) p = cap;
  return p < 1 ? 1 : p;
}
// Part p of P owns the rows [part_begin(p), part_begin(p + 1)) of [0, s): s / P rows each, the
// first s % P parts one more.
OFX_HD int64_t part_begin(int64_t p, int64_t parts, int64_t s) {
  const int64_t q = s / parts, rem = s % parts;
  return p * q + (p < rem ? p : rem);
}

// A segment bound as the device kernels use it: clamped into [0, s], so that a malformed seg_ptr
// never gives an address outside the operands.
template <typename I>
OFX_HD int64_t bound(const I* seg_ptr, int64_t t, int64_t s) {
  const int64_t v = (int64_t)seg_ptr[t];
  return v < 0 ? 0 : (v > s ? s : v);
}

// The first segment of [0, t_count) that ends after row `i` (t_count when none does): where a
// tile's or a part's walk over the segments begins.  A binary search over the clamped bounds.
template <typename I>
OFX_HD int64_t first_segment_after(const I* seg_ptr, int64_t t_count, int64_t s, int64_t i) {
  int64_t lo = 0, hi = t_count;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (bound(seg_ptr, mid + 1, s) > i)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

struct Args {
  int idx_dtype, val_dtype;
  int64_t r, s, t, f_in, f_out;  // x [r, .], s output rows, t segments, w[t] logically [f_in, f_out]
  const void* x;
  int64_t ldx;
  const void* seg_ptr;
  const void* idx;  // [s] or NULL (then s == r)
};

// What every entry checks first (all a workspace query checks).
static inline int check_sizes(const char* fn, int idx_dtype, int val_dtype, int64_t r, int64_t s,
                              int64_t t, int64_t f_in, int64_t f_out) {
  OFX_REQUIRE(is_index_dtype(idx_dtype), OFX_EUNSUPPORTED, "%s: index dtype %d is not int32/int64",
              fn, idx_dtype);
  OFX_REQUIRE(val_dtype == OFX_DT_FLOAT || val_dtype == OFX_DT_FLOAT16 ||
                  val_dtype == OFX_DT_BFLOAT16,
              OFX_EUNSUPPORTED, "%s: value dtype %d is not float/float16/bfloat16 (float64 is not "
              "supported)", fn, val_dtype);
  OFX_REQUIRE(r >= 0 && s >= 0 && t >= 1 && f_in >= 1 && f_out >= 1, OFX_EINVAL,
              "%s: bad size (r=%lld s=%lld t=%lld f_in=%lld f_out=%lld)", fn, (long long)r,
              (long long)s, (long long)t, (long long)f_in, (long long)f_out);
  OFX_REQUIRE(idx_dtype == OFX_DT_INT64 || (r <= INT32_MAX && s <= INT32_MAX && t < INT32_MAX),
              OFX_EINVAL, "%s: int32 indices cannot address r=%lld / s=%lld / t=%lld", fn,
              (long long)r, (long long)s, (long long)t);
  const int64_t big = INT64_MAX / 16;
  OFX_REQUIRE(f_in <= INT32_MAX && f_out <= INT32_MAX && t <= big / f_in / f_out &&
                  (s == 0 || (f_in <= big / s && f_out <= big / s)),
              OFX_EINVAL, "%s: t * f_in * f_out or s * f overflows", fn);
  return OFX_OK;
}

// The operands both entries read: x [r, xcols] with ldx, seg_ptr [t + 1], idx [s] or NULL.
static inline int check_inputs(const char* fn, const Args& a, int64_t xcols) {
  OFX_REQUIRE(a.idx != nullptr || a.s == a.r, OFX_EINVAL,
              "%s: without idx the output has x's rows, got s=%lld and r=%lld", fn, (long long)a.s,
              (long long)a.r);
  OFX_REQUIRE(a.ldx >= xcols, OFX_EINVAL, "%s: ldx=%lld is smaller than x's %lld columns", fn,
              (long long)a.ldx, (long long)xcols);
  OFX_REQUIRE(a.seg_ptr != nullptr && (a.x != nullptr || a.r == 0), OFX_EINVAL,
              "%s: NULL seg_ptr or x", fn);
  return OFX_OK;
}

struct Operand {
  const void* ptr;
  uint64_t bytes;
};
template <int N>
static inline int check_no_alias(const char* fn, const void* out, uint64_t out_bytes,
                                 const Operand (&inputs)[N]) {
  bool alias = false;
  for (const Operand& x : inputs) alias = alias || gat::ranges_overlap(out, out_bytes, x.ptr, x.bytes);
  OFX_REQUIRE(!alias, OFX_EINVAL, "%s: the output overlaps an input", fn);
  return OFX_OK;
}

// The forward: out [s, f_out] with ldo, w [t, f_in, f_out] or, trans_w, [t, f_out, f_in].
static inline int check_forward(const char* fn, const Args& a, const void* w, const void* out,
                                int64_t ldo) {
  if (const int rc = check_sizes(fn, a.idx_dtype, a.val_dtype, a.r, a.s, a.t, a.f_in, a.f_out))
    return rc;
  if (const int rc = check_inputs(fn, a, a.f_in)) return rc;
  OFX_REQUIRE(ldo >= a.f_out, OFX_EINVAL, "%s: ldo=%lld is smaller than f_out=%lld", fn,
              (long long)ldo, (long long)a.f_out);
  OFX_REQUIRE(w != nullptr && (out != nullptr || a.s == 0), OFX_EINVAL, "%s: NULL w or out", fn);
  const uint64_t es = (uint64_t)dtype_size(a.val_dtype), is = (uint64_t)dtype_size(a.idx_dtype);
  const Operand in[] = {{a.x, gv2::extent(a.r, a.ldx, a.f_in, es)},
                        {w, (uint64_t)a.t * (uint64_t)a.f_in * (uint64_t)a.f_out * es},
                        {a.seg_ptr, (uint64_t)(a.t + 1) * is},
                        {a.idx, (uint64_t)a.s * is}};
  return check_no_alias(fn, out, gv2::extent(a.s, ldo, a.f_out, es), in);
}

// The w-gradient: dy [s, f_out] with lddy, dw [t, f_in, f_out] contiguous.
static inline int check_grad_w(const char* fn, const Args& a, const void* dy, int64_t lddy,
                               const void* dw, int64_t parts) {
  if (const int rc = check_sizes(fn, a.idx_dtype, a.val_dtype, a.r, a.s, a.t, a.f_in, a.f_out))
    return rc;
  if (const int rc = check_inputs(fn, a, a.f_in)) return rc;
  OFX_REQUIRE(parts >= 0, OFX_EINVAL, "%s: parts=%lld is negative", fn, (long long)parts);
  OFX_REQUIRE(lddy >= a.f_out, OFX_EINVAL, "%s: lddy=%lld is smaller than f_out=%lld", fn,
              (long long)lddy, (long long)a.f_out);
  OFX_REQUIRE(dw != nullptr && (dy != nullptr || a.s == 0), OFX_EINVAL, "%s: NULL dw or dy", fn);
  const uint64_t es = (uint64_t)dtype_size(a.val_dtype), is = (uint64_t)dtype_size(a.idx_dtype);
  const Operand in[] = {{a.x, gv2::extent(a.r, a.ldx, a.f_in, es)},
                        {dy, gv2::extent(a.s, lddy, a.f_out, es)},
                        {a.seg_ptr, (uint64_t)(a.t + 1) * is},
                        {a.idx, (uint64_t)a.s * is}};
  return check_no_alias(fn, dw, (uint64_t)a.t * (uint64_t)a.f_in * (uint64_t)a.f_out * es, in);
}

}  // namespace segmm
}  // namespace ofx

#endif  // OFX_SEGMENT_MATMUL_H_

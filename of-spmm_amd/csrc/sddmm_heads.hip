// sddmm_heads.hip — the multi-head SDDMM over a CSR pattern (op "sddmm_csr_heads"), gfx950:
//   out[j, h] = <a[row(j), h*D:(h+1)*D], b[col[j], h*D:(h+1)*D]>
// for H heads of width D (out is [nnz, H] row-major): the scores of multi-head graph attention
// and d(values) of spmm_csr_heads.  Contract (include/ofx_spmm.h): ofx_sddmm_csr's
// order WITHIN the head -- products rounded, leaves of 8 consecutive columns of the head summed
// sequentially from +0, the head's leaves zero-padded to a power of two and added pairwise, one
// rounding to T.  Leaves never straddle heads.
//
// Work items as the narrow SDDMM's (spmm_backward.hip): a lane group per row or hub chunk of the
// shared planner's work list (skip_empty; the cut has no numeric effect), the `a` row in registers
// for the whole item, B rows streamed U nonzeros in flight.
//   Fast path (D % 8 == 0, D / 8 a power of two, H*D <= 2048, 16-byte-aligned rows): the group
//   covers all H*D columns, lane t owning the L leaves [t*L, (t+1)*L); the B row is read once with
//   16-byte loads.  A head is D/8 consecutive leaves: the pairwise tree runs in the lane over the
//   head's leaves it holds, then as an xor butterfly restricted to the head's lanes (a segmented
//   butterfly).  The first lane of each head stores its result: the H results of a nonzero are
//   contiguous.
//   General path (any other (H, D) with D <= 2048, or unaligned rows): a lane group per (item,
//   head) with column base h*D and output stride H, scalar loads; the head's leaves are the
//   group's, so the butterfly is the whole group's and the bits are the same by construction.
// No atomics, no allocation, no host synchronisation.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "heads_steps.h"
#include "spmm_extremum.h"
#include "spmm_items_dev.h"

namespace ofx {
namespace {

using namespace item;

using namespace hsteps;  // the item's scores, the layout ladder and the schedule (heads_steps.h)

// FAST: the group covers the n = H*D columns of an item, a head is `lh` = D/8 leaves (a power of
// two).  !FAST: group index = item * H + head; the group covers the head's D columns.
template <typename T, typename I, int LG, int L, int U, bool FAST>
__global__ void __launch_bounds__(kBlock)
    sddmm_heads_kernel(const I* __restrict__ rp, const I* __restrict__ col,
                       const T* __restrict__ a, int64_t lda, const T* __restrict__ B, int64_t ldb,
                       int64_t kb, T* __restrict__ out, int64_t row_begin, int64_t nrows,
                       int64_t heads, int64_t d, int lh, int64_t chunk,
                       const unsigned long long* __restrict__ counters,
                       const int64_t* __restrict__ items, const int64_t* __restrict__ order,
                       int64_t block_base, unsigned* err) {
#pragma clang fp contract(off)
  constexpr int GPW = 64 / LG;
  if (poison_head_nonzeros(counters, block_base, err, rp, row_begin, nrows, heads, out)) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gl = lane & (LG - 1);
  const int gbase = lane & ~(LG - 1);
  const int64_t g = ((block_base + (int64_t)blockIdx.x) * (kBlock / 64) + wave) * GPW + lane / LG;
  const int64_t gi = FAST ? g : g / heads;
  const int64_t head = FAST ? 0 : g - gi * heads;
  Item it;
  if (!work_item<I>(rp, gi, row_begin, nrows, chunk, counters, items, order, &it, true)) return;
  sddmm_heads_item<T, I, LG, L, U, FAST>(col, a + it.lr * lda, B, ldb, kb, out, heads, d, lh, head,
                                         it.j0, it.j1, gl, gbase);
}

struct SdHeadsArgs {
  hipStream_t s;
  const void *rp, *col, *a, *b;
  void* out;
  int64_t lda, ldb, row_begin, nrows, heads, d, nnz, k;
  void* ws;
  size_t ws_bytes;
};

template <typename T, typename I, int LG, int L, bool FAST>
int sd_heads_cfg(const SdHeadsArgs& x) {
  constexpr int U = L >= 4 ? 2 : 4;
  const int lh = FAST ? (int)(x.d / kLeaf) : 0;
  Planned p;
  if (const int rc = prepare_plan<I>("sddmm_csr_heads", x.s, static_cast<const I*>(x.rp),
                                     x.row_begin, x.nrows, x.nnz, x.nnz, 0, 0,
                                     scores_schedule(), false, x.ws, x.ws_bytes, &p))
    return rc;
  const int64_t groups = FAST ? p.work : p.work * x.heads;
  return launch_cut_grid(groups, (kBlock / 64) * (64 / LG), [&](dim3 grid, int64_t b0) {
    hipLaunchKernelGGL((sddmm_heads_kernel<T, I, LG, L, U, FAST>), grid, dim3(kBlock), 0, x.s,
                       static_cast<const I*>(x.rp), static_cast<const I*>(x.col),
                       static_cast<const T*>(x.a), x.lda, static_cast<const T*>(x.b), x.ldb, x.k,
                       static_cast<T*>(x.out), x.row_begin, x.nrows, x.heads, x.d, lh, p.chunk,
                       p.wl.counters, p.wl.items, p.wl.order, b0, p.err);
  });
}

template <typename T, typename I>
int sd_heads_typed(const SdHeadsArgs& x) {
  const bool fast = fast_score_shape(x.heads, x.d, x.k) &&
                    rows_aligned(x.a, x.lda, sizeof(T), kLeaf) &&
                    rows_aligned(x.b, x.ldb, sizeof(T), kLeaf);
  return by_score_layout(fast, x.heads, x.d, [&](auto lg, auto l, auto f) -> int {
    return sd_heads_cfg<T, I, decltype(lg)::value, decltype(l)::value, decltype(f)::value>(x);
  });
}

int check_sd_heads_args(const char* fn, int idx_dtype, int val_dtype, int64_t m, int64_t k,
                        int64_t heads, int64_t d, int64_t nnz) {
  if (const int rc = check_heads_shape(fn, heads, d)) return rc;
  return check_types_sizes(fn, idx_dtype, val_dtype, m, k, heads * d, nnz);
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_sddmm_csr_heads_workspace_size(int idx_dtype, int val_dtype, int64_t m,
                                                  int64_t heads, int64_t d, int64_t nnz,
                                                  size_t* bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(bytes != nullptr, OFX_EINVAL, "sddmm_csr_heads_workspace_size: bytes is NULL");
    if (const int rc = check_sd_heads_args("sddmm_csr_heads_workspace_size", idx_dtype, val_dtype,
                                           m, 0, heads, d, nnz))
      return rc;
    *bytes = plan::ws_layout(m, nnz, 0, 0, scores_schedule()).total;
    return OFX_OK;
  });
}

extern "C" int ofx_sddmm_csr_heads(void* stream, int idx_dtype, int val_dtype, int64_t m, int64_t k,
                                   int64_t heads, int64_t d, int64_t nnz, const void* row_ptr,
                                   const void* col_idx, const void* a, int64_t lda, const void* b,
                                   int64_t ldb, void* out, int64_t row_begin, int64_t row_end,
                                   void* workspace, size_t workspace_bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_TAKE_DEVICE_ERROR("sddmm_csr_heads");  // an earlier launch's loud failure (spmm_plan.h)
    int rc = check_sd_heads_args("sddmm_csr_heads", idx_dtype, val_dtype, m, k, heads, d, nnz);
    if (rc) return rc;
    if ((rc = check_row_range("sddmm_csr_heads", row_begin, row_end, m))) return rc;
    const int64_t n = heads * d;
    OFX_REQUIRE(lda >= n && ldb >= n, OFX_EINVAL, "sddmm_csr_heads: lda=%lld / ldb=%lld < n=%lld",
                (long long)lda, (long long)ldb, (long long)n);
    if (row_end == row_begin || nnz == 0 || heads == 0) return OFX_OK;
    OFX_REQUIRE(d > 0, OFX_EINVAL, "sddmm_csr_heads: d == 0 (use a zero fill)");
    OFX_REQUIRE(d <= kMaxHeadsN, OFX_EUNSUPPORTED,
                "sddmm_csr_heads: d=%lld > %lld is not supported", (long long)d,
                (long long)kMaxHeadsN);
    OFX_REQUIRE(row_ptr && col_idx && out && a && b, OFX_EINVAL, "sddmm_csr_heads: NULL pointer");
    const size_t need = plan::ws_layout(row_end - row_begin, nnz, 0, 0, scores_schedule()).total;
    if ((rc = check_workspace("sddmm_csr_heads", workspace, workspace_bytes, need))) return rc;
    const SdHeadsArgs x{static_cast<hipStream_t>(stream), row_ptr, col_idx, a, b, out, lda, ldb,
                        row_begin, row_end - row_begin, heads, d, nnz, k, workspace,
                        workspace_bytes};
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      return sd_heads_typed<std::remove_pointer_t<decltype(tp)>,
                            std::remove_pointer_t<decltype(ip)>>(x);
    });
  });
}

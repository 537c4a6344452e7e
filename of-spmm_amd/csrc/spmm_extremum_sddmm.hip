// spmm_extremum_sddmm.hip — d(values) of the max / min reductions of op "spmm_csr_reduce",
// gfx950: the masked SDDMM.
//
//   d(values)[j] = sum over columns c of (arg[r, c] == j ? g[r, c] * b[col[j], c] : +0),
//                  r the row of nonzero j,
// in the order contract of ofx_sddmm_csr (spmm_backward.hip): 8-element leaves summed
// sequentially from +0, the leaves (zero-padded to a power of two) added pairwise, fp32
// accumulation for 16-bit types, one rounding to T.  A column the nonzero did not win
// contributes +0 whatever b holds (an inf or NaN there does not leak into the gradient).  Padding
// the leaves to a larger power of two adds +0 to sums that are never -0, so the lane-group widths
// below (a subset of the SDDMM's) give the same bits.
//
// Kernel structure of the SDDMM: a lane-group of LG lanes per work item (a row or a chunk of a
// long row from the shared planner; the results do not depend on the cut), lane t owning the L
// leaves [t * L, (t + 1) * L): it keeps its part of g[r, :] and arg[r, :] in registers for the whole
// item and streams B[col] rows, U in flight.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <climits>

#include "spmm_extremum_dev.h"

namespace ofx {
namespace {

using namespace xt;

constexpr int kLeaf = 8;
constexpr int64_t kSelChunk = 256;         // items of at most this many nonzeros (work layout only)
constexpr int64_t kMaxSelN = 256 * kLeaf;  // 64 lanes x 4 leaves

// The SDDMM's own work layout (spmm_backward.hip sddmm_schedule), so that the workspace query of
// ofx_sddmm_csr serves this launch too.
Schedule sel_schedule(int64_t n) {
  Schedule s = resolve_schedule(n, nullptr);
  s.split = s.chunk = kSelChunk;
  return s;
}

template <typename T, typename I, int LG, int L, int U, bool ALIGNED>
__global__ void __launch_bounds__(kBlock)
    sddmm_select_kernel(const I* __restrict__ rp, const I* __restrict__ col,
                        const I* __restrict__ arg, int64_t ldarg, const T* __restrict__ dC,
                        int64_t ldc, const T* __restrict__ B, int64_t ldb, int64_t kb,
                        T* __restrict__ out, int64_t row_begin, int64_t nrows, int64_t n,
                        int64_t chunk, const unsigned long long* __restrict__ counters,
                        const int64_t* __restrict__ items, const int64_t* __restrict__ order,
                        int64_t block_base, unsigned* err) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  constexpr int GPW = 64 / LG;
  if (counters != nullptr && !plan::plan_valid(counters)) {
    // no valid plan: the nonzeros of the launch's rows become the canonical NaN (as ofx_sddmm_csr)
    if (block_base + blockIdx.x == 0 && threadIdx.x == 0)
      plan::raise_device_error(err, plan::kErrPlanInvalid);
    const int64_t j0 = (int64_t)rp[row_begin], j1 = (int64_t)rp[row_begin + nrows];
    const T p = poison_value<T>();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = j0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < j1; j += stride)
      out[j] = p;
    return;
  }
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gl = lane & (LG - 1);
  const int gbase = lane & ~(LG - 1);
  const int64_t g = ((block_base + (int64_t)blockIdx.x) * (kBlock / 64) + wave) * GPW + lane / LG;
  Item it;
  if (!work_item<I>(rp, g, row_begin, nrows, chunk, counters, items, order, &it)) return;
  if (it.j0 >= it.j1) return;
  const T zero = Num<T>::store(A(0));
  // this lane's leaves of the upstream gradient and of arg, kept for the whole item
  T a[L][kLeaf];
  I w[L][kLeaf];
#pragma unroll
  for (int l = 0; l < L; ++l) {
    const int64_t cb = (int64_t)(gl * L + l) * kLeaf;
    load_cols<T, kLeaf, ALIGNED>(dC + it.lr * ldc, cb, n, zero, a[l]);
    load_cols<I, kLeaf, ALIGNED>(arg + it.lr * ldarg, cb, n, I(-1), w[l]);
  }
  for (int64_t jb = it.j0; jb < it.j1; jb += LG) {
    const int cnt = (int)((it.j1 - jb) < LG ? (it.j1 - jb) : LG);
    const I myc = gl < cnt ? col[jb + gl] : I(0);
    A res = A(0);
    for (int k = 0; k < cnt; k += U) {
      T bv[U][L][kLeaf];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t cu = (int64_t)__shfl((int64_t)myc, gbase + ((k + u) & (LG - 1)), 64);
        if (k + u < cnt) {
          const bool in = (uint64_t)cu < (uint64_t)kb;  // else the zero-filled gathered row
#pragma unroll
          for (int l = 0; l < L; ++l)
            load_cols<T, kLeaf, ALIGNED>(B + (in ? cu : 0) * ldb,
                                         in ? (int64_t)(gl * L + l) * kLeaf : n, n, zero, bv[u][l]);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < cnt) {
          const I j = (I)(jb + k + u);
          A leaf[L];
#pragma unroll
          for (int l = 0; l < L; ++l) {
            A s = A(0);
#pragma unroll
            for (int e = 0; e < kLeaf; ++e) {
              const A term = w[l][e] == j ? Num<T>::load(a[l][e]) * Num<T>::load(bv[u][l][e]) : A(0);
              s = s + term;
            }
            leaf[l] = s;
          }
#pragma unroll
          for (int x = 1; x < L; x <<= 1)
#pragma unroll
            for (int l = 0; l < L; l += 2 * x) leaf[l] = leaf[l] + leaf[l + x];
          A t = leaf[0];
#pragma unroll
          for (int x = 1; x < LG; x <<= 1) t = t + __shfl_xor(t, x, 64);
          if (gl == k + u) res = t;
        }
      }
    }
    if (gl < cnt) out[jb + gl] = Num<T>::store(res);
  }
}

struct SdArgs {
  hipStream_t s;
  const void *rp, *col, *arg, *dC, *B;
  void* out;
  int64_t ldarg, ldc, ldb, row_begin, nrows, n, nnz, k;
  void* ws;
  size_t ws_bytes;
};

template <typename T, typename I, int LG, int L, bool ALIGNED>
int sddmm_select_cfg(const SdArgs& a) {
  constexpr int U = L >= 4 ? 2 : 4;
  constexpr int64_t GPB = (kBlock / 64) * (64 / LG);
  const Schedule sched = sel_schedule(a.n);
  const plan::WsLayout w = plan::ws_layout(a.nrows, a.nnz, 0, 0, sched);
  plan::WorkList wl{};
  if (w.total > 0) {
    OFX_REQUIRE(a.ws && a.ws_bytes >= w.total, OFX_EWORKSPACE,
                "sddmm_csr_select: workspace of %zu bytes < %zu required", a.ws_bytes, w.total);
    const int rc = plan::launch_plan<I>(a.s, static_cast<const I*>(a.rp), a.row_begin, a.nrows,
                                        a.nnz, sched, w, static_cast<char*>(a.ws), &wl);
    if (rc) return rc;
  }
  const int64_t work = a.nrows + (w.total > 0 ? w.max_chunks : 0);
  const int64_t grid = (work + GPB - 1) / GPB;
  for (int64_t b0 = 0; b0 < grid; b0 += kLaunchBlocks) {  // < 2^31 threads per launch
    hipLaunchKernelGGL((sddmm_select_kernel<T, I, LG, L, U, ALIGNED>),
                       dim3((unsigned)std::min(kLaunchBlocks, grid - b0)), dim3(kBlock), 0, a.s,
                       static_cast<const I*>(a.rp), static_cast<const I*>(a.col),
                       static_cast<const I*>(a.arg), a.ldarg, static_cast<const T*>(a.dC), a.ldc,
                       static_cast<const T*>(a.B), a.ldb, a.k, static_cast<T*>(a.out), a.row_begin,
                       a.nrows, a.n, w.total > 0 ? sched.chunk : INT64_MAX, wl.counters, wl.items,
                       wl.order, b0, w.total > 0 ? device_error_words() : nullptr);
    OFX_HIP_CHECK(hipGetLastError());
  }
  return OFX_OK;
}

template <typename T, typename I, bool ALIGNED>
int sddmm_select_width(const SdArgs& a) {
  const int64_t leaves = (a.n + kLeaf - 1) / kLeaf;
  if (leaves <= 1) return sddmm_select_cfg<T, I, 1, 1, ALIGNED>(a);
  if (leaves <= 4) return sddmm_select_cfg<T, I, 4, 1, ALIGNED>(a);
  if (leaves <= 16) return sddmm_select_cfg<T, I, 16, 1, ALIGNED>(a);
  if (leaves <= 64) return sddmm_select_cfg<T, I, 64, 1, ALIGNED>(a);
  return sddmm_select_cfg<T, I, 64, 4, ALIGNED>(a);
}

template <typename T, typename I>
int sddmm_select_typed(const SdArgs& a) {
  const bool aligned = a.n % kLeaf == 0 && rows_aligned(a.dC, a.ldc, sizeof(T), kLeaf) &&
                       rows_aligned(a.B, a.ldb, sizeof(T), kLeaf) &&
                       rows_aligned(a.arg, a.ldarg, sizeof(I), kLeaf);
  return aligned ? sddmm_select_width<T, I, true>(a) : sddmm_select_width<T, I, false>(a);
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_sddmm_csr_select(void* stream, int idx_dtype, int val_dtype, int64_t m, int64_t k,
                                    int64_t n, int64_t nnz, const void* row_ptr,
                                    const void* col_idx, const void* arg, int64_t ldarg,
                                    const void* a, int64_t lda, const void* b, int64_t ldb,
                                    void* out, int64_t row_begin, int64_t row_end, void* workspace,
                                    size_t workspace_bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_TAKE_DEVICE_ERROR("sddmm_csr_select");  // an earlier launch's loud failure (spmm_plan.h)
    int rc = check_sddmm_select_args("sddmm_csr_select", idx_dtype, val_dtype, m, k, n, nnz, ldarg,
                                     lda, ldb, row_begin, row_end);
    if (rc) return rc;
    if (row_end == row_begin || nnz == 0) return OFX_OK;
    OFX_REQUIRE(n <= kMaxSelN, OFX_EUNSUPPORTED, "sddmm_csr_select: n=%lld > %lld is not supported",
                (long long)n, (long long)kMaxSelN);
    OFX_REQUIRE(arg != nullptr, OFX_EINVAL,
                "sddmm_csr_select: arg is NULL (the gradient of max / min needs it)");
    OFX_REQUIRE(row_ptr && col_idx && out && a && b, OFX_EINVAL, "sddmm_csr_select: NULL pointer");
    const SdArgs args{static_cast<hipStream_t>(stream), row_ptr, col_idx, arg, a, b, out, ldarg,
                      lda, ldb, row_begin, row_end - row_begin, n, nnz, k, workspace,
                      workspace_bytes};
    return xt::by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      return sddmm_select_typed<std::remove_pointer_t<decltype(tp)>,
                                std::remove_pointer_t<decltype(ip)>>(args);
    });
  });
}

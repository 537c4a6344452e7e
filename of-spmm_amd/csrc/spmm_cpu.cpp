// spmm_cpu.cpp — the DeviceType::kCPU kernels of ops "spmm_csr" and "fused_spmm_csr" (SURVEY.md §8
// row a2) and of their gradients: the SDDMM ("sddmm_csr", and its masked form for max / min) and
// the fused epilogue's backward.  The host utilities of the CSR itself are in csr_host_cpu.cpp.
//
// Row-parallel over OpenMP in the idiom of CpuStream::ParallelFor
// (oneflow/core/ep/cpu/cpu_stream.h:104-145): rows are independent, each row is reduced by
// one thread in the contract order of spmm_common.h (gather -> multiply -> segment-sum,
// oneflow/user/kernels/gather_kernel_util.cpp:72-92 + unsorted_segment_sum_kernel_util.cpp:29-45),
// including the same hub-row chunking as the HIP kernel, so CPU and GPU produce identical bits.
// The row loops are the one-head case of spmm_rows_cpu.h.
// Thread count: OMP_NUM_THREADS like oneflow/core/job/env_global_objects_scope.cpp:90-99.
#pragma clang fp contract(off)

#include <omp.h>

#include <vector>

#include "ofx_internal.h"
#include "spmm_common.h"
#include "spmm_extremum.h"
#include "spmm_rows_cpu.h"

using namespace ofx;

namespace {

int spmm_cpu_entry(int num_threads, int idx_dtype, int val_dtype, int64_t m, int64_t k, int64_t n,
                   int64_t nnz, const void* row_ptr, const void* col_idx, const void* values,
                   const void* b, int64_t ldb, void* c, int64_t ldc, int64_t row_begin,
                   int64_t row_end, const void* bias, int act, const ofx_spmm_options* opts) {
  OFX_READ_OPTIONS(opts, "spmm_csr_cpu");
  if (const int rc = check_types_sizes("spmm_csr_cpu", idx_dtype, val_dtype, m, k, n, nnz)) return rc;
  if (const int rc = check_row_range("spmm_csr_cpu", row_begin, row_end, m)) return rc;
  OFX_REQUIRE(ldb >= n && ldc >= n, OFX_EINVAL, "spmm_csr_cpu: ldb/ldc < n");
  OFX_REQUIRE(act == OFX_ACT_NONE || act == OFX_ACT_RELU, OFX_EINVAL,
              "spmm_csr_cpu: unknown activation %d", act);
  if (row_end == row_begin || n == 0) return OFX_OK;
  OFX_REQUIRE(row_ptr && c && (nnz == 0 || (col_idx && values && b)), OFX_EINVAL,
              "spmm_csr_cpu: NULL pointer");
  const Schedule s = resolve_schedule(n, opts);
  return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
    using T = std::remove_pointer_t<decltype(tp)>;
    using I = std::remove_pointer_t<decltype(ip)>;
    return cpu_spmm_rows<T, I>("spmm_csr_cpu", threads_of(num_threads), k, 1, n, (const I*)row_ptr,
                               (const I*)col_idx, (const T*)values, (const T*)b, ldb, (T*)c, ldc,
                               row_begin, row_end, s, (const T*)bias, act);
  });
}

// Either SDDMM over rows [row_begin, row_end), its arguments checked by the entry.  A negative
// column is refused before anything is written.
template <bool MASKED>
int run_sddmm(const char* fn, int num_threads, int idx_dtype, int val_dtype, int64_t k, int64_t n,
              const void* row_ptr, const void* col_idx, const void* arg, int64_t ldarg,
              const void* a, int64_t lda, const void* b, int64_t ldb, void* out, int64_t row_begin,
              int64_t row_end) {
  return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
    using T = std::remove_pointer_t<decltype(tp)>;
    using I = std::remove_pointer_t<decltype(ip)>;
    const I* rp = (const I*)row_ptr;
    OFX_REQUIRE(!negative_column((const I*)col_idx, (int64_t)rp[row_begin], (int64_t)rp[row_end]),
                OFX_EINVAL, "%s: negative column index (gather_kernel_util.cpp:80 CHECK_GE(idx, 0))",
                fn);
    cpu_sddmm_rows<T, I, MASKED>(threads_of(num_threads), k, 1, n, rp, (const I*)col_idx,
                                 (const I*)arg, ldarg, (const T*)a, lda, (const T*)b, ldb, (T*)out,
                                 row_begin, row_end);
    return OFX_OK;
  });
}

}  // namespace

extern "C" int ofx_spmm_csr_cpu(int num_threads, int idx_dtype, int val_dtype, int64_t m,
                                int64_t k, int64_t n, int64_t nnz, const void* row_ptr,
                                const void* col_idx, const void* values, const void* b,
                                int64_t ldb, void* c, int64_t ldc, int64_t row_begin,
                                int64_t row_end, const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    return spmm_cpu_entry(num_threads, idx_dtype, val_dtype, m, k, n, nnz, row_ptr, col_idx, values,
                          b, ldb, c, ldc, row_begin, row_end, nullptr, OFX_ACT_NONE, opts);
  });
}

extern "C" int ofx_spmm_csr_fused_cpu(int num_threads, int idx_dtype, int val_dtype, int64_t m,
                                      int64_t k, int64_t n, int64_t nnz, const void* row_ptr,
                                      const void* col_idx, const void* values, const void* b,
                                      int64_t ldb, void* c, int64_t ldc, int64_t row_begin,
                                      int64_t row_end, const void* bias, int activation,
                                      const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    return spmm_cpu_entry(num_threads, idx_dtype, val_dtype, m, k, n, nnz, row_ptr, col_idx, values,
                          b, ldb, c, ldc, row_begin, row_end, bias, activation, opts);
  });
}

// ---- backward on the host (same bits as the HIP kernels) ---------------------------------------
extern "C" int ofx_sddmm_csr_cpu(int num_threads, int idx_dtype, int val_dtype, int64_t m,
                                 int64_t k, int64_t n, int64_t nnz, const void* row_ptr,
                                 const void* col_idx, const void* a, int64_t lda, const void* b,
                                 int64_t ldb, void* out, int64_t row_begin, int64_t row_end) {
  return ::ofx::guarded(__func__, [&]() -> int {
    if (const int rc = check_types_sizes("sddmm_csr_cpu", idx_dtype, val_dtype, m, k, n, nnz))
      return rc;
    if (const int rc = check_row_range("sddmm_csr_cpu", row_begin, row_end, m)) return rc;
    OFX_REQUIRE(n > 0 && lda >= n && ldb >= n, OFX_EINVAL,
                "sddmm_csr_cpu: n=%lld must be > 0 and lda=%lld / ldb=%lld >= n", (long long)n,
                (long long)lda, (long long)ldb);
    if (row_end == row_begin || nnz == 0) return OFX_OK;
    return run_sddmm<false>("sddmm_csr_cpu", num_threads, idx_dtype, val_dtype, k, n, row_ptr,
                            col_idx, nullptr, 0, a, lda, b, ldb, out, row_begin, row_end);
  });
}

// d(values) of the max / min reductions: the masked SDDMM (csrc/spmm_extremum_cpu.cpp has the
// other kCPU kernels of op "spmm_csr_reduce").
extern "C" int ofx_sddmm_csr_select_cpu(int num_threads, int idx_dtype, int val_dtype, int64_t m,
                                        int64_t k, int64_t n, int64_t nnz, const void* row_ptr,
                                        const void* col_idx, const void* arg, int64_t ldarg,
                                        const void* a, int64_t lda, const void* b, int64_t ldb,
                                        void* out, int64_t row_begin, int64_t row_end) {
  return ::ofx::guarded(__func__, [&]() -> int {
    int rc = check_sddmm_select_args("sddmm_csr_select_cpu", idx_dtype, val_dtype, m, k, n, nnz,
                                     ldarg, lda, ldb, row_begin, row_end);
    if (rc) return rc;
    if (row_end == row_begin || nnz == 0) return OFX_OK;
    OFX_REQUIRE(arg != nullptr, OFX_EINVAL,
                "sddmm_csr_select_cpu: arg is NULL (the gradient of max / min needs it)");
    OFX_REQUIRE(row_ptr && col_idx && out && a && b, OFX_EINVAL,
                "sddmm_csr_select_cpu: NULL pointer");
    return run_sddmm<true>("sddmm_csr_select_cpu", num_threads, idx_dtype, val_dtype, k, n, row_ptr,
                           col_idx, arg, ldarg, a, lda, b, ldb, out, row_begin, row_end);
  });
}

// ---- fused-epilogue backward on the host (csrc/epilogue_grad.hip states the order) -----------
namespace {

constexpr int64_t kGradRows = 2048;  // same chunking as the HIP kernel
constexpr int kGradLanes = 8;

// The chunks are fixed rows, so the bits do not depend on the thread count.
template <typename T>
int relu_bias_grad_cpu(int nthreads, int64_t m, int64_t n, const T* y, int64_t ldy, const T* dy,
                       int64_t lddy, T* dx, int64_t lddx, T* d_bias, int relu) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  const int64_t nch = (m + kGradRows - 1) / kGradRows;
  std::vector<A> part(d_bias ? (size_t)nch * (size_t)n : 0);
#pragma omp parallel for num_threads(nthreads) schedule(static)
  for (int64_t c = 0; c < nch; ++c) {
    const int64_t r1 = (c + 1) * kGradRows < m ? (c + 1) * kGradRows : m;
    for (int64_t j = 0; j < n; ++j) {
      A acc = A(0);
      for (int64_t r = c * kGradRows; r < r1; ++r) {
        const A g = (relu && !(Num<T>::load(y[r * ldy + j]) > A(0))) ? A(0)
                                                                       : Num<T>::load(dy[r * lddy + j]);
        if (dx) dx[r * lddx + j] = Num<T>::store(g);
        acc = acc + g;
      }
      if (d_bias) part[(size_t)c * n + j] = acc;
    }
  }
  if (d_bias) {
    for (int64_t j = 0; j < n; ++j) {
      A lane[kGradLanes];
      for (int l = 0; l < kGradLanes; ++l) {
        A acc = A(0);
        for (int64_t c = l; c < nch; c += kGradLanes) acc = acc + part[(size_t)c * n + j];
        lane[l] = acc;
      }
      for (int s = kGradLanes / 2; s >= 1; s >>= 1)
        for (int l = 0; l < s; ++l) lane[l] = lane[l] + lane[l + s];
      d_bias[j] = Num<T>::store(lane[0]);
    }
  }
  return OFX_OK;
}

}  // namespace

extern "C" int ofx_relu_bias_grad_cpu(int num_threads, int val_dtype, int64_t m, int64_t n,
                                      const void* y, int64_t ldy, const void* dy, int64_t lddy,
                                      void* dx, int64_t lddx, void* d_bias, int relu) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(is_value_dtype(val_dtype), OFX_EUNSUPPORTED, "relu_bias_grad: bad dtype %d",
                val_dtype);
    OFX_REQUIRE(m >= 0 && n >= 0, OFX_EINVAL, "relu_bias_grad: negative size");
    if (n == 0) return OFX_OK;
    OFX_REQUIRE(m == 0 || (dy && (!relu || y) && lddy >= n && (!relu || ldy >= n)), OFX_EINVAL,
                "relu_bias_grad: NULL input or leading dimension < n");
    OFX_REQUIRE(dx == nullptr || lddx >= n, OFX_EINVAL, "relu_bias_grad: lddx < n");
    return by_value(val_dtype, [&](auto* tp) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      return relu_bias_grad_cpu<T>(threads_of(num_threads), m, n, (const T*)y, ldy, (const T*)dy,
                                   lddy, (T*)dx, lddx, (T*)d_bias, relu);
    });
  });
}

// spmm_extremum_cpu.cpp — the DeviceType::kCPU kernels of the max / min / mean reductions of
// op "spmm_csr_reduce" and of their gradients (contracts in include/ofx_spmm.h, shared helpers in
// spmm_extremum.h).  Row-parallel over OpenMP like spmm_cpu.cpp; the same bits as the HIP kernels
// (spmm_extremum.hip, spmm_extremum_grad.hip).  d(values), the masked SDDMM, is beside the plain
// SDDMM in spmm_cpu.cpp.
#pragma clang fp contract(off)

#include <omp.h>

#include <climits>
#include <type_traits>
#include <vector>

#include "ofx_internal.h"
#include "spmm_common.h"
#include "spmm_extremum.h"

namespace ofx {
namespace {

// out[r, :] = extremum over the row's products in ascending j (spmm_extremum.h `better`); the
// walk is the contract itself, so chunking a row cannot change it and the schedule is not read.
template <typename T, typename I>
int cpu_extremum(int nthreads, int64_t k, int64_t n, const I* rp, const I* col, const T* val,
                 const T* B, int64_t ldb, T* C, int64_t ldc, I* arg, int64_t ldarg,
                 int64_t row_begin, int64_t row_end, bool is_max) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  bool any_neg = false;
#pragma omp parallel num_threads(nthreads) reduction(|| : any_neg)
  {
    std::vector<A> best(n);
    std::vector<int64_t> barg(n);
    bool neg = false;
#pragma omp for schedule(dynamic, 64)
    for (int64_t r = row_begin; r < row_end; ++r) {
      for (int64_t c = 0; c < n; ++c) {
        best[c] = A(0);
        barg[c] = -1;
      }
      for (int64_t j = (int64_t)rp[r]; j < (int64_t)rp[r + 1]; ++j) {
        const A v = Num<T>::load(val[j]);
        const int64_t cj = (int64_t)col[j];
        const bool in = cj >= 0 && cj < k;  // else the zero-filled gathered row
        if (cj < 0) neg = true;
        const T* brow = in ? B + cj * ldb : nullptr;
        for (int64_t c = 0; c < n; ++c) {
          const A p = Num<T>::mul(v, in ? Num<T>::load(brow[c]) : A(0));
          const bool take = (int(barg[c] < 0) | int(better(p, best[c], is_max))) != 0;
          best[c] = take ? p : best[c];
          barg[c] = take ? j : barg[c];
        }
      }
      T* out = C + (r - row_begin) * ldc;
      for (int64_t c = 0; c < n; ++c) out[c] = Num<T>::store(canonical_nan(best[c]));
      if (arg != nullptr) {
        I* ao = arg + (r - row_begin) * ldarg;
        for (int64_t c = 0; c < n; ++c) ao[c] = (I)barg[c];
      }
    }
    any_neg = any_neg || neg;
  }
  OFX_REQUIRE(!any_neg, OFX_EINVAL,
              "spmm_csr_reduce_cpu: negative column index (gather_kernel_util.cpp:80 "
              "CHECK_GE(idx, 0))");
  return OFX_OK;
}

// d(b) of max / min: row kk of A^T in the sum op's order and hub-chunk schedule, adding only the
// entries that won their (row, column).
template <typename T, typename I>
void select_row(const I* col_t, const I* perm, const T* val, const I* arg, int64_t ldarg,
                const T* g, int64_t ldg, int64_t m, int64_t nnz, int64_t n, int64_t t0,
                int64_t t1, typename Num<T>::acc* acc) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  for (int64_t c = 0; c < n; ++c) acc[c] = A(0);
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t j = (int64_t)perm[t], r = (int64_t)col_t[t];
    if ((uint64_t)j >= (uint64_t)nnz || (uint64_t)r >= (uint64_t)m) continue;
    const A v = Num<T>::load(val[j]);
    const I* arow = arg + r * ldarg;
    const T* grow = g + r * ldg;
    for (int64_t c = 0; c < n; ++c)
      if ((int64_t)arow[c] == j) acc[c] = acc[c] + Num<T>::mul(v, Num<T>::load(grow[c]));
  }
}

template <typename T, typename I>
void cpu_select(int nthreads, int64_t m, int64_t nnz, int64_t n, const I* rp_t, const I* col_t,
                const I* perm, const T* val, const I* arg, int64_t ldarg, const T* g, int64_t ldg,
                T* db, int64_t lddb, int64_t row_begin, int64_t row_end, const Schedule& s) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
#pragma omp parallel num_threads(nthreads)
  {
    std::vector<A> acc(n), part(n);
#pragma omp for schedule(dynamic, 64)
    for (int64_t kk = row_begin; kk < row_end; ++kk) {
      const int64_t t0 = (int64_t)rp_t[kk], t1 = (int64_t)rp_t[kk + 1];
      const int64_t len = t1 - t0;
      if (len <= s.split) {
        select_row<T, I>(col_t, perm, val, arg, ldarg, g, ldg, m, nnz, n, t0, t1, acc.data());
      } else {
        const int64_t nc = num_chunks(len, s.chunk);
        for (int64_t c = 0; c < n; ++c) acc[c] = A(0);
        for (int64_t q = 0; q < nc; ++q) {
          const int64_t a = t0 + q * s.chunk;
          const int64_t e = (q == nc - 1) ? t1 : a + s.chunk;
          select_row<T, I>(col_t, perm, val, arg, ldarg, g, ldg, m, nnz, n, a, e, part.data());
          for (int64_t c = 0; c < n; ++c) acc[c] = acc[c] + part[c];
        }
      }
      T* out = db + (kk - row_begin) * lddb;
      for (int64_t c = 0; c < n; ++c) out[c] = Num<T>::store(acc[c]);
    }
  }
}

template <typename T, typename I>
void cpu_row_scale(int nthreads, int64_t n, const I* rp, const T* src, int64_t ldsrc, T* dst,
                   int64_t lddst, int64_t row_begin, int64_t row_end) {
#pragma clang fp contract(off)
#pragma omp parallel for num_threads(nthreads) schedule(static)
  for (int64_t r = row_begin; r < row_end; ++r) {
    const int64_t deg = (int64_t)rp[r + 1] - (int64_t)rp[r];
    const T* s = src + (r - row_begin) * ldsrc;
    T* d = dst + (r - row_begin) * lddst;
    for (int64_t c = 0; c < n; ++c) d[c] = scale_by_degree<T>(s[c], deg);
  }
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_spmm_csr_reduce_cpu(int num_threads, int idx_dtype, int val_dtype, int64_t m,
                                       int64_t k, int64_t n, int64_t nnz, const void* row_ptr,
                                       const void* col_idx, const void* values, const void* b,
                                       int64_t ldb, void* c, int64_t ldc, void* arg, int64_t ldarg,
                                       int64_t row_begin, int64_t row_end, int reduce,
                                       const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    int rc = check_reduce_code(reduce, "spmm_csr_reduce_cpu");
    if (rc) return rc;
    if (reduce == OFX_REDUCE_SUM || reduce == OFX_REDUCE_MEAN) {
      rc = ofx_spmm_csr_cpu(num_threads, idx_dtype, val_dtype, m, k, n, nnz, row_ptr, col_idx,
                            values, b, ldb, c, ldc, row_begin, row_end, opts);
      if (rc || reduce == OFX_REDUCE_SUM) return rc;
      return ofx_row_scale_by_degree_cpu(num_threads, idx_dtype, val_dtype, m, n, row_ptr, c, ldc,
                                         c, ldc, row_begin, row_end);
    }
    OFX_READ_OPTIONS(opts, "spmm_csr_reduce_cpu");  // validated; the schedule has no effect here
    rc = check_reduce_args("spmm_csr_reduce_cpu", idx_dtype, val_dtype, m, k, n, nnz, ldb, ldc,
                           arg != nullptr, ldarg, row_begin, row_end);
    if (rc) return rc;
    if (row_end == row_begin || n == 0) return OFX_OK;
    OFX_REQUIRE(row_ptr && c && (nnz == 0 || (col_idx && values && b)), OFX_EINVAL,
                "spmm_csr_reduce_cpu: NULL pointer");
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      return cpu_extremum<T, I>(threads_of(num_threads), k, n, (const I*)row_ptr,
                                (const I*)col_idx, (const T*)values, (const T*)b, ldb, (T*)c, ldc,
                                (I*)arg, ldarg, row_begin, row_end, reduce == OFX_REDUCE_MAX);
    });
  });
}

extern "C" int ofx_spmm_csr_select_cpu(int num_threads, int idx_dtype, int val_dtype, int64_t m,
                                       int64_t k, int64_t n, int64_t nnz, const void* row_ptr_t,
                                       const void* col_idx_t, const void* perm, const void* values,
                                       const void* arg, int64_t ldarg, const void* g, int64_t ldg,
                                       void* db, int64_t lddb, int64_t row_begin, int64_t row_end,
                                       const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_READ_OPTIONS(opts, "spmm_csr_select_cpu");
    int rc = check_select_args("spmm_csr_select_cpu", idx_dtype, val_dtype, m, k, n, nnz, ldarg,
                               ldg, lddb, row_begin, row_end);
    if (rc) return rc;
    if (row_end == row_begin || n == 0) return OFX_OK;
    OFX_REQUIRE(row_ptr_t && db, OFX_EINVAL, "spmm_csr_select_cpu: NULL row_ptr or output");
    OFX_REQUIRE(nnz == 0 || m == 0 || arg != nullptr, OFX_EINVAL,
                "spmm_csr_select_cpu: arg is NULL (the gradient of max / min needs it)");
    OFX_REQUIRE(nnz == 0 || (col_idx_t && perm && values && g), OFX_EINVAL,
                "spmm_csr_select_cpu: NULL pointer with nnz=%lld", (long long)nnz);
    const Schedule s = resolve_schedule(n, opts);
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      cpu_select<T, I>(threads_of(num_threads), m, nnz, n, (const I*)row_ptr_t,
                       (const I*)col_idx_t, (const I*)perm, (const T*)values, (const I*)arg, ldarg,
                       (const T*)g, ldg, (T*)db, lddb, row_begin, row_end, s);
      return OFX_OK;
    });
  });
}

extern "C" int ofx_row_scale_by_degree_cpu(int num_threads, int idx_dtype, int val_dtype,
                                           int64_t m, int64_t n, const void* row_ptr,
                                           const void* src, int64_t ldsrc, void* dst,
                                           int64_t lddst, int64_t row_begin, int64_t row_end) {
  return ::ofx::guarded(__func__, [&]() -> int {
    int rc = check_row_scale_args("row_scale_by_degree_cpu", idx_dtype, val_dtype, m, n, ldsrc,
                                  lddst, row_begin, row_end);
    if (rc) return rc;
    if (row_end == row_begin || n == 0) return OFX_OK;
    OFX_REQUIRE(row_ptr && src && dst, OFX_EINVAL, "row_scale_by_degree_cpu: NULL pointer");
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      cpu_row_scale<T, I>(threads_of(num_threads), n, (const I*)row_ptr, (const T*)src, ldsrc,
                          (T*)dst, lddst, row_begin, row_end);
      return OFX_OK;
    });
  });
}

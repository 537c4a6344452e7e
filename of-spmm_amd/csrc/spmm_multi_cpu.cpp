// spmm_multi_cpu.cpp — the DeviceType::kCPU kernel of op "spmm_csr_multi" (sum / mean / max / min /
// var / std of every row's messages from one walk; contract in include/ofx_spmm.h).
// The row template of spmm_rows_cpu.h with the statistics of spmm_multi.h in place of the one sum:
// a row of at most s.split nonzeros is one in-order walk, a longer one the in-order merge of its
// chunks' statistics (num_chunks), then the finishing step the HIP kernels take.  The same bits as
// spmm_multi.hip whatever the thread count: a row is one thread's.
#pragma clang fp contract(off)

#include <omp.h>

#include <vector>

#include "ofx_internal.h"
#include "spmm_common.h"
#include "spmm_multi.h"

using namespace ofx;

namespace {

// Nonzeros [j0, j1) fed to st[0 .. n): a column outside [0, k) is the zero-filled gathered row, a
// negative one is reported (`neg`), as row_sum of spmm_rows_cpu.h.
template <typename T, typename I>
void multi_run(const I* col, const T* val, const T* B, int64_t ldb, int64_t k, int64_t n,
               int64_t j0, int64_t j1, multi::Stats<typename Num<T>::acc, int64_t>* st, bool* neg) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  for (int64_t c = 0; c < n; ++c) st[c] = multi::empty_stats<A, int64_t>();
  for (int64_t j = j0; j < j1; ++j) {
    const int64_t cj = (int64_t)col[j];
    const bool in = cj >= 0 && cj < k;
    if (cj < 0) *neg = true;
    const A v = Num<T>::load(val[j]);
    const T* brow = in ? B + cj * ldb : nullptr;
    for (int64_t c = 0; c < n; ++c)
      multi::feed<2, true>(st[c], Num<T>::mul(v, in ? Num<T>::load(brow[c]) : A(0)), j);
  }
}

template <typename T, typename I>
int cpu_multi(int nthreads, int64_t k, int64_t n, const I* rp, const I* col, const T* val,
              const T* B, int64_t ldb, const multi::Outputs<T, I>& o, int64_t row_begin,
              int64_t row_end, const Schedule& s) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  using S = multi::Stats<A, int64_t>;
  const int64_t rows = row_end - row_begin;
  bool any_neg = false;
#pragma omp parallel num_threads(nthreads) reduction(|| : any_neg)
  {
    std::vector<S> acc(n), part(n);
    bool neg = false;
#pragma omp for schedule(dynamic, 64)
    for (int64_t g = 0; g < rows; ++g) {
      const int64_t j0 = (int64_t)rp[row_begin + g], j1 = (int64_t)rp[row_begin + g + 1];
      const int64_t len = j1 - j0;
      if (len <= s.split) {
        multi_run<T, I>(col, val, B, ldb, k, n, j0, j1, acc.data(), &neg);
      } else {
        const int64_t nc = num_chunks(len, s.chunk);
        for (int64_t q = 0; q < nc; ++q) {
          const int64_t a = j0 + q * s.chunk;
          multi_run<T, I>(col, val, B, ldb, k, n, a, q == nc - 1 ? j1 : a + s.chunk, part.data(),
                          &neg);
          for (int64_t c = 0; c < n; ++c) {
            if (q == 0) {  // the moments into +0, the extrema from the first chunk
              acc[c] = part[c];
              acc[c].s1 = A(0) + part[c].s1;
              acc[c].s2 = A(0) + part[c].s2;
            } else {
              multi::merge(acc[c], part[c]);
            }
          }
        }
      }
      T* const slices[6] = {o.sum, o.mean, o.mx, o.mn, o.var, o.sd};
      for (int64_t c = 0; c < n; ++c) {
        const multi::Finished<T> f = multi::finish<T>(acc[c], len, o.eps, o.mask);
        const T values[6] = {f.sum, f.mean, f.mx, f.mn, f.var, f.sd};
        for (int a = 0; a < 6; ++a)
          if (slices[a] != nullptr) slices[a][g * o.ldc + c] = values[a];
        if (o.arg_max != nullptr) o.arg_max[g * o.ldarg + c] = (I)acc[c].amax;
        if (o.arg_min != nullptr) o.arg_min[g * o.ldarg + c] = (I)acc[c].amin;
      }
    }
    any_neg = any_neg || neg;
  }
  OFX_REQUIRE(!any_neg, OFX_EINVAL,
              "spmm_csr_multi_cpu: negative column index (gather_kernel_util.cpp:80 "
              "CHECK_GE(idx, 0))");
  return OFX_OK;
}

}  // namespace

extern "C" int ofx_spmm_csr_multi_cpu(int num_threads, int idx_dtype, int val_dtype, int64_t m,
                                      int64_t k, int64_t n, int64_t nnz, const void* row_ptr,
                                      const void* col_idx, const void* values, const void* b,
                                      int64_t ldb, int aggr_mask, double eps, void* c, int64_t ldc,
                                      int64_t slice_stride, void* arg_max, void* arg_min,
                                      int64_t ldarg, int64_t row_begin, int64_t row_end,
                                      const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_READ_OPTIONS(opts, "spmm_csr_multi_cpu");
    bool nothing = false;
    const int rc = multi::check_multi_args("spmm_csr_multi_cpu", idx_dtype, val_dtype, m, k, n,
                                           nnz, row_ptr, col_idx, values, b, ldb, aggr_mask, eps, c,
                                           ldc, slice_stride, arg_max, arg_min, ldarg, row_begin,
                                           row_end, &nothing);
    if (rc || nothing) return rc;
    const Schedule s = resolve_schedule(n, opts);
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      return cpu_multi<T, I>(threads_of(num_threads), b ? k : 0, n, (const I*)row_ptr,
                             (const I*)col_idx, (const T*)values, (const T*)b, ldb,
                             multi::outputs_of<T, I>(aggr_mask, c, ldc, slice_stride, arg_max,
                                                     arg_min, ldarg, eps),
                             row_begin, row_end, s);
    });
  });
}

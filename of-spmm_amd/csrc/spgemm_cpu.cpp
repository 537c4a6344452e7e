// spgemm_cpu.cpp — the kCPU kernel of the CSR x CSR product: the same arrays, bit for bit, as
// spgemm.hip (rules in spgemm.h, contract in include/ofx_spmm.h).  The readable
// statement of the contract, not tuned: a thread keeps a dense accumulator over the n columns and a
// mark of the row that touched a column last; a row's touched columns are listed, sorted and
// written.  Rows are independent, so OpenMP runs over rows and nothing depends on num_threads.
#include <omp.h>

#include <algorithm>
#include <vector>

#include "ofx_internal.h"
#include "spgemm.h"
#include "spmm_common.h"

using namespace ofx;

namespace {

// The first bad row of a CSR with `rows` rows and nnz entries, or -1.
template <typename I>
int64_t first_bad_row(int nthreads, int64_t rows, int64_t nnz, const I* rp) {
  int64_t first_bad = INT64_MAX;
#pragma omp parallel for num_threads(nthreads) schedule(static) reduction(min : first_bad)
  for (int64_t i = 0; i < rows; ++i)
    if (!nsg::row_ok((int64_t)rp[i], (int64_t)rp[i + 1], nnz) && i < first_bad) first_bad = i;
  return first_bad == INT64_MAX ? -1 : first_bad;
}

// B's rows: 0 good, 1 a column outside [0, n), 2 not strictly ascending; *where: the first such row.
template <typename I>
int check_b_rows(int nthreads, int64_t k, int64_t n, const I* rp, const I* ci, int64_t* where) {
  int64_t outside = INT64_MAX, unsorted = INT64_MAX;
#pragma omp parallel for num_threads(nthreads) schedule(dynamic, 256) \
    reduction(min : outside) reduction(min : unsorted)
  for (int64_t r = 0; r < k; ++r)
    for (int64_t j = (int64_t)rp[r]; j < (int64_t)rp[r + 1]; ++j) {
      const int64_t c = (int64_t)ci[j];
      if ((c < 0 || c >= n) && r < outside) outside = r;
      if (j > (int64_t)rp[r] && c <= (int64_t)ci[j - 1] && r < unsorted) unsorted = r;
    }
  *where = outside != INT64_MAX ? outside : unsorted;
  return outside != INT64_MAX ? 1 : unsorted != INT64_MAX ? 2 : 0;
}

// The first row of A with a negative column, or -1.
template <typename I>
int64_t first_negative(int nthreads, int64_t m, const I* rp, const I* ci) {
  int64_t first = INT64_MAX;
#pragma omp parallel for num_threads(nthreads) schedule(dynamic, 256) reduction(min : first)
  for (int64_t i = 0; i < m; ++i)
    for (int64_t p = (int64_t)rp[i]; p < (int64_t)rp[i + 1]; ++p)
      if ((int64_t)ci[p] < 0 && i < first) first = i;
  return first == INT64_MAX ? -1 : first;
}

// One pass over the rows.  COUNT: counts[i + 1] = the distinct columns of row i.  Otherwise the
// columns, ascending, and (with values) the sums behind row_ptr_c.
template <bool COUNT, typename I, typename T>
void cpu_rows(int nthreads, int64_t m, int64_t k, int64_t n, const I* rp_a, const I* ci_a,
              const T* va, const I* rp_b, const I* ci_b, const T* vb, int64_t* counts,
              const I* rp_c, I* out_col, T* out_val) {
  using Acc = typename Num<T>::acc;
#pragma omp parallel num_threads(nthreads)
  {
    std::vector<int32_t> mark((size_t)n, -1);  // the row that touched the column last (m < 2^31)
    std::vector<Acc> acc(COUNT || out_val == nullptr ? (size_t)0 : (size_t)n);
    std::vector<int64_t> touched;
#pragma omp for schedule(dynamic, 64)
    for (int64_t i = 0; i < m; ++i) {
      touched.clear();
      for (int64_t p = (int64_t)rp_a[i]; p < (int64_t)rp_a[i + 1]; ++p) {
        const int64_t ca = (int64_t)ci_a[p];
        if (ca >= k) continue;  // a zero row: no product and no entry
        for (int64_t q = (int64_t)rp_b[ca]; q < (int64_t)rp_b[ca + 1]; ++q) {
          const int64_t c = (int64_t)ci_b[q];
          if (mark[(size_t)c] != (int32_t)i) {
            mark[(size_t)c] = (int32_t)i;
            touched.push_back(c);
            if (!acc.empty()) acc[(size_t)c] = Acc(0);
          }
          if (!acc.empty())
            acc[(size_t)c] =
                acc[(size_t)c] + Acc(Num<T>::mul(Num<T>::load(va[p]), Num<T>::load(vb[q])));
        }
      }
      if (COUNT) {
        counts[i + 1] = (int64_t)touched.size();
        continue;
      }
      std::sort(touched.begin(), touched.end());
      const int64_t o = (int64_t)rp_c[i];
      for (size_t r = 0; r < touched.size(); ++r) {
        out_col[o + (int64_t)r] = (I)touched[r];
        if (!acc.empty()) out_val[o + (int64_t)r] = Num<T>::store(acc[(size_t)touched[r]]);
      }
    }
  }
}

// Every check of the contract; after it no index is out of range.
template <typename I>
int check_inputs(const char* fn, int nt, int64_t m, int64_t k, int64_t n, int64_t nnz_a,
                 int64_t nnz_b, const I* rp_a, const I* ci_a, const I* rp_b, const I* ci_b) {
  const int64_t bad_a = first_bad_row<I>(nt, m, nnz_a, rp_a);
  OFX_REQUIRE(bad_a < 0, OFX_EINVAL,
              "%s: row %lld of A has the entry range [%lld, %lld): its degree is outside [0, 2^31) "
              "or its entries are outside [0, %lld)",
              fn, (long long)bad_a, (long long)rp_a[bad_a], (long long)rp_a[bad_a + 1],
              (long long)nnz_a);
  const int64_t bad_b = first_bad_row<I>(nt, k, nnz_b, rp_b);
  OFX_REQUIRE(bad_b < 0, OFX_EINVAL,
              "%s: row %lld of B has the entry range [%lld, %lld): its degree is outside [0, 2^31) "
              "or its entries are outside [0, %lld)",
              fn, (long long)bad_b, (long long)rp_b[bad_b], (long long)rp_b[bad_b + 1],
              (long long)nnz_b);
  const int64_t neg = first_negative<I>(nt, m, rp_a, ci_a);
  OFX_REQUIRE(neg < 0, OFX_EINVAL, "%s: row %lld of A holds a negative column: outside [0, %lld)",
              fn, (long long)neg, (long long)k);
  int64_t where = 0;
  const int what = check_b_rows<I>(nt, k, n, rp_b, ci_b, &where);
  OFX_REQUIRE(what != 1, OFX_EINVAL, "%s: row %lld of B holds a column outside [0, %lld)", fn,
              (long long)where, (long long)n);
  OFX_REQUIRE(what != 2, OFX_EINVAL,
              "%s: row %lld of B is not strictly ascending (pass B through coo_to_csr with "
              "merge_duplicates)",
              fn, (long long)where);
  return OFX_OK;
}

}  // namespace

extern "C" int ofx_spgemm_count_cpu(int num_threads, int idx_dtype, int64_t m, int64_t k, int64_t n,
                                    int64_t nnz_a, int64_t nnz_b, const void* rp_a,
                                    const void* ci_a, const void* rp_b, const void* ci_b,
                                    void* out_row_ptr, int64_t* out_nnz) {
  return ::ofx::guarded(__func__, [&]() -> int {
    const int rc = spg::check_count_args("spgemm_count_cpu", idx_dtype, m, k, n, nnz_a, nnz_b, rp_a,
                                         ci_a, rp_b, ci_b, out_row_ptr, out_nnz);
    if (rc) return rc;
    const int nt = threads_of(num_threads);
    return by_index(idx_dtype, [&](auto* ip) -> int {
      using I = std::remove_pointer_t<decltype(ip)>;
      const int rb = check_inputs<I>("spgemm_count_cpu", nt, m, k, n, nnz_a, nnz_b, (const I*)rp_a,
                                     (const I*)ci_a, (const I*)rp_b, (const I*)ci_b);
      if (rb) return rb;
      std::vector<int64_t> counts((size_t)m + 1, 0);
      cpu_rows<true, I, float>(nt, m, k, n, (const I*)rp_a, (const I*)ci_a, nullptr, (const I*)rp_b,
                               (const I*)ci_b, nullptr, counts.data(), nullptr, nullptr, nullptr);
      I* out_rp = (I*)out_row_ptr;
      out_rp[0] = (I)0;
      for (int64_t i = 0; i < m; ++i) {
        counts[(size_t)i + 1] += counts[(size_t)i];
        out_rp[i + 1] = (I)counts[(size_t)i + 1];
      }
      *out_nnz = counts[(size_t)m];
      return OFX_OK;
    });
  });
}

extern "C" int ofx_spgemm_fill_cpu(int num_threads, int idx_dtype, int val_dtype, int64_t m,
                                   int64_t k, int64_t n, int64_t nnz_a, int64_t nnz_b,
                                   int64_t nnz_c, const void* rp_a, const void* ci_a, const void* va,
                                   const void* rp_b, const void* ci_b, const void* vb,
                                   const void* row_ptr_c, void* out_col_idx, void* out_values) {
  return ::ofx::guarded(__func__, [&]() -> int {
    const int rc = spg::check_fill_args("spgemm_fill_cpu", idx_dtype, val_dtype, m, k, n, nnz_a,
                                        nnz_b, nnz_c, rp_a, ci_a, va, rp_b, ci_b, vb, row_ptr_c,
                                        out_col_idx, out_values);
    if (rc) return rc;
    const int nt = threads_of(num_threads);
    return by_types(idx_dtype, out_values ? val_dtype : OFX_DT_FLOAT, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      const int rb = check_inputs<I>("spgemm_fill_cpu", nt, m, k, n, nnz_a, nnz_b, (const I*)rp_a,
                                     (const I*)ci_a, (const I*)rp_b, (const I*)ci_b);
      if (rb) return rb;
      const I* rp_c = (const I*)row_ptr_c;
      OFX_REQUIRE(m == 0 || (int64_t)rp_c[m] == nnz_c, OFX_EINVAL,
                  "spgemm_fill_cpu: row_ptr_c ends at %lld, not at nnz_c %lld",
                  (long long)rp_c[m], (long long)nnz_c);
      cpu_rows<false, I, T>(nt, m, k, n, (const I*)rp_a, (const I*)ci_a, (const T*)va,
                            (const I*)rp_b, (const I*)ci_b, (const T*)vb, nullptr, rp_c,
                            (I*)out_col_idx, (T*)out_values);
      return OFX_OK;
    });
  });
}

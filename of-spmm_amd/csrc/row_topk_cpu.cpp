// row_topk_cpu.cpp — the kCPU kernel of the per-row top-k selection: the same arrays, bit for bit,
// as row_topk.hip (rules in row_topk.h, contract in include/ofx_spmm.h).  Rows are
// independent, so both passes run over rows under OpenMP and the output does not depend on
// num_threads.  A row longer than k: std::nth_element over (key, position) pairs in the order
// "larger key first, lower position first", which is total, then the kept positions ascending.
#include <omp.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "ofx_internal.h"
#include "row_topk.h"
#include "spmm_common.h"

using namespace ofx;

namespace {

// out_rp[i + 1] = min(deg, k); the first bad row, or -1.
template <typename I>
int64_t cpu_lengths(int nthreads, int64_t m, int64_t nnz, const I* rp, int k, I* out_rp) {
  int64_t first_bad = INT64_MAX;
#pragma omp parallel for num_threads(nthreads) schedule(static) reduction(min : first_bad)
  for (int64_t i = 0; i < m; ++i) {
    const int64_t lo = (int64_t)rp[i], hi = (int64_t)rp[i + 1];
    int64_t len = 0;
    if (nsg::row_ok(lo, hi, nnz))
      len = hi - lo < (int64_t)k ? hi - lo : (int64_t)k;
    else if (i < first_bad)
      first_bad = i;
    out_rp[i + 1] = (I)len;
  }
  return first_bad == INT64_MAX ? -1 : first_bad;
}

template <typename I, typename U>
void cpu_select(int nthreads, int64_t m, const I* rp, const I* ci, const U* values, int k, U flip,
                const I* out_rp, I* out_col, I* out_eid) {
#pragma omp parallel num_threads(nthreads)
  {
    std::vector<std::pair<U, int>> keyed;  // (key, position), this thread's
    std::vector<int> kept;
#pragma omp for schedule(dynamic, 256)
    for (int64_t i = 0; i < m; ++i) {
      const int64_t begin = (int64_t)rp[i];
      const int deg = (int)((int64_t)rp[i + 1] - begin);
      const int64_t o = (int64_t)out_rp[i];
      const int len = deg < k ? deg : k;
      kept.resize((size_t)len);
      if (deg <= k) {
        for (int p = 0; p < deg; ++p) kept[(size_t)p] = p;
      } else {
        keyed.resize((size_t)deg);
        for (int p = 0; p < deg; ++p) keyed[(size_t)p] = {rtk::key_of(values[begin + p], flip), p};
        std::nth_element(keyed.begin(), keyed.begin() + (k - 1), keyed.end(),
                         [](const std::pair<U, int>& a, const std::pair<U, int>& b) {
                           return a.first != b.first ? a.first > b.first : a.second < b.second;
                         });
        for (int t = 0; t < k; ++t) kept[(size_t)t] = keyed[(size_t)t].second;
        std::sort(kept.begin(), kept.end());
      }
      for (int t = 0; t < len; ++t) {
        const int64_t e = begin + kept[(size_t)t];
        out_col[o + t] = ci[e];
        if (out_eid != nullptr) out_eid[o + t] = (I)e;
      }
    }
  }
}

}  // namespace

extern "C" int ofx_row_topk_cpu(int num_threads, int idx_dtype, int val_dtype, int64_t m,
                                int64_t nnz, const void* row_ptr, const void* col_idx,
                                const void* values, int64_t k, int largest, void* out_row_ptr,
                                void* out_col_idx, void* out_edge_ids, int64_t* out_nnz) {
  return ::ofx::guarded(__func__, [&]() -> int {
    const int rc = rtk::check_topk_args("row_topk_cpu", idx_dtype, val_dtype, m, nnz, row_ptr,
                                        col_idx, values, k, out_row_ptr, out_col_idx, out_nnz);
    if (rc) return rc;
    const int nt = threads_of(num_threads);
    const int kk = rtk::clamp_k(k);
    return by_index(idx_dtype, [&](auto* ip) -> int {
      using I = std::remove_pointer_t<decltype(ip)>;
      const I* rp = (const I*)row_ptr;
      I* out_rp = (I*)out_row_ptr;
      out_rp[0] = (I)0;
      const int64_t bad = cpu_lengths<I>(nt, m, nnz, rp, kk, out_rp);
      OFX_REQUIRE(bad < 0, OFX_EINVAL,
                  "row_topk_cpu: row %lld has the entry range [%lld, %lld): its degree is outside "
                  "[0, 2^31) or its entries are outside [0, %lld)",
                  (long long)bad, (long long)rp[bad], (long long)rp[bad + 1], (long long)nnz);
      for (int64_t i = 0; i < m; ++i) out_rp[i + 1] = (I)(out_rp[i + 1] + out_rp[i]);
      *out_nnz = (int64_t)out_rp[m];
      return rtk::by_key(val_dtype, [&](auto* up) -> int {
        using U = std::remove_pointer_t<decltype(up)>;
        cpu_select<I, U>(nt, m, rp, (const I*)col_idx, (const U*)values, kk,
                         largest ? (U)0 : (U)~(U)0, out_rp, (I*)out_col_idx, (I*)out_edge_ids);
        return OFX_OK;
      });
    });
  });
}

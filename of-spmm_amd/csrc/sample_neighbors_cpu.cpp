// sample_neighbors_cpu.cpp — the kCPU kernel of the neighbour sampler: the same arrays, bit for
// bit, as sample_neighbors.hip (rules in sample_neighbors.h, contract in include/ofx_spmm.h).
// Seeds are independent (the draw is keyed by the node), so the two passes run over seeds under
// OpenMP and the output does not depend on num_threads.
#include <omp.h>

#include "ofx_internal.h"
#include "sample_neighbors.h"
#include "spmm_common.h"

using namespace ofx;

namespace {

// out_rp[i + 1] = the length of output row i; the first bad seed's position, or -1.
template <typename I>
int64_t cpu_lengths(int nthreads, int64_t m, int64_t num_seeds, const I* rp, const I* seeds,
                    int fanout, I* out_rp) {
  int64_t first_bad = INT64_MAX;
#pragma omp parallel for num_threads(nthreads) schedule(static) reduction(min : first_bad)
  for (int64_t i = 0; i < num_seeds; ++i) {
    const smp::RowOf row = smp::row_of(rp, m, (int64_t)seeds[i], fanout);
    out_rp[i + 1] = (I)row.len;
    if (row.bad && i < first_bad) first_bad = i;
  }
  return first_bad == INT64_MAX ? -1 : first_bad;
}

template <typename I>
void cpu_sample(int nthreads, int64_t m, int64_t num_seeds, const I* rp, const I* ci,
                const I* seeds, int fanout, uint64_t seed, const I* out_rp, I* out_col,
                I* out_eid) {
#pragma omp parallel for num_threads(nthreads) schedule(dynamic, 256)
  for (int64_t i = 0; i < num_seeds; ++i) {
    const int64_t v = (int64_t)seeds[i];
    const smp::RowOf row = smp::row_of(rp, m, v, fanout);
    uint32_t pos[smp::kMaxFanout];
    if (row.deg > (int64_t)fanout)
      smp::sample_positions((uint64_t)v, (uint32_t)row.deg, fanout, seed, pos);
    else
      for (int t = 0; t < row.len; ++t) pos[t] = (uint32_t)t;
    const int64_t o = (int64_t)out_rp[i];
    for (int t = 0; t < row.len; ++t) {
      const int64_t e = row.begin + (int64_t)pos[t];
      out_col[o + t] = ci[e];
      if (out_eid != nullptr) out_eid[o + t] = (I)e;
    }
  }
}

}  // namespace

extern "C" int ofx_sample_neighbors_cpu(int num_threads, int idx_dtype, int64_t m,
                                        int64_t num_seeds, const void* row_ptr, const void* col_idx,
                                        const void* seeds, int fanout, uint64_t seed,
                                        void* out_row_ptr, void* out_col_idx, void* out_edge_ids,
                                        int64_t* out_nnz) {
  return ::ofx::guarded(__func__, [&]() -> int {
    const int rc =
        smp::check_sample_args("sample_neighbors_cpu", idx_dtype, m, num_seeds, row_ptr, col_idx,
                               seeds, fanout, out_row_ptr, out_col_idx, out_nnz);
    if (rc) return rc;
    const int nt = threads_of(num_threads);
    return by_index(idx_dtype, [&](auto* ip) -> int {
      using I = std::remove_pointer_t<decltype(ip)>;
      I* out_rp = (I*)out_row_ptr;
      out_rp[0] = (I)0;
      const int64_t bad = cpu_lengths<I>(nt, m, num_seeds, (const I*)row_ptr, (const I*)seeds,
                                         fanout, out_rp);
      OFX_REQUIRE(bad < 0, OFX_EINVAL,
                  "sample_neighbors_cpu: seed %lld at position %lld is outside [0, %lld), or its "
                  "row's degree is outside [0, 2^31)",
                  (long long)((const I*)seeds)[bad], (long long)bad, (long long)m);
      for (int64_t i = 0; i < num_seeds; ++i) out_rp[i + 1] = (I)(out_rp[i + 1] + out_rp[i]);
      cpu_sample<I>(nt, m, num_seeds, (const I*)row_ptr, (const I*)col_idx, (const I*)seeds, fanout,
                    seed, out_rp, (I*)out_col_idx, (I*)out_edge_ids);
      *out_nnz = (int64_t)out_rp[num_seeds];
      return OFX_OK;
    });
  });
}

// random_walk_cpu.cpp — the kCPU kernel of the random walks: the same arrays, bit for bit, as
// random_walk.hip (rules in random_walk.h, contract in include/ofx_spmm.h).  A walk
// depends on (seed, i, starts[i]) alone, so the walks run under OpenMP and the output does not
// depend on num_threads.
#include <omp.h>

#include "ofx_internal.h"
#include "random_walk.h"
#include "spmm_common.h"

using namespace ofx;

namespace {

// The walks; the first walk that met a bad start or a bad row, or -1.
template <typename I>
int64_t cpu_walks(int nthreads, int64_t m, int64_t nnz, int64_t num_walks, const I* rp, const I* ci,
                  const I* starts, int length, const rw::Thresholds& th, uint64_t seed, I* walks,
                  I* eids) {
  int64_t first_bad = INT64_MAX;
#pragma omp parallel for num_threads(nthreads) schedule(dynamic, 256) reduction(min : first_bad)
  for (int64_t i = 0; i < num_walks; ++i) {
    I* w = walks + i * ((int64_t)length + 1);
    I* eo = eids ? eids + i * (int64_t)length : nullptr;
    int64_t v = (int64_t)starts[i];
    w[0] = (I)v;
    bool bad = v < 0 || v >= m;
    rw::Row row = rw::row_of(rp, m, nnz, v);
    int64_t u = -1, ub = 0, ue = 0;
    for (int t = 1; t <= length; ++t) {
      bad = bad || row.bad;
      int64_t x = -1, e = -1;
      if (!row.ended) {
        e = rw::step(ci, (uint64_t)i, (uint32_t)t, seed, th, row.begin, row.end, t >= 2, u, ub, ue);
        x = (int64_t)ci[e];
        u = v;
        ub = row.begin;
        ue = row.end;
        v = x;
        if (t < length) row = rw::row_of(rp, m, nnz, v);  // the last node's row is not read
      }
      w[t] = (I)x;
      if (eo) eo[t - 1] = (I)e;
    }
    if (bad && i < first_bad) first_bad = i;
  }
  return first_bad == INT64_MAX ? -1 : first_bad;
}

}  // namespace

extern "C" int ofx_random_walk_cpu(int num_threads, int idx_dtype, int64_t m, int64_t nnz,
                                   int64_t num_walks, const void* row_ptr, const void* col_idx,
                                   const void* starts, int length, double p, double q,
                                   uint64_t seed, void* out_walks, void* out_edge_ids) {
  return ::ofx::guarded(__func__, [&]() -> int {
    rw::Thresholds th;
    const int rc = rw::check_walk_args("random_walk_cpu", idx_dtype, m, nnz, num_walks, row_ptr,
                                       col_idx, starts, length, p, q, out_walks, &th);
    if (rc) return rc;
    const int nt = threads_of(num_threads);
    return by_index(idx_dtype, [&](auto* ip) -> int {
      using I = std::remove_pointer_t<decltype(ip)>;
      const int64_t bad =
          cpu_walks<I>(nt, m, nnz, num_walks, (const I*)row_ptr, (const I*)col_idx,
                       (const I*)starts, length, th, seed, (I*)out_walks, (I*)out_edge_ids);
      OFX_REQUIRE(bad < 0, OFX_EINVAL,
                  "random_walk_cpu: walk %lld starts outside [0, %lld), or reads a row whose degree "
                  "is outside [0, 2^31) or whose entries are outside [0, %lld)",
                  (long long)bad, (long long)m, (long long)nnz);
      return OFX_OK;
    });
  });
}

// spmm_edge_cpu.cpp — the DeviceType::kCPU kernels of ops "spmm_csr_edge", "spmm_csr_edge_grad_e"
// and "spmm_csr_edge_grad_b" (the SpMM over per-edge feature vectors and its gradients; contract
// in include/ofx_spmm.h).  One row template serves the three entries, in the style
// of spmm_rows_cpu.h: the walk over a run of a row's nonzeros with the gathered row and the e row
// of each, and what is done with the pair (spmm_edge.h's message and gradient terms, the steps the
// HIP kernels of spmm_edge.hip / spmm_edge_grad.hip take) is the entry's.  The sums add in the
// contract's order whatever the thread count: a row is one thread's.
#pragma clang fp contract(off)

#include <omp.h>

#include <vector>

#include "ofx_internal.h"
#include "spmm_common.h"
#include "spmm_edge.h"

using namespace ofx;

namespace {

// f(j, xrow) for the nonzeros jt of [j0, j1), ascending: j = perm ? perm[jt] : jt (the e row) and
// xrow = X + col[jt] * ldx, or NULL for a column outside [0, kx) (the row reads as +0).
template <typename T, typename I, typename F>
void edge_row(const I* col, const I* perm, const T* X, int64_t ldx, int64_t kx, int64_t j0,
              int64_t j1, F&& f) {
  for (int64_t jt = j0; jt < j1; ++jt) {
    const int64_t cj = (int64_t)col[jt];
    f(perm ? (int64_t)perm[jt] : jt, (uint64_t)cj < (uint64_t)kx ? X + cj * ldx : nullptr);
  }
}

// out[g, :] for rows [row_begin, row_end) of the CSR (rp, col, perm): the sum over the row's
// nonzeros of term(g, j, xrow, c) in the accumulation type, a row of at most s.split nonzeros in
// one in-order sum, a longer one as the in-order sum of its chunks' sums; one rounding to T.
template <typename T, typename I, typename F>
void edge_row_sums(int nthreads, const I* rp, const I* col, const I* perm, const T* X, int64_t ldx,
                   int64_t kx, int64_t n, T* out, int64_t ldc, int64_t row_begin, int64_t row_end,
                   const Schedule& s, F&& term) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  const int64_t rows = row_end - row_begin;
#pragma omp parallel num_threads(nthreads)
  {
    std::vector<A> acc(n), part(n);
#pragma omp for schedule(dynamic, 64)
    for (int64_t g = 0; g < rows; ++g) {
      const int64_t j0 = (int64_t)rp[row_begin + g], j1 = (int64_t)rp[row_begin + g + 1];
      const auto run = [&](int64_t a, int64_t e, A* sum) {
        for (int64_t c = 0; c < n; ++c) sum[c] = A(0);
        edge_row<T, I>(col, perm, X, ldx, kx, a, e, [&](int64_t j, const T* xrow) {
          for (int64_t c = 0; c < n; ++c) sum[c] = sum[c] + term(g, j, xrow, c);
        });
      };
      if (j1 - j0 <= s.split) {
        run(j0, j1, acc.data());
      } else {
        const int64_t nc = num_chunks(j1 - j0, s.chunk);
        for (int64_t c = 0; c < n; ++c) acc[c] = A(0);
        for (int64_t q = 0; q < nc; ++q) {
          const int64_t a = j0 + q * s.chunk;
          run(a, q == nc - 1 ? j1 : a + s.chunk, part.data());
          for (int64_t c = 0; c < n; ++c) acc[c] = acc[c] + part[c];
        }
      }
      for (int64_t c = 0; c < n; ++c) out[g * ldc + c] = Num<T>::store(acc[c]);
    }
  }
}

template <typename T>
typename Num<T>::acc at(const T* row, int64_t c) {
  return row != nullptr ? Num<T>::load(row[c]) : typename Num<T>::acc(0);
}

// de[j, :] for the nonzeros j of rows [row_begin, row_end); dy holds the rows from row_begin on.
template <typename T, typename I, int OP, bool RELU>
void edge_grad_e_rows(int nthreads, const I* rp, const I* col, const T* E, const T* B, int64_t ldb,
                      int64_t k, int64_t n, const T* dy, int64_t lddy, T* de, int64_t row_begin,
                      int64_t row_end) {
#pragma omp parallel for num_threads(nthreads) schedule(dynamic, 64)
  for (int64_t r = row_begin; r < row_end; ++r) {
    const T* grow = dy + (r - row_begin) * lddy;
    edge_row<T, I>(col, (const I*)nullptr, B, ldb, k, (int64_t)rp[r], (int64_t)rp[r + 1],
                   [&](int64_t j, const T* brow) {
                     for (int64_t c = 0; c < n; ++c) {
                       const typename Num<T>::acc bv = at(brow, c);
                       de[j * n + c] = edge::grad_term<T, OP, RELU>(grow[c], bv, bv,
                                                                    Num<T>::load(E[j * n + c]));
                     }
                   });
  }
}

}  // namespace

extern "C" int ofx_spmm_csr_edge_cpu(int num_threads, int idx_dtype, int val_dtype, int64_t m,
                                     int64_t k, int64_t n, int64_t nnz, const void* row_ptr,
                                     const void* col_idx, const void* e, const void* b,
                                     int64_t ldb, int op, int act, void* c, int64_t ldc,
                                     int64_t row_begin, int64_t row_end,
                                     const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_READ_OPTIONS(opts, "spmm_csr_edge_cpu");
    bool nothing = false;
    const int rc = edge::check_edge_args("spmm_csr_edge_cpu", false, idx_dtype, val_dtype, m, k, n,
                                         nnz, row_ptr, col_idx, e, b, ldb, op, act, nullptr, 0, c,
                                         ldc, row_begin, row_end, opts, &nothing);
    if (rc || nothing) return rc;
    const Schedule s = resolve_schedule(n, opts);
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      const T* E = (const T*)e;
      return edge::by_op_act(op, act, [&](auto o, auto relu) -> int {
        edge_row_sums<T, I>(threads_of(num_threads), (const I*)row_ptr, (const I*)col_idx,
                            (const I*)nullptr, (const T*)b, ldb, b ? k : 0, n, (T*)c, ldc,
                            row_begin, row_end, s,
                            [&](int64_t, int64_t j, const T* brow, int64_t col) {
                              return edge::message<T, decltype(o)::value, decltype(relu)::value>(
                                  at(brow, col), Num<T>::load(E[j * n + col]));
                            });
        return OFX_OK;
      });
    });
  });
}

extern "C" int ofx_spmm_csr_edge_grad_e_cpu(int num_threads, int idx_dtype, int val_dtype,
                                            int64_t m, int64_t k, int64_t n, int64_t nnz,
                                            const void* row_ptr, const void* col_idx,
                                            const void* e, const void* b, int64_t ldb, int op,
                                            int act, const void* dy, int64_t lddy, void* de,
                                            int64_t row_begin, int64_t row_end) {
  return ::ofx::guarded(__func__, [&]() -> int {
    bool nothing = false;
    const int rc = edge::check_edge_args("spmm_csr_edge_grad_e_cpu", true, idx_dtype, val_dtype, m,
                                         k, n, nnz, row_ptr, col_idx, e, b, ldb, op, act, dy, lddy,
                                         de, 0, row_begin, row_end, nullptr, &nothing);
    if (rc || nothing) return rc;
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      return edge::by_op_act(op, act, [&](auto o, auto relu) -> int {
        edge_grad_e_rows<T, I, decltype(o)::value, decltype(relu)::value>(
            threads_of(num_threads), (const I*)row_ptr, (const I*)col_idx, (const T*)e,
            (const T*)b, ldb, b ? k : 0, n, (const T*)dy, lddy, (T*)de, row_begin, row_end);
        return OFX_OK;
      });
    });
  });
}

extern "C" int ofx_spmm_csr_edge_grad_b_cpu(int num_threads, int idx_dtype, int val_dtype,
                                            int64_t m, int64_t k, int64_t n, int64_t nnz,
                                            const void* row_ptr_t, const void* col_idx_t,
                                            const void* perm, const void* e, const void* b,
                                            int64_t ldb, int op, int act, const void* dy,
                                            int64_t lddy, void* db, int64_t lddb,
                                            int64_t row_begin, int64_t row_end,
                                            const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_READ_OPTIONS(opts, "spmm_csr_edge_grad_b_cpu");
    bool nothing = false;
    const int rc = edge::check_edge_grad_b_args("spmm_csr_edge_grad_b_cpu", idx_dtype, val_dtype,
                                                m, k, n, nnz, row_ptr_t, col_idx_t, perm, e, b,
                                                ldb, op, act, dy, lddy, db, lddb, row_begin,
                                                row_end, opts, &nothing);
    if (rc || nothing) return rc;
    const Schedule s = resolve_schedule(n, opts);
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      const T *E = (const T*)e, *B = (const T*)b;
      const T zero = Num<T>::store(typename Num<T>::acc(0));
      return edge::by_op_act(op, act, [&](auto o, auto relu) -> int {
        edge_row_sums<T, I>(
            threads_of(num_threads), (const I*)row_ptr_t, (const I*)col_idx_t, (const I*)perm,
            (const T*)dy, lddy, dy ? m : 0, n, (T*)db, lddb, row_begin, row_end, s,
            [&](int64_t g, int64_t j, const T* grow, int64_t col) {
              // a perm entry outside [0, nnz) (never from ofx_csr_transpose) reads e row 0
              const int64_t je = (uint64_t)j < (uint64_t)nnz ? j : 0;
              const auto ev = Num<T>::load(E[je * n + col]);
              return Num<T>::load(edge::grad_term<T, decltype(o)::value, decltype(relu)::value>(
                  grow != nullptr ? grow[col] : zero, ev, Num<T>::load(B[g * ldb + col]), ev));
            });
        return OFX_OK;
      });
    });
  });
}

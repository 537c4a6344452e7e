// graph_attention_heads_cpu.cpp — the DeviceType::kCPU kernel of op "graph_attention_csr_heads"
// (contract in include/ofx_spmm.h): the three kCPU kernels of the composition one
// after the other with attn as the intermediate (the softmax normalises it in place: it reads a
// row's head into its own buffer before it writes), which has the contract's bits by construction.
#include "graph_attention.h"

using namespace ofx;

extern "C" int ofx_graph_attention_csr_heads_cpu(int num_threads, int idx_dtype, int val_dtype,
                                                 int64_t m, int64_t k, int64_t heads, int64_t d,
                                                 int64_t nnz, const void* row_ptr,
                                                 const void* col_idx, const void* q, int64_t ldq,
                                                 const void* kmat, int64_t ldk, const void* v,
                                                 int64_t ldv, void* out, int64_t ldo, void* attn,
                                                 int64_t row_begin, int64_t row_end,
                                                 const ofx_spmm_options* opts) {
  const ofx_spmm_options* caller_opts = opts;
  gat::Shape sh;
  const int rc = ::ofx::guarded(__func__, [&]() -> int {
    OFX_READ_OPTIONS(opts, "graph_attention_csr_heads_cpu");
    return gat::check_graph_attention_args("graph_attention_csr_heads_cpu", idx_dtype, val_dtype, m,
                                           k, heads, d, nnz, row_ptr, col_idx, q, ldq, kmat, ldk, v,
                                           ldv, out, ldo, attn, row_begin, row_end, opts, &sh);
  });
  if (rc != OFX_OK || sh.nothing) return rc;
  if (int r = ofx_sddmm_csr_heads_cpu(num_threads, idx_dtype, val_dtype, m, k, heads, d, nnz,
                                      row_ptr, col_idx, q, ldq, kmat, ldk, attn, row_begin, row_end))
    return r;
  if (int r = ofx_edge_softmax_csr_heads_cpu(num_threads, idx_dtype, val_dtype, m, heads, nnz,
                                             row_ptr, attn, attn, row_begin, row_end, caller_opts))
    return r;
  return ofx_spmm_csr_heads_cpu(num_threads, idx_dtype, val_dtype, m, k, heads, d, nnz, row_ptr,
                                col_idx, attn, v, ldv, out, ldo, row_begin, row_end, caller_opts);
}

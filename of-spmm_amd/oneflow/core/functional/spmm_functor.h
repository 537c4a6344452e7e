// spmm_functor.h — the functional layer's internal C++ entries shared by the eager functor
// (spmm_functor.cpp), the compiled row-split job (ccl_functor.cpp) and the kernel's state
// (user/kernels/spmm_kernel.cpp).  The C-ABI entries in include/ofx_spmm.h wrap these.
#ifndef OFX_ONEFLOW_CORE_FUNCTIONAL_SPMM_FUNCTOR_H_
#define OFX_ONEFLOW_CORE_FUNCTIONAL_SPMM_FUNCTOR_H_

#include <memory>

#include "oneflow/core/framework/framework.h"
#include "ofx_spmm.h"

namespace oneflow {

// functional::SpmmCsr on one rank of a placement with an explicit kernel state: the lazy path's
// form, where each compiled op owns its OpKernelState (core/kernel/user_kernel.cpp keeps it per
// UserKernel).  *state is created through the registered kernel's CreateOpKernelState on the
// first launching call that has none.  static_csr is the op attribute (include/ofx_spmm.h
// ofx_spmm_attrs).
int SpmmCsrGlobalWithState(void* stream, const ofx_tensor_desc* row_ptr,
                           const ofx_tensor_desc* col_idx, const ofx_tensor_desc* values,
                           int64_t m, int64_t k, const ofx_tensor_desc* b, int64_t b_logical_cols,
                           ofx_tensor_desc* out, void* tmp, size_t tmp_bytes, int hierarchy_ndim,
                           const int64_t* hierarchy, const int32_t* out_split_axes,
                           int64_t parallel_id, int64_t static_csr,
                           std::shared_ptr<user_op::OpKernelState>* state);

// The static-CSR plan counters of a spmm_csr kernel state, added to *entries / *plans / *hits
// (release: its workspaces are freed first).  False when `state` is not one.
bool SpmmCsrPlanStateStats(user_op::OpKernelState* state, int64_t* entries, int64_t* plans,
                           int64_t* hits, bool release);

// functional::EdgeSoftmaxCsr / EdgeSoftmaxCsrGrad: ops "edge_softmax_csr" (in = e, grad == NULL)
// and "edge_softmax_csr_grad" (in = y, grad = dy) through the op-registry dispatch.  With
// tmp_size_out != NULL only the tmp-buffer size is computed.  num_threads: CPU kernel only.
int EdgeSoftmaxCsr(void* stream, const ofx_tensor_desc* row_ptr, const ofx_tensor_desc* col_idx,
                   const ofx_tensor_desc* in, const ofx_tensor_desc* grad, ofx_tensor_desc* out,
                   void* tmp, size_t tmp_bytes, size_t* tmp_size_out, int num_threads);

// functional::EdgeSoftmaxCsrHeads / EdgeSoftmaxCsrHeadsGrad: the same for ops
// "edge_softmax_csr_heads" (in = e [nnz, H]) and "edge_softmax_csr_heads_grad" (in = y, grad = dy).
int EdgeSoftmaxCsrHeads(void* stream, const ofx_tensor_desc* row_ptr,
                        const ofx_tensor_desc* col_idx, const ofx_tensor_desc* in,
                        const ofx_tensor_desc* grad, ofx_tensor_desc* out, void* tmp,
                        size_t tmp_bytes, size_t* tmp_size_out, int num_threads);

// functional::GatSoftmaxCsrHeads / GatSoftmaxCsrHeadsGrad: ops "gat_softmax_csr_heads" (dy == NULL:
// s_row [M, H], s_col [K, H] -> out [nnz, H]) and "gat_softmax_csr_heads_grad" (y, dy [nnz, H] ->
// out = ds [nnz, H], d_row [M, H]); negative_slope is the ops' attr.
int GatSoftmaxCsrHeads(void* stream, const ofx_tensor_desc* row_ptr, const ofx_tensor_desc* col_idx,
                       const ofx_tensor_desc* s_row, const ofx_tensor_desc* s_col,
                       const ofx_tensor_desc* y, const ofx_tensor_desc* dy, double negative_slope,
                       ofx_tensor_desc* out, ofx_tensor_desc* d_row, void* tmp, size_t tmp_bytes,
                       size_t* tmp_size_out, int num_threads);

}  // namespace oneflow

#endif  // OFX_ONEFLOW_CORE_FUNCTIONAL_SPMM_FUNCTOR_H_

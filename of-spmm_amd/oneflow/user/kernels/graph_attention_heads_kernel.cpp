/*
 * graph_attention_heads_kernel.cpp — kernels of op "graph_attention_csr_heads" for
 * DeviceType::kCPU and DeviceType::kHIP (same registration pattern as spmm_heads_kernel.cpp;
 * device work through the C-ABI of include/ofx_spmm.h).  Two outputs: out [M, N] and
 * attn [nnz, H], the latter also the HIP kernel's hand-off buffer between its phases.
 */
#include "oneflow/core/framework/framework.h"
#include "oneflow/user/kernels/csr_kernel_util.h"
#include "ofx_spmm.h"

namespace oneflow {

namespace {

template <DeviceType device_type>
class GraphAttentionCsrHeadsKernel final : public user_op::OpKernel,
                                           public user_op::CudaGraphSupport {
 public:
  bool AlwaysComputeWhenAllOutputsEmpty() const override { return false; }

 private:
  using user_op::OpKernel::Compute;
  void Compute(user_op::KernelComputeContext* ctx, user_op::OpKernelState*,
               const user_op::OpKernelCache*) const override {
    const user_op::Tensor* row_ptr = ctx->Tensor4ArgNameAndIndex("a_csr_row_ptr", 0);
    const user_op::Tensor* col_idx = ctx->Tensor4ArgNameAndIndex("a_csr_col_idx", 0);
    const user_op::Tensor* q = ctx->Tensor4ArgNameAndIndex("q", 0);
    const user_op::Tensor* k = ctx->Tensor4ArgNameAndIndex("k", 0);
    const user_op::Tensor* v = ctx->Tensor4ArgNameAndIndex("v", 0);
    user_op::Tensor* out = ctx->Tensor4ArgNameAndIndex("out", 0);
    user_op::Tensor* attn = ctx->Tensor4ArgNameAndIndex("attn", 0);
    const int64_t m = row_ptr->shape_view().elem_cnt() - 1;
    const int64_t kk = k->shape_view().At(0);
    const int64_t n = k->shape_view().At(1);
    const int64_t nnz = col_idx->shape_view().elem_cnt();
    const int64_t heads = ctx->Attr<int64_t>("num_heads");
    const int64_t d = heads > 0 ? n / heads : 0;
    const int idx_dt = DtCode(row_ptr->data_type()), val_dt = DtCode(k->data_type());
    int rc;
    if (device_type == DeviceType::kHIP) {
      const TmpBuffer tmp(ctx);
      void* stream = ctx->stream()->As<ep::HipStream>()->hip_stream();
      rc = ofx_graph_attention_csr_heads(stream, idx_dt, val_dt, m, kk, heads, d, nnz,
                                         row_ptr->dptr(), col_idx->dptr(), q->dptr(),
                                         q->row_stride(), k->dptr(), k->row_stride(), v->dptr(),
                                         v->row_stride(), out->mut_dptr(), out->row_stride(),
                                         attn->mut_dptr(), 0, m, tmp.ptr, tmp.bytes, nullptr);
    } else {
      const int threads = ctx->stream()->As<ep::CpuStream>()->num_threads();
      rc = ofx_graph_attention_csr_heads_cpu(threads, idx_dt, val_dt, m, kk, heads, d, nnz,
                                             row_ptr->dptr(), col_idx->dptr(), q->dptr(),
                                             q->row_stride(), k->dptr(), k->row_stride(),
                                             v->dptr(), v->row_stride(), out->mut_dptr(),
                                             out->row_stride(), attn->mut_dptr(), 0, m, nullptr);
    }
    OFX_KERNEL_CHECK(rc == OFX_OK, "graph_attention_csr_heads kernel failed (" << rc << "): "
                                                                               << ofx_last_error());
  }
};

size_t InferGraphAttentionTmpSize(user_op::InferSizeContext* ctx) {
  const user_op::TensorDesc& row_ptr = ctx->InputTensorDesc("a_csr_row_ptr", 0);
  const user_op::TensorDesc& col_idx = ctx->InputTensorDesc("a_csr_col_idx", 0);
  const user_op::TensorDesc& k = ctx->InputTensorDesc("k", 0);
  const int64_t heads = ctx->Attr<int64_t>("num_heads");
  const int64_t d = heads > 0 ? k.shape().At(1) / heads : 0;
  size_t bytes = 0;
  const int rc = ofx_graph_attention_csr_heads_workspace_size(
      DtCode(row_ptr.data_type()), DtCode(k.data_type()), row_ptr.shape().At(0) - 1,
      k.shape().At(0), heads, d, col_idx.shape().At(0), nullptr, &bytes);
  return rc == OFX_OK ? bytes : 0;
}

}  // namespace

REGISTER_CSR_KERNEL_ALL_DTYPES("graph_attention_csr_heads", "out", "a_csr_row_ptr", DeviceType::kCPU, NoTmp,
                               GraphAttentionCsrHeadsKernel<DeviceType::kCPU>)
REGISTER_CSR_KERNEL_ALL_DTYPES("graph_attention_csr_heads", "out", "a_csr_row_ptr", DeviceType::kHIP, InferGraphAttentionTmpSize,
                               GraphAttentionCsrHeadsKernel<DeviceType::kHIP>)

}  // namespace oneflow

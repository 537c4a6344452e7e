/*
 * edge_softmax_heads_kernel.cpp — kernels of ops "edge_softmax_csr_heads" and
 * "edge_softmax_csr_heads_grad" for DeviceType::kCPU and DeviceType::kHIP (same registration
 * pattern as edge_softmax_kernel.cpp; device work through the C-ABI of include/ofx_spmm.h).
 */
#include "oneflow/core/framework/framework.h"
#include "oneflow/user/kernels/csr_kernel_util.h"
#include "ofx_spmm.h"

namespace oneflow {

namespace {

// GRAD: inputs y, dy [nnz, H] -> dx; else input e [nnz, H] -> out.
template <DeviceType device_type, bool GRAD>
class EdgeSoftmaxCsrHeadsKernel final : public user_op::OpKernel,
                                        public user_op::CudaGraphSupport {
 public:
  bool AlwaysComputeWhenAllOutputsEmpty() const override { return false; }

 private:
  using user_op::OpKernel::Compute;
  void Compute(user_op::KernelComputeContext* ctx, user_op::OpKernelState*,
               const user_op::OpKernelCache*) const override {
    const user_op::Tensor* row_ptr = ctx->Tensor4ArgNameAndIndex("a_csr_row_ptr", 0);
    const user_op::Tensor* a = ctx->Tensor4ArgNameAndIndex(GRAD ? "y" : "e", 0);
    const user_op::Tensor* dy = GRAD ? ctx->Tensor4ArgNameAndIndex("dy", 0) : nullptr;
    user_op::Tensor* out = ctx->Tensor4ArgNameAndIndex(GRAD ? "dx" : "out", 0);
    const int64_t m = row_ptr->shape_view().elem_cnt() - 1;
    const int64_t nnz = a->shape_view().At(0);
    const int64_t heads = a->shape_view().At(1);
    const int idx_dt = DtCode(row_ptr->data_type()), val_dt = DtCode(a->data_type());
    const char* name = GRAD ? "edge_softmax_csr_heads_grad" : "edge_softmax_csr_heads";
    // the C-ABI takes packed [nnz, H] tensors: no row stride
    OFX_KERNEL_CHECK(a->row_stride() == heads && out->row_stride() == heads &&
                         (!GRAD || dy->row_stride() == heads),
                     name << ": the per-nonzero tensors should be contiguous [nnz, heads]");
    int rc;
    if (device_type == DeviceType::kHIP) {
      const TmpBuffer tmp(ctx);
      void* stream = ctx->stream()->As<ep::HipStream>()->hip_stream();
      if (GRAD)
        rc = ofx_edge_softmax_csr_heads_grad(stream, idx_dt, val_dt, m, heads, nnz,
                                             row_ptr->dptr(), a->dptr(), dy->dptr(),
                                             out->mut_dptr(), 0, m, tmp.ptr, tmp.bytes, nullptr);
      else
        rc = ofx_edge_softmax_csr_heads(stream, idx_dt, val_dt, m, heads, nnz, row_ptr->dptr(),
                                        a->dptr(), out->mut_dptr(), 0, m, tmp.ptr, tmp.bytes, nullptr);
    } else {
      const int threads = ctx->stream()->As<ep::CpuStream>()->num_threads();
      if (GRAD)
        rc = ofx_edge_softmax_csr_heads_grad_cpu(threads, idx_dt, val_dt, m, heads, nnz,
                                                 row_ptr->dptr(), a->dptr(), dy->dptr(),
                                                 out->mut_dptr(), 0, m, nullptr);
      else
        rc = ofx_edge_softmax_csr_heads_cpu(threads, idx_dt, val_dt, m, heads, nnz,
                                            row_ptr->dptr(), a->dptr(), out->mut_dptr(), 0, m,
                                            nullptr);
    }
    OFX_KERNEL_CHECK(rc == OFX_OK, name << " kernel failed (" << rc << "): " << ofx_last_error());
  }
};

template <bool GRAD>
size_t InferEdgeSoftmaxHeadsTmpSize(user_op::InferSizeContext* ctx) {
  const user_op::TensorDesc& row_ptr = ctx->InputTensorDesc("a_csr_row_ptr", 0);
  const user_op::TensorDesc& a = ctx->InputTensorDesc(GRAD ? "y" : "e", 0);
  size_t bytes = 0;
  const int rc = ofx_edge_softmax_csr_heads_workspace_size(
      DtCode(row_ptr.data_type()), DtCode(a.data_type()), row_ptr.shape().At(0) - 1,
      a.shape().At(1), a.shape().At(0), nullptr, &bytes);
  return rc == OFX_OK ? bytes : 0;
}

}  // namespace

REGISTER_CSR_KERNEL_ALL_DTYPES("edge_softmax_csr_heads", "out", "a_csr_row_ptr", DeviceType::kCPU, NoTmp,
                               EdgeSoftmaxCsrHeadsKernel<DeviceType::kCPU, false>)
REGISTER_CSR_KERNEL_ALL_DTYPES("edge_softmax_csr_heads", "out", "a_csr_row_ptr", DeviceType::kHIP, InferEdgeSoftmaxHeadsTmpSize<false>,
                               EdgeSoftmaxCsrHeadsKernel<DeviceType::kHIP, false>)
REGISTER_CSR_KERNEL_ALL_DTYPES("edge_softmax_csr_heads_grad", "dx", "a_csr_row_ptr", DeviceType::kCPU, NoTmp,
                               EdgeSoftmaxCsrHeadsKernel<DeviceType::kCPU, true>)
REGISTER_CSR_KERNEL_ALL_DTYPES("edge_softmax_csr_heads_grad", "dx", "a_csr_row_ptr", DeviceType::kHIP, InferEdgeSoftmaxHeadsTmpSize<true>,
                               EdgeSoftmaxCsrHeadsKernel<DeviceType::kHIP, true>)

}  // namespace oneflow

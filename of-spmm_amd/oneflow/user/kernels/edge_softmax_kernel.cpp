/*
 * edge_softmax_kernel.cpp — kernels of ops "edge_softmax_csr" and "edge_softmax_csr_grad" for
 * DeviceType::kCPU and DeviceType::kHIP (same registration pattern as sddmm_kernel.cpp; device
 * work through the C-ABI of include/ofx_spmm.h).
 */
#include "oneflow/core/framework/framework.h"
#include "oneflow/user/kernels/csr_kernel_util.h"
#include "ofx_spmm.h"

namespace oneflow {

namespace {

// GRAD: inputs y, dy -> dx; else input e -> out.
template <DeviceType device_type, bool GRAD>
class EdgeSoftmaxCsrKernel final : public user_op::OpKernel, public user_op::CudaGraphSupport {
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
    const int64_t nnz = a->shape_view().elem_cnt();
    const int idx_dt = DtCode(row_ptr->data_type()), val_dt = DtCode(a->data_type());
    const char* name = GRAD ? "edge_softmax_csr_grad" : "edge_softmax_csr";
    int rc;
    if (device_type == DeviceType::kHIP) {
      const TmpBuffer tmp(ctx);
      void* stream = ctx->stream()->As<ep::HipStream>()->hip_stream();
      if (GRAD)
        rc = ofx_edge_softmax_csr_grad(stream, idx_dt, val_dt, m, nnz, row_ptr->dptr(), a->dptr(),
                                       dy->dptr(), out->mut_dptr(), 0, m, tmp.ptr, tmp.bytes, nullptr);
      else
        rc = ofx_edge_softmax_csr(stream, idx_dt, val_dt, m, nnz, row_ptr->dptr(), a->dptr(),
                                  out->mut_dptr(), 0, m, tmp.ptr, tmp.bytes, nullptr);
    } else {
      const int threads = ctx->stream()->As<ep::CpuStream>()->num_threads();
      if (GRAD)
        rc = ofx_edge_softmax_csr_grad_cpu(threads, idx_dt, val_dt, m, nnz, row_ptr->dptr(),
                                           a->dptr(), dy->dptr(), out->mut_dptr(), 0, m, nullptr);
      else
        rc = ofx_edge_softmax_csr_cpu(threads, idx_dt, val_dt, m, nnz, row_ptr->dptr(), a->dptr(),
                                      out->mut_dptr(), 0, m, nullptr);
    }
    OFX_KERNEL_CHECK(rc == OFX_OK, name << " kernel failed (" << rc << "): " << ofx_last_error());
  }
};

template <bool GRAD>
size_t InferEdgeSoftmaxTmpSize(user_op::InferSizeContext* ctx) {
  const user_op::TensorDesc& row_ptr = ctx->InputTensorDesc("a_csr_row_ptr", 0);
  const user_op::TensorDesc& a = ctx->InputTensorDesc(GRAD ? "y" : "e", 0);
  size_t bytes = 0;
  const int rc = ofx_edge_softmax_csr_workspace_size(
      DtCode(row_ptr.data_type()), DtCode(a.data_type()), row_ptr.shape().At(0) - 1,
      a.shape().At(0), nullptr, &bytes);
  return rc == OFX_OK ? bytes : 0;
}

}  // namespace

REGISTER_CSR_KERNEL_ALL_DTYPES("edge_softmax_csr", "out", "a_csr_row_ptr", DeviceType::kCPU, NoTmp,
                               EdgeSoftmaxCsrKernel<DeviceType::kCPU, false>)
REGISTER_CSR_KERNEL_ALL_DTYPES("edge_softmax_csr", "out", "a_csr_row_ptr", DeviceType::kHIP, InferEdgeSoftmaxTmpSize<false>,
                               EdgeSoftmaxCsrKernel<DeviceType::kHIP, false>)
REGISTER_CSR_KERNEL_ALL_DTYPES("edge_softmax_csr_grad", "dx", "a_csr_row_ptr", DeviceType::kCPU, NoTmp,
                               EdgeSoftmaxCsrKernel<DeviceType::kCPU, true>)
REGISTER_CSR_KERNEL_ALL_DTYPES("edge_softmax_csr_grad", "dx", "a_csr_row_ptr", DeviceType::kHIP, InferEdgeSoftmaxTmpSize<true>,
                               EdgeSoftmaxCsrKernel<DeviceType::kHIP, true>)

}  // namespace oneflow

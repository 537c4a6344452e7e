/*
 * gat_softmax_heads_kernel.cpp — kernels of ops "gat_softmax_csr_heads" and
 * "gat_softmax_csr_heads_grad" for DeviceType::kCPU and DeviceType::kHIP (same registration
 * pattern as edge_softmax_kernel.cpp; device work through the C-ABI of include/ofx_spmm.h).
 */
#include "oneflow/core/framework/framework.h"
#include "oneflow/user/kernels/csr_kernel_util.h"
#include "ofx_spmm.h"

namespace oneflow {

namespace {

// GRAD: inputs s_row, s_col, y, dy -> ds [nnz, H], d_row [M, H]; else s_row, s_col -> out [nnz, H].
template <DeviceType device_type, bool GRAD>
class GatSoftmaxCsrHeadsKernel final : public user_op::OpKernel,
                                       public user_op::CudaGraphSupport {
 public:
  bool AlwaysComputeWhenAllOutputsEmpty() const override { return false; }

 private:
  using user_op::OpKernel::Compute;
  void Compute(user_op::KernelComputeContext* ctx, user_op::OpKernelState*,
               const user_op::OpKernelCache*) const override {
    const user_op::Tensor* row_ptr = ctx->Tensor4ArgNameAndIndex("a_csr_row_ptr", 0);
    const user_op::Tensor* col_idx = ctx->Tensor4ArgNameAndIndex("a_csr_col_idx", 0);
    const user_op::Tensor* s_row = ctx->Tensor4ArgNameAndIndex("s_row", 0);
    const user_op::Tensor* s_col = ctx->Tensor4ArgNameAndIndex("s_col", 0);
    const user_op::Tensor* y = GRAD ? ctx->Tensor4ArgNameAndIndex("y", 0) : nullptr;
    const user_op::Tensor* dy = GRAD ? ctx->Tensor4ArgNameAndIndex("dy", 0) : nullptr;
    user_op::Tensor* out = ctx->Tensor4ArgNameAndIndex(GRAD ? "ds" : "out", 0);
    user_op::Tensor* d_row = GRAD ? ctx->Tensor4ArgNameAndIndex("d_row", 0) : nullptr;
    const int64_t m = row_ptr->shape_view().elem_cnt() - 1;
    const int64_t k = s_col->shape_view().At(0);
    const int64_t heads = s_row->shape_view().At(1);
    const int64_t nnz = col_idx->shape_view().elem_cnt();
    const double slope = ctx->Attr<double>("negative_slope");
    const int idx_dt = DtCode(row_ptr->data_type()), val_dt = DtCode(s_row->data_type());
    const char* name = GRAD ? "gat_softmax_csr_heads_grad" : "gat_softmax_csr_heads";
    // the C-ABI takes packed [rows, H] tensors: no row stride
    OFX_KERNEL_CHECK(s_row->row_stride() == heads && s_col->row_stride() == heads &&
                         out->row_stride() == heads &&
                         (!GRAD || (y->row_stride() == heads && dy->row_stride() == heads &&
                                    d_row->row_stride() == heads)),
                     name << ": every tensor should be contiguous [rows, heads]");
    int rc;
    if (device_type == DeviceType::kHIP) {
      const TmpBuffer tmp(ctx);
      void* stream = ctx->stream()->As<ep::HipStream>()->hip_stream();
      if (GRAD)
        rc = ofx_gat_softmax_csr_heads_grad(stream, idx_dt, val_dt, m, k, heads, nnz,
                                            row_ptr->dptr(), col_idx->dptr(), s_row->dptr(),
                                            s_col->dptr(), slope, y->dptr(), dy->dptr(),
                                            out->mut_dptr(), d_row->mut_dptr(), 0, m, tmp.ptr,
                                            tmp.bytes, nullptr);
      else
        rc = ofx_gat_softmax_csr_heads(stream, idx_dt, val_dt, m, k, heads, nnz, row_ptr->dptr(),
                                       col_idx->dptr(), s_row->dptr(), s_col->dptr(), slope,
                                       out->mut_dptr(), 0, m, tmp.ptr, tmp.bytes, nullptr);
    } else {
      const int threads = ctx->stream()->As<ep::CpuStream>()->num_threads();
      if (GRAD)
        rc = ofx_gat_softmax_csr_heads_grad_cpu(threads, idx_dt, val_dt, m, k, heads, nnz,
                                                row_ptr->dptr(), col_idx->dptr(), s_row->dptr(),
                                                s_col->dptr(), slope, y->dptr(), dy->dptr(),
                                                out->mut_dptr(), d_row->mut_dptr(), 0, m, nullptr);
      else
        rc = ofx_gat_softmax_csr_heads_cpu(threads, idx_dt, val_dt, m, k, heads, nnz,
                                           row_ptr->dptr(), col_idx->dptr(), s_row->dptr(),
                                           s_col->dptr(), slope, out->mut_dptr(), 0, m, nullptr);
    }
    OFX_KERNEL_CHECK(rc == OFX_OK, name << " kernel failed (" << rc << "): " << ofx_last_error());
  }
};

size_t InferGatSoftmaxHeadsTmpSize(user_op::InferSizeContext* ctx) {
  const user_op::TensorDesc& row_ptr = ctx->InputTensorDesc("a_csr_row_ptr", 0);
  const user_op::TensorDesc& col_idx = ctx->InputTensorDesc("a_csr_col_idx", 0);
  const user_op::TensorDesc& s_col = ctx->InputTensorDesc("s_col", 0);
  size_t bytes = 0;
  const int rc = ofx_gat_softmax_csr_heads_workspace_size(
      DtCode(row_ptr.data_type()), DtCode(s_col.data_type()), row_ptr.shape().At(0) - 1,
      s_col.shape().At(0), s_col.shape().At(1), col_idx.shape().At(0), nullptr, &bytes);
  return rc == OFX_OK ? bytes : 0;
}

}  // namespace

REGISTER_CSR_KERNEL_ALL_DTYPES("gat_softmax_csr_heads", "out", "a_csr_row_ptr", DeviceType::kCPU, NoTmp,
                               GatSoftmaxCsrHeadsKernel<DeviceType::kCPU, false>)
REGISTER_CSR_KERNEL_ALL_DTYPES("gat_softmax_csr_heads", "out", "a_csr_row_ptr", DeviceType::kHIP, InferGatSoftmaxHeadsTmpSize,
                               GatSoftmaxCsrHeadsKernel<DeviceType::kHIP, false>)
REGISTER_CSR_KERNEL_ALL_DTYPES("gat_softmax_csr_heads_grad", "ds", "a_csr_row_ptr", DeviceType::kCPU, NoTmp,
                               GatSoftmaxCsrHeadsKernel<DeviceType::kCPU, true>)
REGISTER_CSR_KERNEL_ALL_DTYPES("gat_softmax_csr_heads_grad", "ds", "a_csr_row_ptr", DeviceType::kHIP, InferGatSoftmaxHeadsTmpSize,
                               GatSoftmaxCsrHeadsKernel<DeviceType::kHIP, true>)

}  // namespace oneflow

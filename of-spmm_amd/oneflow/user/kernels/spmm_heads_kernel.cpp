/*
 * spmm_heads_kernel.cpp — kernels of ops "spmm_csr_heads" and "sddmm_csr_heads" for
 * DeviceType::kCPU and DeviceType::kHIP (same registration pattern as edge_softmax_kernel.cpp;
 * device work through the C-ABI of include/ofx_spmm.h).
 */
#include "oneflow/core/framework/framework.h"
#include "oneflow/user/kernels/csr_kernel_util.h"
#include "ofx_spmm.h"

namespace oneflow {

namespace {

// SDDMM: inputs a, b -> out [nnz, H]; else inputs a_csr_values [nnz, H], b -> out [M, N].
template <DeviceType device_type, bool SDDMM>
class CsrHeadsKernel final : public user_op::OpKernel, public user_op::CudaGraphSupport {
 public:
  bool AlwaysComputeWhenAllOutputsEmpty() const override { return false; }

 private:
  using user_op::OpKernel::Compute;
  void Compute(user_op::KernelComputeContext* ctx, user_op::OpKernelState*,
               const user_op::OpKernelCache*) const override {
    const user_op::Tensor* row_ptr = ctx->Tensor4ArgNameAndIndex("a_csr_row_ptr", 0);
    const user_op::Tensor* col_idx = ctx->Tensor4ArgNameAndIndex("a_csr_col_idx", 0);
    const user_op::Tensor* x = ctx->Tensor4ArgNameAndIndex(SDDMM ? "a" : "a_csr_values", 0);
    const user_op::Tensor* b = ctx->Tensor4ArgNameAndIndex("b", 0);
    user_op::Tensor* out = ctx->Tensor4ArgNameAndIndex("out", 0);
    const int64_t m = row_ptr->shape_view().elem_cnt() - 1;
    const int64_t k = b->shape_view().At(0);
    const int64_t n = b->shape_view().At(1);
    const int64_t nnz = col_idx->shape_view().elem_cnt();
    const int64_t heads = SDDMM ? ctx->Attr<int64_t>("num_heads") : x->shape_view().At(1);
    const int64_t d = heads > 0 ? n / heads : 0;
    const int idx_dt = DtCode(row_ptr->data_type()), val_dt = DtCode(b->data_type());
    const char* name = SDDMM ? "sddmm_csr_heads" : "spmm_csr_heads";
    int rc;
    if (device_type == DeviceType::kHIP) {
      const TmpBuffer tmp(ctx);
      void* stream = ctx->stream()->As<ep::HipStream>()->hip_stream();
      if (SDDMM)
        rc = ofx_sddmm_csr_heads(stream, idx_dt, val_dt, m, k, heads, d, nnz, row_ptr->dptr(),
                                 col_idx->dptr(), x->dptr(), x->row_stride(), b->dptr(),
                                 b->row_stride(), out->mut_dptr(), 0, m, tmp.ptr, tmp.bytes);
      else
        rc = ofx_spmm_csr_heads(stream, idx_dt, val_dt, m, k, heads, d, nnz, row_ptr->dptr(),
                                col_idx->dptr(), x->dptr(), b->dptr(), b->row_stride(),
                                out->mut_dptr(), out->row_stride(), 0, m, tmp.ptr, tmp.bytes, nullptr);
    } else {
      const int threads = ctx->stream()->As<ep::CpuStream>()->num_threads();
      if (SDDMM)
        rc = ofx_sddmm_csr_heads_cpu(threads, idx_dt, val_dt, m, k, heads, d, nnz, row_ptr->dptr(),
                                     col_idx->dptr(), x->dptr(), x->row_stride(), b->dptr(),
                                     b->row_stride(), out->mut_dptr(), 0, m);
      else
        rc = ofx_spmm_csr_heads_cpu(threads, idx_dt, val_dt, m, k, heads, d, nnz, row_ptr->dptr(),
                                    col_idx->dptr(), x->dptr(), b->dptr(), b->row_stride(),
                                    out->mut_dptr(), out->row_stride(), 0, m, nullptr);
    }
    OFX_KERNEL_CHECK(rc == OFX_OK, name << " kernel failed (" << rc << "): " << ofx_last_error());
  }
};

template <bool SDDMM>
size_t InferHeadsTmpSize(user_op::InferSizeContext* ctx) {
  const user_op::TensorDesc& row_ptr = ctx->InputTensorDesc("a_csr_row_ptr", 0);
  const user_op::TensorDesc& col_idx = ctx->InputTensorDesc("a_csr_col_idx", 0);
  const user_op::TensorDesc& b = ctx->InputTensorDesc("b", 0);
  const int64_t heads = SDDMM ? ctx->Attr<int64_t>("num_heads")
                              : ctx->InputTensorDesc("a_csr_values", 0).shape().At(1);
  const int64_t d = heads > 0 ? b.shape().At(1) / heads : 0;
  const int idx_dt = DtCode(row_ptr.data_type()), val_dt = DtCode(b.data_type());
  const int64_t m = row_ptr.shape().At(0) - 1, nnz = col_idx.shape().At(0);
  size_t bytes = 0;
  const int rc =
      SDDMM ? ofx_sddmm_csr_heads_workspace_size(idx_dt, val_dt, m, heads, d, nnz, &bytes)
            : ofx_spmm_csr_heads_workspace_size(idx_dt, val_dt, m, b.shape().At(0), heads, d, nnz,
                                                nullptr, &bytes);
  return rc == OFX_OK ? bytes : 0;
}

}  // namespace

REGISTER_CSR_KERNEL_ALL_DTYPES("spmm_csr_heads", "out", "a_csr_row_ptr", DeviceType::kCPU, NoTmp,
                               CsrHeadsKernel<DeviceType::kCPU, false>)
REGISTER_CSR_KERNEL_ALL_DTYPES("spmm_csr_heads", "out", "a_csr_row_ptr", DeviceType::kHIP, InferHeadsTmpSize<false>,
                               CsrHeadsKernel<DeviceType::kHIP, false>)
REGISTER_CSR_KERNEL_ALL_DTYPES("sddmm_csr_heads", "out", "a_csr_row_ptr", DeviceType::kCPU, NoTmp,
                               CsrHeadsKernel<DeviceType::kCPU, true>)
REGISTER_CSR_KERNEL_ALL_DTYPES("sddmm_csr_heads", "out", "a_csr_row_ptr", DeviceType::kHIP, InferHeadsTmpSize<true>,
                               CsrHeadsKernel<DeviceType::kHIP, true>)

}  // namespace oneflow

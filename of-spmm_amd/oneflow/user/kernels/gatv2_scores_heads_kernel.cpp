/*
 * gatv2_scores_heads_kernel.cpp — kernels of ops "gatv2_scores_csr_heads" and
 * "gatv2_scores_csr_heads_grad" for DeviceType::kCPU and DeviceType::kHIP (same registration
 * pattern as gat_softmax_heads_kernel.cpp; device work through the C-ABI of include/ofx_spmm.h).
 */
#include "oneflow/core/framework/framework.h"
#include "oneflow/user/kernels/csr_kernel_util.h"
#include "ofx_spmm.h"

namespace oneflow {

namespace {

// GRAD: inputs x_row, x_col, att, dy -> d_x [M, N], p [M, N] or [0, N]; else -> out [nnz, H].
template <DeviceType device_type, bool GRAD>
class Gatv2ScoresCsrHeadsKernel final : public user_op::OpKernel,
                                        public user_op::CudaGraphSupport {
 public:
  bool AlwaysComputeWhenAllOutputsEmpty() const override { return false; }

 private:
  using user_op::OpKernel::Compute;
  void Compute(user_op::KernelComputeContext* ctx, user_op::OpKernelState*,
               const user_op::OpKernelCache*) const override {
    const user_op::Tensor* row_ptr = ctx->Tensor4ArgNameAndIndex("a_csr_row_ptr", 0);
    const user_op::Tensor* col_idx = ctx->Tensor4ArgNameAndIndex("a_csr_col_idx", 0);
    const user_op::Tensor* x_row = ctx->Tensor4ArgNameAndIndex("x_row", 0);
    const user_op::Tensor* x_col = ctx->Tensor4ArgNameAndIndex("x_col", 0);
    const user_op::Tensor* att = ctx->Tensor4ArgNameAndIndex("att", 0);
    const user_op::Tensor* dy = GRAD ? ctx->Tensor4ArgNameAndIndex("dy", 0) : nullptr;
    user_op::Tensor* out = ctx->Tensor4ArgNameAndIndex(GRAD ? "d_x" : "out", 0);
    user_op::Tensor* p = GRAD ? ctx->Tensor4ArgNameAndIndex("p", 0) : nullptr;
    const int64_t m = row_ptr->shape_view().elem_cnt() - 1;
    const int64_t k = x_col->shape_view().At(0);
    const int64_t n = x_col->shape_view().At(1);
    const int64_t nnz = col_idx->shape_view().elem_cnt();
    const int64_t heads = ctx->Attr<int64_t>("num_heads");
    const int64_t d = heads > 0 ? n / heads : 0;
    const double slope = ctx->Attr<double>("negative_slope");
    const int idx_dt = DtCode(row_ptr->data_type()), val_dt = DtCode(x_row->data_type());
    const char* name = GRAD ? "gatv2_scores_csr_heads_grad" : "gatv2_scores_csr_heads";
    // the C-ABI takes packed [nnz, H] tensors: no row stride
    OFX_KERNEL_CHECK(nnz == 0 || (GRAD ? dy->row_stride() == heads : out->row_stride() == heads),
                     name << ": the per-nonzero tensor should be contiguous [nnz, heads]");
    const bool with_p = GRAD && p->shape_view().elem_cnt() > 0;
    void* p_ptr = with_p ? p->mut_dptr() : nullptr;
    const int64_t ldp = with_p ? p->row_stride() : n;
    int rc;
    if (device_type == DeviceType::kHIP) {
      const TmpBuffer tmp(ctx);
      void* stream = ctx->stream()->As<ep::HipStream>()->hip_stream();
      if (GRAD)
        rc = ofx_gatv2_scores_csr_heads_grad(
            stream, idx_dt, val_dt, m, k, heads, d, nnz, row_ptr->dptr(), col_idx->dptr(),
            x_row->dptr(), x_row->row_stride(), x_col->dptr(), x_col->row_stride(), att->dptr(),
            slope, dy->dptr(), out->mut_dptr(), out->row_stride(), p_ptr, ldp, 0, m, tmp.ptr,
            tmp.bytes, nullptr);
      else
        rc = ofx_gatv2_scores_csr_heads(stream, idx_dt, val_dt, m, k, heads, d, nnz,
                                        row_ptr->dptr(), col_idx->dptr(), x_row->dptr(),
                                        x_row->row_stride(), x_col->dptr(), x_col->row_stride(),
                                        att->dptr(), slope, out->mut_dptr(), 0, m, tmp.ptr,
                                        tmp.bytes);
    } else {
      const int threads = ctx->stream()->As<ep::CpuStream>()->num_threads();
      if (GRAD)
        rc = ofx_gatv2_scores_csr_heads_grad_cpu(
            threads, idx_dt, val_dt, m, k, heads, d, nnz, row_ptr->dptr(), col_idx->dptr(),
            x_row->dptr(), x_row->row_stride(), x_col->dptr(), x_col->row_stride(), att->dptr(),
            slope, dy->dptr(), out->mut_dptr(), out->row_stride(), p_ptr, ldp, 0, m, nullptr);
      else
        rc = ofx_gatv2_scores_csr_heads_cpu(threads, idx_dt, val_dt, m, k, heads, d, nnz,
                                            row_ptr->dptr(), col_idx->dptr(), x_row->dptr(),
                                            x_row->row_stride(), x_col->dptr(),
                                            x_col->row_stride(), att->dptr(), slope,
                                            out->mut_dptr(), 0, m);
    }
    OFX_KERNEL_CHECK(rc == OFX_OK, name << " kernel failed (" << rc << "): " << ofx_last_error());
  }
};

template <bool GRAD>
size_t InferGatv2ScoresTmpSize(user_op::InferSizeContext* ctx) {
  const user_op::TensorDesc& row_ptr = ctx->InputTensorDesc("a_csr_row_ptr", 0);
  const user_op::TensorDesc& col_idx = ctx->InputTensorDesc("a_csr_col_idx", 0);
  const user_op::TensorDesc& x_col = ctx->InputTensorDesc("x_col", 0);
  const int64_t heads = ctx->Attr<int64_t>("num_heads");
  const int64_t d = heads > 0 ? x_col.shape().At(1) / heads : 0;
  const int idx_dt = DtCode(row_ptr.data_type()), val_dt = DtCode(x_col.data_type());
  const int64_t m = row_ptr.shape().At(0) - 1, nnz = col_idx.shape().At(0);
  size_t bytes = 0;
  const int rc =
      GRAD ? ofx_gatv2_scores_csr_heads_grad_workspace_size(
                 idx_dt, val_dt, m, x_col.shape().At(0), heads, d, nnz,
                 ctx->Attr<int64_t>("with_att") != 0 ? 1 : 0, nullptr, &bytes)
           : ofx_gatv2_scores_csr_heads_workspace_size(idx_dt, val_dt, m, heads, d, nnz, &bytes);
  return rc == OFX_OK ? bytes : 0;
}

}  // namespace

REGISTER_CSR_KERNEL_ALL_DTYPES("gatv2_scores_csr_heads", "out", "a_csr_row_ptr", DeviceType::kCPU, NoTmp,
                               Gatv2ScoresCsrHeadsKernel<DeviceType::kCPU, false>)
REGISTER_CSR_KERNEL_ALL_DTYPES("gatv2_scores_csr_heads", "out", "a_csr_row_ptr", DeviceType::kHIP, InferGatv2ScoresTmpSize<false>,
                               Gatv2ScoresCsrHeadsKernel<DeviceType::kHIP, false>)
REGISTER_CSR_KERNEL_ALL_DTYPES("gatv2_scores_csr_heads_grad", "d_x", "a_csr_row_ptr", DeviceType::kCPU, NoTmp,
                               Gatv2ScoresCsrHeadsKernel<DeviceType::kCPU, true>)
REGISTER_CSR_KERNEL_ALL_DTYPES("gatv2_scores_csr_heads_grad", "d_x", "a_csr_row_ptr", DeviceType::kHIP, InferGatv2ScoresTmpSize<true>,
                               Gatv2ScoresCsrHeadsKernel<DeviceType::kHIP, true>)

}  // namespace oneflow

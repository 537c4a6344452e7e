/*
 * spmm_heads_fp8_kernel.cpp — kernels of op "spmm_csr_heads_fp8" for DeviceType::kCPU and
 * DeviceType::kHIP (same registration pattern as spmm_heads_kernel.cpp; device work through the
 * C-ABI of include/ofx_spmm.h).  Registered for float, float16 and bfloat16 values: the op has no
 * double kernel.
 */
#include "oneflow/core/framework/framework.h"
#include "oneflow/user/kernels/csr_kernel_util.h"
#include "ofx_spmm.h"

namespace oneflow {

namespace {

template <DeviceType device_type>
class SpmmCsrHeadsFp8Kernel final : public user_op::OpKernel, public user_op::CudaGraphSupport {
 public:
  bool AlwaysComputeWhenAllOutputsEmpty() const override { return false; }

 private:
  using user_op::OpKernel::Compute;
  void Compute(user_op::KernelComputeContext* ctx, user_op::OpKernelState*,
               const user_op::OpKernelCache*) const override {
    const user_op::Tensor* row_ptr = ctx->Tensor4ArgNameAndIndex("a_csr_row_ptr", 0);
    const user_op::Tensor* col_idx = ctx->Tensor4ArgNameAndIndex("a_csr_col_idx", 0);
    const user_op::Tensor* values = ctx->Tensor4ArgNameAndIndex("a_csr_values", 0);
    const user_op::Tensor* b = ctx->Tensor4ArgNameAndIndex("b", 0);
    const user_op::Tensor* scale = ctx->Tensor4ArgNameAndIndex("b_scale", 0);  // optional
    user_op::Tensor* out = ctx->Tensor4ArgNameAndIndex("out", 0);
    const int64_t m = row_ptr->shape_view().elem_cnt() - 1;
    const int64_t k = b->shape_view().At(0);
    const int64_t n = b->shape_view().At(1);
    const int64_t nnz = col_idx->shape_view().elem_cnt();
    const int64_t heads = values->shape_view().At(1);
    const int64_t d = heads > 0 ? n / heads : 0;
    const int fmt = (int)ctx->Attr<int64_t>("b_format");
    const int idx_dt = DtCode(row_ptr->data_type()), val_dt = DtCode(values->data_type());
    const void* sptr = scale != nullptr ? scale->dptr() : nullptr;
    int rc;
    if (device_type == DeviceType::kHIP) {
      const TmpBuffer tmp(ctx);
      void* stream = ctx->stream()->As<ep::HipStream>()->hip_stream();
      rc = ofx_spmm_csr_heads_fp8(stream, idx_dt, val_dt, fmt, m, k, heads, d, nnz,
                                  row_ptr->dptr(), col_idx->dptr(), values->dptr(), b->dptr(),
                                  b->row_stride(), sptr, out->mut_dptr(), out->row_stride(), 0, m,
                                  tmp.ptr, tmp.bytes, nullptr);
    } else {
      const int threads = ctx->stream()->As<ep::CpuStream>()->num_threads();
      rc = ofx_spmm_csr_heads_fp8_cpu(threads, idx_dt, val_dt, fmt, m, k, heads, d, nnz,
                                      row_ptr->dptr(), col_idx->dptr(), values->dptr(), b->dptr(),
                                      b->row_stride(), sptr, out->mut_dptr(), out->row_stride(), 0,
                                      m, nullptr);
    }
    OFX_KERNEL_CHECK(rc == OFX_OK,
                     "spmm_csr_heads_fp8 kernel failed (" << rc << "): " << ofx_last_error());
  }
};

size_t InferHeadsFp8TmpSize(user_op::InferSizeContext* ctx) {
  const user_op::TensorDesc& row_ptr = ctx->InputTensorDesc("a_csr_row_ptr", 0);
  const user_op::TensorDesc& col_idx = ctx->InputTensorDesc("a_csr_col_idx", 0);
  const user_op::TensorDesc& values = ctx->InputTensorDesc("a_csr_values", 0);
  const user_op::TensorDesc& b = ctx->InputTensorDesc("b", 0);
  const int64_t heads = values.shape().At(1);
  const int64_t d = heads > 0 ? b.shape().At(1) / heads : 0;
  size_t bytes = 0;
  const int rc = ofx_spmm_csr_heads_fp8_workspace_size(
      DtCode(row_ptr.data_type()), DtCode(values.data_type()),
      (int)ctx->Attr<int64_t>("b_format"), row_ptr.shape().At(0) - 1, b.shape().At(0), heads, d,
      col_idx.shape().At(0), nullptr, &bytes);
  return rc == OFX_OK ? bytes : 0;
}

}  // namespace

// The three value dtypes x two index dtypes of the op.
#define REGISTER_FP8_KERNELS(device, tmp_fn)                                                   \
  REGISTER_CSR_KERNEL("spmm_csr_heads_fp8", "out", "a_csr_row_ptr", device, tmp_fn, kFloat,    \
                      kInt32, SpmmCsrHeadsFp8Kernel<device>)                                   \
  REGISTER_CSR_KERNEL("spmm_csr_heads_fp8", "out", "a_csr_row_ptr", device, tmp_fn, kFloat,    \
                      kInt64, SpmmCsrHeadsFp8Kernel<device>)                                   \
  REGISTER_CSR_KERNEL("spmm_csr_heads_fp8", "out", "a_csr_row_ptr", device, tmp_fn, kFloat16,  \
                      kInt32, SpmmCsrHeadsFp8Kernel<device>)                                   \
  REGISTER_CSR_KERNEL("spmm_csr_heads_fp8", "out", "a_csr_row_ptr", device, tmp_fn, kFloat16,  \
                      kInt64, SpmmCsrHeadsFp8Kernel<device>)                                   \
  REGISTER_CSR_KERNEL("spmm_csr_heads_fp8", "out", "a_csr_row_ptr", device, tmp_fn, kBFloat16, \
                      kInt32, SpmmCsrHeadsFp8Kernel<device>)                                   \
  REGISTER_CSR_KERNEL("spmm_csr_heads_fp8", "out", "a_csr_row_ptr", device, tmp_fn, kBFloat16, \
                      kInt64, SpmmCsrHeadsFp8Kernel<device>)

REGISTER_FP8_KERNELS(DeviceType::kCPU, NoTmp)
REGISTER_FP8_KERNELS(DeviceType::kHIP, InferHeadsFp8TmpSize)

}  // namespace oneflow

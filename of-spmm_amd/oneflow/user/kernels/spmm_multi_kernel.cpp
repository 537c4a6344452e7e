/*
 * spmm_multi_kernel.cpp — kernels of op "spmm_csr_multi" for DeviceType::kCPU and DeviceType::kHIP
 * (registration pattern of spmm_reduce_kernel.cpp; device work through the C-ABI of
 * include/ofx_spmm.h).  The row range of a row-split out comes from the OpKernelCache as
 * spmm_csr_reduce's; b is broadcast under the op's one signature, so its width is the logical one
 * and the hub schedule needs no option.
 */
#include "oneflow/core/framework/framework.h"
#include "oneflow/user/kernels/csr_kernel_util.h"
#include "ofx_spmm.h"

namespace oneflow {

namespace {

template <DeviceType device_type>
class SpmmCsrMultiKernel final : public user_op::OpKernel, public user_op::CudaGraphSupport {
 public:
  std::shared_ptr<user_op::OpKernelCache> InitOpKernelCache(
      user_op::KernelCacheContext* ctx) const override {
    return CreateCsrRowRangeCache(ctx);
  }

  bool AlwaysComputeWhenAllOutputsEmpty() const override { return false; }

 private:
  using user_op::OpKernel::Compute;
  void Compute(user_op::KernelComputeContext* ctx, user_op::OpKernelState*,
               const user_op::OpKernelCache* cache) const override {
    const user_op::Tensor* row_ptr = ctx->Tensor4ArgNameAndIndex("a_csr_row_ptr", 0);
    const user_op::Tensor* col_idx = ctx->Tensor4ArgNameAndIndex("a_csr_col_idx", 0);
    const user_op::Tensor* values = ctx->Tensor4ArgNameAndIndex("a_csr_values", 0);
    const user_op::Tensor* b = ctx->Tensor4ArgNameAndIndex("b", 0);
    user_op::Tensor* out = ctx->Tensor4ArgNameAndIndex("out", 0);
    const int64_t m = ctx->Attr<int64_t>("a_num_rows");
    const int64_t k = ctx->Attr<int64_t>("a_num_cols");
    const int mask = static_cast<int>(ctx->Attr<int64_t>("aggr_mask"));
    const double eps = ctx->Attr<double>("eps");
    const int64_t n = b->shape_view().At(1);
    const int64_t nnz = col_idx->shape_view().elem_cnt();
    OFX_KERNEL_CHECK(out->shape_view().NumAxes() == 2 &&
                         out->shape_view().At(1) == __builtin_popcount(mask) * n,
                     "out should have one block of b's columns per aggregator. ");
    OFX_KERNEL_CHECK(out->data_type() == b->data_type(), "out datatype should be equal to b. ");
    // the cache's options are sized for out's width, not b's: only its rows are taken
    const CsrRowRange rows = RowRangeOf(cache, m, out->shape_view().At(0));
    const int64_t nrows = rows.end - rows.begin;
    int64_t ldarg = 0;
    const auto arg_of = [&](const char* name, int bit) -> void* {
      if (!(mask & bit)) return nullptr;
      user_op::Tensor* arg = ctx->Tensor4ArgNameAndIndex(name, 0);
      OFX_KERNEL_CHECK(arg != nullptr && arg->shape_view().NumAxes() == 2 &&
                           arg->shape_view().At(0) == nrows && arg->shape_view().At(1) == n &&
                           arg->data_type() == row_ptr->data_type() &&
                           (ldarg == 0 || ldarg == arg->row_stride()),
                       name << " must be [" << nrows << ", " << n << "] of the index dtype");
      ldarg = arg->row_stride();
      return arg->mut_dptr();
    };
    void* arg_max = arg_of("arg_max", OFX_AGGR_MAX);
    void* arg_min = arg_of("arg_min", OFX_AGGR_MIN);
    const int idx_dt = DtCode(row_ptr->data_type()), val_dt = DtCode(values->data_type());
    int rc;
    if (device_type == DeviceType::kHIP) {
      const TmpBuffer tmp(ctx);
      rc = ofx_spmm_csr_multi(ctx->stream()->As<ep::HipStream>()->hip_stream(), idx_dt, val_dt, m,
                              k, n, nnz, row_ptr->dptr(), col_idx->dptr(), values->dptr(),
                              b->dptr(), b->row_stride(), mask, eps, out->mut_dptr(),
                              out->row_stride(), n, arg_max, arg_min, ldarg, rows.begin, rows.end,
                              tmp.ptr, tmp.bytes, nullptr);
    } else {
      rc = ofx_spmm_csr_multi_cpu(ctx->stream()->As<ep::CpuStream>()->num_threads(), idx_dt,
                                  val_dt, m, k, n, nnz, row_ptr->dptr(), col_idx->dptr(),
                                  values->dptr(), b->dptr(), b->row_stride(), mask, eps,
                                  out->mut_dptr(), out->row_stride(), n, arg_max, arg_min, ldarg,
                                  rows.begin, rows.end, nullptr);
    }
    OFX_KERNEL_CHECK(rc == OFX_OK,
                     "spmm_csr_multi kernel failed (" << rc << "): " << ofx_last_error());
  }
};

size_t InferMultiTmpSize(user_op::InferSizeContext* ctx) {
  const user_op::TensorDesc& row_ptr = ctx->InputTensorDesc("a_csr_row_ptr", 0);
  const user_op::TensorDesc& col_idx = ctx->InputTensorDesc("a_csr_col_idx", 0);
  const user_op::TensorDesc& b = ctx->InputTensorDesc("b", 0);
  size_t bytes = 0;
  const int rc = ofx_spmm_csr_multi_workspace_size(
      DtCode(row_ptr.data_type()), DtCode(b.data_type()), ctx->Attr<int64_t>("a_num_rows"),
      ctx->Attr<int64_t>("a_num_cols"), b.shape().At(1), col_idx.shape().At(0),
      static_cast<int>(ctx->Attr<int64_t>("aggr_mask")), nullptr, &bytes);
  return rc == OFX_OK ? bytes : 0;
}

}  // namespace

REGISTER_CSR_KERNEL_ALL_DTYPES("spmm_csr_multi", "out", "a_csr_row_ptr", DeviceType::kCPU, NoTmp,
                               SpmmCsrMultiKernel<DeviceType::kCPU>)
REGISTER_CSR_KERNEL_ALL_DTYPES("spmm_csr_multi", "out", "a_csr_row_ptr", DeviceType::kHIP,
                               InferMultiTmpSize, SpmmCsrMultiKernel<DeviceType::kHIP>)

}  // namespace oneflow

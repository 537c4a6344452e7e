/*
 * spmm_reduce_kernel.cpp — kernels of ops "spmm_csr_reduce", "spmm_csr_reduce_grad_b" and
 * "spmm_csr_reduce_grad_values" for DeviceType::kCPU and DeviceType::kHIP (registration pattern of
 * spmm_kernel.cpp / sddmm_kernel.cpp; device work through the C-ABI of include/ofx_spmm.h).
 *
 * The forward takes its row range from the OpKernelCache exactly as spmm_csr does
 * (unsorted_segment_sum_kernel.cpp:46-78): arg holds global nonzero indices, so a row split
 * needs no fix-up.  The hub schedule is the logical width's (numeric for sum / mean only).
 */
#include "oneflow/core/framework/framework.h"
#include "oneflow/user/kernels/csr_kernel_util.h"
#include "ofx_spmm.h"

namespace oneflow {

namespace {

template <DeviceType device_type>
class SpmmCsrReduceKernel final : public user_op::OpKernel, public user_op::CudaGraphSupport {
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
    user_op::Tensor* arg = ctx->Tensor4ArgNameAndIndex("arg", 0);
    const int64_t m = ctx->Attr<int64_t>("a_num_rows");
    const int64_t k = ctx->Attr<int64_t>("a_num_cols");
    const int reduce = static_cast<int>(ctx->Attr<int64_t>("reduce"));
    OFX_KERNEL_CHECK(out->shape_view().NumAxes() == 2, "out Numdims should be equal to 2. ");
    OFX_KERNEL_CHECK(out->data_type() == b->data_type(), "out datatype should be equal to b. ");
    const int64_t n = out->shape_view().At(1);
    const int64_t nnz = col_idx->shape_view().elem_cnt();
    const CsrRowRange rows = RowRangeOf(cache, m, out->shape_view().At(0));
    const int64_t row_begin = rows.begin, row_end = rows.end;
    const bool has_arg = reduce == OFX_REDUCE_MAX || reduce == OFX_REDUCE_MIN;
    void* arg_ptr = nullptr;
    int64_t ldarg = 0;
    if (has_arg) {
      OFX_KERNEL_CHECK(arg != nullptr && arg->shape_view().NumAxes() == 2 &&
                           arg->shape_view().At(0) == row_end - row_begin &&
                           arg->shape_view().At(1) == n &&
                           arg->data_type() == row_ptr->data_type(),
                       "arg must be [" << row_end - row_begin << ", " << n
                                       << "] of the index dtype");
      arg_ptr = arg->mut_dptr();
      ldarg = arg->row_stride();
    }
    const int idx_dt = DtCode(row_ptr->data_type()), val_dt = DtCode(values->data_type());
    int rc;
    if (device_type == DeviceType::kHIP) {
      const TmpBuffer tmp(ctx);
      rc = ofx_spmm_csr_reduce(ctx->stream()->As<ep::HipStream>()->hip_stream(), idx_dt, val_dt, m,
                               k, n, nnz, row_ptr->dptr(), col_idx->dptr(), values->dptr(),
                               b->dptr(), b->row_stride(), out->mut_dptr(), out->row_stride(),
                               arg_ptr, ldarg, row_begin, row_end, reduce,
                               tmp.ptr, tmp.bytes, &rows.opts);
    } else {
      rc = ofx_spmm_csr_reduce_cpu(ctx->stream()->As<ep::CpuStream>()->num_threads(), idx_dt,
                                   val_dt, m, k, n, nnz, row_ptr->dptr(), col_idx->dptr(),
                                   values->dptr(), b->dptr(), b->row_stride(), out->mut_dptr(),
                                   out->row_stride(), arg_ptr, ldarg, row_begin, row_end, reduce,
                                   &rows.opts);
    }
    OFX_KERNEL_CHECK(rc == OFX_OK,
                     "spmm_csr_reduce kernel failed (" << rc << "): " << ofx_last_error());
  }
};

template <DeviceType device_type>
class SpmmCsrReduceGradBKernel final : public user_op::OpKernel, public user_op::CudaGraphSupport {
 public:
  bool AlwaysComputeWhenAllOutputsEmpty() const override { return false; }

 private:
  using user_op::OpKernel::Compute;
  void Compute(user_op::KernelComputeContext* ctx, user_op::OpKernelState*,
               const user_op::OpKernelCache*) const override {
    const user_op::Tensor* rp_t = ctx->Tensor4ArgNameAndIndex("at_row_ptr", 0);
    const user_op::Tensor* ci_t = ctx->Tensor4ArgNameAndIndex("at_col_idx", 0);
    const user_op::Tensor* perm = ctx->Tensor4ArgNameAndIndex("at_perm", 0);
    const user_op::Tensor* values = ctx->Tensor4ArgNameAndIndex("a_csr_values", 0);
    const user_op::Tensor* arg = ctx->Tensor4ArgNameAndIndex("arg", 0);
    const user_op::Tensor* dy = ctx->Tensor4ArgNameAndIndex("dy", 0);
    user_op::Tensor* out = ctx->Tensor4ArgNameAndIndex("out", 0);
    const int64_t m = ctx->Attr<int64_t>("a_num_rows");
    const int64_t k = ctx->Attr<int64_t>("a_num_cols");
    const int64_t n = dy->shape_view().At(1);
    const int64_t nnz = ci_t->shape_view().elem_cnt();
    const int idx_dt = DtCode(rp_t->data_type()), val_dt = DtCode(dy->data_type());
    ofx_spmm_options opts = OFX_SPMM_OPTIONS_INIT;
    int rc;
    if (device_type == DeviceType::kHIP) {
      const TmpBuffer tmp(ctx);
      rc = ofx_spmm_csr_select(ctx->stream()->As<ep::HipStream>()->hip_stream(), idx_dt, val_dt, m,
                               k, n, nnz, rp_t->dptr(), ci_t->dptr(), perm->dptr(), values->dptr(),
                               arg->dptr(), arg->row_stride(), dy->dptr(), dy->row_stride(),
                               out->mut_dptr(), out->row_stride(), 0, k,
                               tmp.ptr, tmp.bytes, &opts);
    } else {
      rc = ofx_spmm_csr_select_cpu(ctx->stream()->As<ep::CpuStream>()->num_threads(), idx_dt,
                                   val_dt, m, k, n, nnz, rp_t->dptr(), ci_t->dptr(), perm->dptr(),
                                   values->dptr(), arg->dptr(), arg->row_stride(), dy->dptr(),
                                   dy->row_stride(), out->mut_dptr(), out->row_stride(), 0, k,
                                   &opts);
    }
    OFX_KERNEL_CHECK(rc == OFX_OK,
                     "spmm_csr_reduce_grad_b kernel failed (" << rc << "): " << ofx_last_error());
  }
};

template <DeviceType device_type>
class SpmmCsrReduceGradValuesKernel final : public user_op::OpKernel,
                                            public user_op::CudaGraphSupport {
 public:
  bool AlwaysComputeWhenAllOutputsEmpty() const override { return false; }

 private:
  using user_op::OpKernel::Compute;
  void Compute(user_op::KernelComputeContext* ctx, user_op::OpKernelState*,
               const user_op::OpKernelCache*) const override {
    const user_op::Tensor* row_ptr = ctx->Tensor4ArgNameAndIndex("a_csr_row_ptr", 0);
    const user_op::Tensor* col_idx = ctx->Tensor4ArgNameAndIndex("a_csr_col_idx", 0);
    const user_op::Tensor* arg = ctx->Tensor4ArgNameAndIndex("arg", 0);
    const user_op::Tensor* dy = ctx->Tensor4ArgNameAndIndex("dy", 0);
    const user_op::Tensor* b = ctx->Tensor4ArgNameAndIndex("b", 0);
    user_op::Tensor* out = ctx->Tensor4ArgNameAndIndex("out", 0);
    const int64_t m = ctx->Attr<int64_t>("a_num_rows");
    const int64_t k = ctx->Attr<int64_t>("a_num_cols");
    const int64_t n = b->shape_view().At(1);
    const int64_t nnz = col_idx->shape_view().elem_cnt();
    const int idx_dt = DtCode(row_ptr->data_type()), val_dt = DtCode(b->data_type());
    int rc;
    if (device_type == DeviceType::kHIP) {
      const TmpBuffer tmp(ctx);
      rc = ofx_sddmm_csr_select(ctx->stream()->As<ep::HipStream>()->hip_stream(), idx_dt, val_dt, m,
                                k, n, nnz, row_ptr->dptr(), col_idx->dptr(), arg->dptr(),
                                arg->row_stride(), dy->dptr(), dy->row_stride(), b->dptr(),
                                b->row_stride(), out->mut_dptr(), 0, m,
                                tmp.ptr, tmp.bytes);
    } else {
      rc = ofx_sddmm_csr_select_cpu(ctx->stream()->As<ep::CpuStream>()->num_threads(), idx_dt,
                                    val_dt, m, k, n, nnz, row_ptr->dptr(), col_idx->dptr(),
                                    arg->dptr(), arg->row_stride(), dy->dptr(), dy->row_stride(),
                                    b->dptr(), b->row_stride(), out->mut_dptr(), 0, m);
    }
    OFX_KERNEL_CHECK(rc == OFX_OK, "spmm_csr_reduce_grad_values kernel failed ("
                                       << rc << "): " << ofx_last_error());
  }
};

// tmp_buffer sizes from the workspace queries (the logical width fixes the forward's schedule)
size_t InferReduceTmpSize(user_op::InferSizeContext* ctx) {
  const user_op::TensorDesc& row_ptr = ctx->InputTensorDesc("a_csr_row_ptr", 0);
  const user_op::TensorDesc& col_idx = ctx->InputTensorDesc("a_csr_col_idx", 0);
  const user_op::TensorDesc& b = ctx->InputTensorDesc("b", 0);
  const ofx_spmm_options opts =
      LogicalWidthOptions(ctx->LogicalTensorDesc4ArgNameAndIndex("out", 0));
  size_t bytes = 0;
  const int rc = ofx_spmm_csr_reduce_workspace_size(
      DtCode(row_ptr.data_type()), DtCode(b.data_type()), ctx->Attr<int64_t>("a_num_rows"),
      ctx->Attr<int64_t>("a_num_cols"), b.shape().At(1), col_idx.shape().At(0),
      static_cast<int>(ctx->Attr<int64_t>("reduce")), &opts, &bytes);
  return rc == OFX_OK ? bytes : 0;
}

size_t InferGradBTmpSize(user_op::InferSizeContext* ctx) {
  const user_op::TensorDesc& rp_t = ctx->InputTensorDesc("at_row_ptr", 0);
  const user_op::TensorDesc& ci_t = ctx->InputTensorDesc("at_col_idx", 0);
  const user_op::TensorDesc& dy = ctx->InputTensorDesc("dy", 0);
  size_t bytes = 0;
  const int rc = ofx_spmm_csr_select_workspace_size(
      DtCode(rp_t.data_type()), DtCode(dy.data_type()), ctx->Attr<int64_t>("a_num_rows"),
      ctx->Attr<int64_t>("a_num_cols"), dy.shape().At(1), ci_t.shape().At(0), nullptr, &bytes);
  return rc == OFX_OK ? bytes : 0;
}

}  // namespace

REGISTER_CSR_KERNEL_ALL_DTYPES("spmm_csr_reduce", "out", "a_csr_row_ptr", DeviceType::kCPU, NoTmp,
                               SpmmCsrReduceKernel<DeviceType::kCPU>)
REGISTER_CSR_KERNEL_ALL_DTYPES("spmm_csr_reduce", "out", "a_csr_row_ptr", DeviceType::kHIP, InferReduceTmpSize,
                               SpmmCsrReduceKernel<DeviceType::kHIP>)
REGISTER_CSR_KERNEL_ALL_DTYPES("spmm_csr_reduce_grad_b", "out", "at_row_ptr", DeviceType::kCPU, NoTmp,
                               SpmmCsrReduceGradBKernel<DeviceType::kCPU>)
REGISTER_CSR_KERNEL_ALL_DTYPES("spmm_csr_reduce_grad_b", "out", "at_row_ptr", DeviceType::kHIP, InferGradBTmpSize,
                               SpmmCsrReduceGradBKernel<DeviceType::kHIP>)
REGISTER_CSR_KERNEL_ALL_DTYPES("spmm_csr_reduce_grad_values", "out", "a_csr_row_ptr", DeviceType::kCPU, NoTmp,
                               SpmmCsrReduceGradValuesKernel<DeviceType::kCPU>)
REGISTER_CSR_KERNEL_ALL_DTYPES("spmm_csr_reduce_grad_values", "out", "a_csr_row_ptr", DeviceType::kHIP, InferSddmmTmpSize,
                               SpmmCsrReduceGradValuesKernel<DeviceType::kHIP>)

}  // namespace oneflow

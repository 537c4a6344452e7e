/*
 * segment_matmul_kernel.cpp — kernels of ops "segment_matmul" and "segment_matmul_grad_w" for
 * DeviceType::kCPU and DeviceType::kHIP (registration pattern of spmm_edge_kernel.cpp; device work
 * through the C-ABI of include/ofx_spmm.h).  Three value dtypes (no double) x two index dtypes.
 */
#include "oneflow/core/framework/framework.h"
#include "oneflow/user/kernels/csr_kernel_util.h"
#include "ofx_spmm.h"

namespace oneflow {

namespace {

template <DeviceType device_type, bool GRAD_W>
class SegmentMatmulKernel final : public user_op::OpKernel, public user_op::CudaGraphSupport {
 public:
  bool AlwaysComputeWhenAllOutputsEmpty() const override { return false; }

 private:
  using user_op::OpKernel::Compute;
  void Compute(user_op::KernelComputeContext* ctx, user_op::OpKernelState*,
               const user_op::OpKernelCache*) const override {
    const user_op::Tensor* x = ctx->Tensor4ArgNameAndIndex("x", 0);
    const user_op::Tensor* other = ctx->Tensor4ArgNameAndIndex(GRAD_W ? "dy" : "w", 0);
    const user_op::Tensor* seg_ptr = ctx->Tensor4ArgNameAndIndex("seg_ptr", 0);
    const user_op::Tensor* idx = ctx->Tensor4ArgNameAndIndex("idx", 0);  // optional
    user_op::Tensor* out = ctx->Tensor4ArgNameAndIndex(GRAD_W ? "dw" : "out", 0);
    const int64_t r = x->shape_view().At(0), f_in = x->shape_view().At(1);
    const int64_t t = seg_ptr->shape_view().elem_cnt() - 1;
    const int64_t s = idx != nullptr ? idx->shape_view().elem_cnt() : r;
    const int64_t f_out = out->shape_view().At(1);
    const int idx_dt = DtCode(seg_ptr->data_type()), val_dt = DtCode(x->data_type());
    const void* idx_ptr = idx != nullptr ? idx->dptr() : nullptr;
    const bool hip = device_type == DeviceType::kHIP;
    void* stream = nullptr;
    int threads = 0;
    TmpBuffer tmp(ctx);
    if (hip)
      stream = ctx->stream()->As<ep::HipStream>()->hip_stream();
    else
      threads = ctx->stream()->As<ep::CpuStream>()->num_threads();
    int rc;
    if (GRAD_W) {
      OFX_KERNEL_CHECK(out->row_stride() == f_out, "dw should be contiguous. ");
      const int64_t parts = ctx->Attr<int64_t>("parts");
      rc = hip ? ofx_segment_matmul_grad_w(stream, idx_dt, val_dt, r, s, t, f_in, f_out, x->dptr(),
                                           x->row_stride(), other->dptr(), other->row_stride(),
                                           seg_ptr->dptr(), idx_ptr, out->mut_dptr(), parts,
                                           tmp.ptr, tmp.bytes)
               : ofx_segment_matmul_grad_w_cpu(threads, idx_dt, val_dt, r, s, t, f_in, f_out,
                                               x->dptr(), x->row_stride(), other->dptr(),
                                               other->row_stride(), seg_ptr->dptr(), idx_ptr,
                                               out->mut_dptr());
    } else {
      OFX_KERNEL_CHECK(other->row_stride() == other->shape_view().At(1),
                       "w should be contiguous. ");
      const int trans = ctx->Attr<int64_t>("trans_w") != 0 ? 1 : 0;
      rc = hip ? ofx_segment_matmul(stream, idx_dt, val_dt, r, s, t, f_in, f_out, x->dptr(),
                                    x->row_stride(), other->dptr(), trans, seg_ptr->dptr(),
                                    idx_ptr, out->mut_dptr(), out->row_stride(), tmp.ptr,
                                    tmp.bytes)
               : ofx_segment_matmul_cpu(threads, idx_dt, val_dt, r, s, t, f_in, f_out, x->dptr(),
                                        x->row_stride(), other->dptr(), trans, seg_ptr->dptr(),
                                        idx_ptr, out->mut_dptr(), out->row_stride());
    }
    OFX_KERNEL_CHECK(rc == OFX_OK, (GRAD_W ? "segment_matmul_grad_w" : "segment_matmul")
                                       << " kernel failed (" << rc << "): " << ofx_last_error());
  }
};

// The tmp buffer from the workspace queries: (r, s, t, f_in, f_out) from the input shapes alone.
template <bool GRAD_W>
size_t InferSegmentTmpSize(user_op::InferSizeContext* ctx) {
  const user_op::TensorDesc& x = ctx->InputTensorDesc("x", 0);
  const user_op::TensorDesc& seg_ptr = ctx->InputTensorDesc("seg_ptr", 0);
  const user_op::TensorDesc& other = ctx->InputTensorDesc(GRAD_W ? "dy" : "w", 0);
  const int idx_dt = DtCode(seg_ptr.data_type()), val_dt = DtCode(x.data_type());
  const int64_t r = x.shape().At(0), f_in = x.shape().At(1), t = seg_ptr.shape().At(0) - 1;
  size_t bytes = 0;
  int rc;
  if (GRAD_W) {
    const int64_t s = other.shape().At(0);
    rc = ofx_segment_matmul_grad_w_workspace_size(idx_dt, val_dt, r, s, t, f_in,
                                                  other.shape().At(1),
                                                  ctx->Attr<int64_t>("parts"), &bytes);
  } else {
    const bool trans = ctx->Attr<int64_t>("trans_w") != 0;
    const int64_t f_out = trans ? other.shape().At(0) / (t > 0 ? t : 1) : other.shape().At(1);
    rc = ofx_segment_matmul_workspace_size(idx_dt, val_dt, r, r, t, f_in, f_out, &bytes);
  }
  return rc == OFX_OK ? bytes : 0;
}

}  // namespace

#define REGISTER_SEGMENT_KERNELS(op, out, device, tmp_fn, ...)                            \
  REGISTER_CSR_KERNEL(op, out, "seg_ptr", device, tmp_fn, kFloat, kInt32, __VA_ARGS__)    \
  REGISTER_CSR_KERNEL(op, out, "seg_ptr", device, tmp_fn, kFloat, kInt64, __VA_ARGS__)    \
  REGISTER_CSR_KERNEL(op, out, "seg_ptr", device, tmp_fn, kFloat16, kInt32, __VA_ARGS__)  \
  REGISTER_CSR_KERNEL(op, out, "seg_ptr", device, tmp_fn, kFloat16, kInt64, __VA_ARGS__)  \
  REGISTER_CSR_KERNEL(op, out, "seg_ptr", device, tmp_fn, kBFloat16, kInt32, __VA_ARGS__) \
  REGISTER_CSR_KERNEL(op, out, "seg_ptr", device, tmp_fn, kBFloat16, kInt64, __VA_ARGS__)

REGISTER_SEGMENT_KERNELS("segment_matmul", "out", DeviceType::kCPU, NoTmp,
                         SegmentMatmulKernel<DeviceType::kCPU, false>)
REGISTER_SEGMENT_KERNELS("segment_matmul", "out", DeviceType::kHIP, InferSegmentTmpSize<false>,
                         SegmentMatmulKernel<DeviceType::kHIP, false>)
REGISTER_SEGMENT_KERNELS("segment_matmul_grad_w", "dw", DeviceType::kCPU, NoTmp,
                         SegmentMatmulKernel<DeviceType::kCPU, true>)
REGISTER_SEGMENT_KERNELS("segment_matmul_grad_w", "dw", DeviceType::kHIP,
                         InferSegmentTmpSize<true>, SegmentMatmulKernel<DeviceType::kHIP, true>)

}  // namespace oneflow

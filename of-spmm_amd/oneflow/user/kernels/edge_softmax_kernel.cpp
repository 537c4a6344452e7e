/*
 * edge_softmax_kernel.cpp — kernels of ops "edge_softmax_csr", "edge_softmax_csr_heads" and of
 * their gradients for DeviceType::kCPU and DeviceType::kHIP (same registration pattern as
 * sddmm_kernel.cpp; device work through the C-ABI of include/ofx_spmm.h).  One class for the four
 * ops: HEADS says whether the per-nonzero tensors are [nnz, H] (contiguous) or [nnz], which names
 * the messages carry and which C-ABI entries are called.
 */
#include "oneflow/core/framework/framework.h"
#include "oneflow/user/kernels/csr_kernel_util.h"
#include "ofx_spmm.h"

namespace oneflow {

namespace {

// GRAD: inputs y, dy -> dx; else input e -> out.
template <DeviceType device_type, bool HEADS, bool GRAD>
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
    const int64_t nnz = HEADS ? a->shape_view().At(0) : a->shape_view().elem_cnt();
    const int64_t heads = HEADS ? a->shape_view().At(1) : 1;
    const int idx_dt = DtCode(row_ptr->data_type()), val_dt = DtCode(a->data_type());
    const char* name = HEADS ? (GRAD ? "edge_softmax_csr_heads_grad" : "edge_softmax_csr_heads")
                             : (GRAD ? "edge_softmax_csr_grad" : "edge_softmax_csr");
    if (HEADS) {  // the C-ABI takes packed [nnz, H] tensors: no row stride
      OFX_KERNEL_CHECK(a->row_stride() == heads && out->row_stride() == heads &&
                           (!GRAD || dy->row_stride() == heads),
                       name << ": the per-nonzero tensors should be contiguous [nnz, heads]");
    }
    const void *rp = row_ptr->dptr(), *ap = a->dptr(), *gp = GRAD ? dy->dptr() : nullptr;
    void* op = out->mut_dptr();
    int rc;
    if (device_type == DeviceType::kHIP) {
      const TmpBuffer tmp(ctx);
      void* stream = ctx->stream()->As<ep::HipStream>()->hip_stream();
      if (HEADS)
        rc = GRAD ? ofx_edge_softmax_csr_heads_grad(stream, idx_dt, val_dt, m, heads, nnz, rp, ap,
                                                    gp, op, 0, m, tmp.ptr, tmp.bytes, nullptr)
                  : ofx_edge_softmax_csr_heads(stream, idx_dt, val_dt, m, heads, nnz, rp, ap, op, 0,
                                               m, tmp.ptr, tmp.bytes, nullptr);
      else
        rc = GRAD ? ofx_edge_softmax_csr_grad(stream, idx_dt, val_dt, m, nnz, rp, ap, gp, op, 0, m,
                                              tmp.ptr, tmp.bytes, nullptr)
                  : ofx_edge_softmax_csr(stream, idx_dt, val_dt, m, nnz, rp, ap, op, 0, m, tmp.ptr,
                                         tmp.bytes, nullptr);
    } else {
      const int threads = ctx->stream()->As<ep::CpuStream>()->num_threads();
      if (HEADS)
        rc = GRAD ? ofx_edge_softmax_csr_heads_grad_cpu(threads, idx_dt, val_dt, m, heads, nnz, rp,
                                                        ap, gp, op, 0, m, nullptr)
                  : ofx_edge_softmax_csr_heads_cpu(threads, idx_dt, val_dt, m, heads, nnz, rp, ap,
                                                   op, 0, m, nullptr);
      else
        rc = GRAD ? ofx_edge_softmax_csr_grad_cpu(threads, idx_dt, val_dt, m, nnz, rp, ap, gp, op,
                                                  0, m, nullptr)
                  : ofx_edge_softmax_csr_cpu(threads, idx_dt, val_dt, m, nnz, rp, ap, op, 0, m,
                                             nullptr);
    }
    OFX_KERNEL_CHECK(rc == OFX_OK, name << " kernel failed (" << rc << "): " << ofx_last_error());
  }
};

template <bool HEADS, bool GRAD>
size_t InferEdgeSoftmaxTmpSize(user_op::InferSizeContext* ctx) {
  const user_op::TensorDesc& row_ptr = ctx->InputTensorDesc("a_csr_row_ptr", 0);
  const user_op::TensorDesc& a = ctx->InputTensorDesc(GRAD ? "y" : "e", 0);
  const int idx_dt = DtCode(row_ptr.data_type()), val_dt = DtCode(a.data_type());
  const int64_t m = row_ptr.shape().At(0) - 1, nnz = a.shape().At(0);
  size_t bytes = 0;
  const int rc = HEADS ? ofx_edge_softmax_csr_heads_workspace_size(idx_dt, val_dt, m,
                                                                   a.shape().At(1), nnz, nullptr,
                                                                   &bytes)
                       : ofx_edge_softmax_csr_workspace_size(idx_dt, val_dt, m, nnz, nullptr,
                                                             &bytes);
  return rc == OFX_OK ? bytes : 0;
}

}  // namespace

#define REGISTER_EDGE_SOFTMAX_KERNELS(op, outname, HEADS, GRAD)                                  \
  REGISTER_CSR_KERNEL_ALL_DTYPES(op, outname, "a_csr_row_ptr", DeviceType::kCPU, NoTmp,          \
                                 EdgeSoftmaxCsrKernel<DeviceType::kCPU, HEADS, GRAD>)            \
  REGISTER_CSR_KERNEL_ALL_DTYPES(op, outname, "a_csr_row_ptr", DeviceType::kHIP,                 \
                                 (InferEdgeSoftmaxTmpSize<HEADS, GRAD>),                         \
                                 EdgeSoftmaxCsrKernel<DeviceType::kHIP, HEADS, GRAD>)

REGISTER_EDGE_SOFTMAX_KERNELS("edge_softmax_csr", "out", false, false)
REGISTER_EDGE_SOFTMAX_KERNELS("edge_softmax_csr_grad", "dx", false, true)
REGISTER_EDGE_SOFTMAX_KERNELS("edge_softmax_csr_heads", "out", true, false)
REGISTER_EDGE_SOFTMAX_KERNELS("edge_softmax_csr_heads_grad", "dx", true, true)

}  // namespace oneflow

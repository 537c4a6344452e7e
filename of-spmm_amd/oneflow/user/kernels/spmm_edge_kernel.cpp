/*
 * spmm_edge_kernel.cpp — kernels of ops "spmm_csr_edge", "spmm_csr_edge_grad_e" and
 * "spmm_csr_edge_grad_b" for DeviceType::kCPU and DeviceType::kHIP (same registration pattern as
 * spmm_heads_kernel.cpp; device work through the C-ABI of include/ofx_spmm.h).
 */
#include "oneflow/core/framework/framework.h"
#include "oneflow/user/kernels/csr_kernel_util.h"
#include "ofx_spmm.h"

namespace oneflow {

namespace {

enum class EdgeOp { kForward, kGradE, kGradB };

constexpr const char* EdgeOpName(EdgeOp which) {
  return which == EdgeOp::kForward ? "spmm_csr_edge"
         : which == EdgeOp::kGradE ? "spmm_csr_edge_grad_e"
                                   : "spmm_csr_edge_grad_b";
}
constexpr const char* EdgeOutName(EdgeOp which) {
  return which == EdgeOp::kForward ? "out" : which == EdgeOp::kGradE ? "de" : "db";
}

// The CSR inputs are A's (forward, d(e): M rows) or A^T's (d(b): K rows, with perm).
template <DeviceType device_type, EdgeOp WHICH>
class SpmmCsrEdgeKernel final : public user_op::OpKernel, public user_op::CudaGraphSupport {
 public:
  bool AlwaysComputeWhenAllOutputsEmpty() const override { return false; }

 private:
  using user_op::OpKernel::Compute;
  void Compute(user_op::KernelComputeContext* ctx, user_op::OpKernelState*,
               const user_op::OpKernelCache*) const override {
    const user_op::Tensor* row_ptr = ctx->Tensor4ArgNameAndIndex("a_csr_row_ptr", 0);
    const user_op::Tensor* col_idx = ctx->Tensor4ArgNameAndIndex("a_csr_col_idx", 0);
    const user_op::Tensor* e = ctx->Tensor4ArgNameAndIndex("e", 0);
    const user_op::Tensor* b = ctx->Tensor4ArgNameAndIndex("b", 0);
    user_op::Tensor* out = ctx->Tensor4ArgNameAndIndex(EdgeOutName(WHICH), 0);
    const int64_t rows = row_ptr->shape_view().elem_cnt() - 1;
    const int64_t n = b->shape_view().At(1);
    const int64_t nnz = col_idx->shape_view().elem_cnt();
    const int idx_dt = DtCode(row_ptr->data_type()), val_dt = DtCode(b->data_type());
    const int op = (int)ctx->Attr<int64_t>("op"), act = (int)ctx->Attr<int64_t>("act");
    const bool hip = device_type == DeviceType::kHIP;
    void* stream = nullptr;
    int threads = 0;
    TmpBuffer tmp(ctx);
    if (hip)
      stream = ctx->stream()->As<ep::HipStream>()->hip_stream();
    else
      threads = ctx->stream()->As<ep::CpuStream>()->num_threads();
    int rc;
    if (WHICH == EdgeOp::kForward) {
      const int64_t k = b->shape_view().At(0);
      rc = hip ? ofx_spmm_csr_edge(stream, idx_dt, val_dt, rows, k, n, nnz, row_ptr->dptr(),
                                   col_idx->dptr(), e->dptr(), b->dptr(), b->row_stride(), op, act,
                                   out->mut_dptr(), out->row_stride(), 0, rows, tmp.ptr, tmp.bytes,
                                   nullptr)
               : ofx_spmm_csr_edge_cpu(threads, idx_dt, val_dt, rows, k, n, nnz, row_ptr->dptr(),
                                       col_idx->dptr(), e->dptr(), b->dptr(), b->row_stride(), op,
                                       act, out->mut_dptr(), out->row_stride(), 0, rows, nullptr);
    } else if (WHICH == EdgeOp::kGradE) {
      const user_op::Tensor* dy = ctx->Tensor4ArgNameAndIndex("dy", 0);
      const int64_t k = b->shape_view().At(0);
      rc = hip ? ofx_spmm_csr_edge_grad_e(stream, idx_dt, val_dt, rows, k, n, nnz, row_ptr->dptr(),
                                          col_idx->dptr(), e->dptr(), b->dptr(), b->row_stride(),
                                          op, act, dy->dptr(), dy->row_stride(), out->mut_dptr(),
                                          0, rows, tmp.ptr, tmp.bytes)
               : ofx_spmm_csr_edge_grad_e_cpu(threads, idx_dt, val_dt, rows, k, n, nnz,
                                              row_ptr->dptr(), col_idx->dptr(), e->dptr(),
                                              b->dptr(), b->row_stride(), op, act, dy->dptr(),
                                              dy->row_stride(), out->mut_dptr(), 0, rows);
    } else {
      const user_op::Tensor* dy = ctx->Tensor4ArgNameAndIndex("dy", 0);
      const user_op::Tensor* perm = ctx->Tensor4ArgNameAndIndex("perm", 0);
      const int64_t m = dy->shape_view().At(0);
      rc = hip ? ofx_spmm_csr_edge_grad_b(stream, idx_dt, val_dt, m, rows, n, nnz, row_ptr->dptr(),
                                          col_idx->dptr(), perm->dptr(), e->dptr(), b->dptr(),
                                          b->row_stride(), op, act, dy->dptr(), dy->row_stride(),
                                          out->mut_dptr(), out->row_stride(), 0, rows, tmp.ptr,
                                          tmp.bytes, nullptr)
               : ofx_spmm_csr_edge_grad_b_cpu(threads, idx_dt, val_dt, m, rows, n, nnz,
                                              row_ptr->dptr(), col_idx->dptr(), perm->dptr(),
                                              e->dptr(), b->dptr(), b->row_stride(), op, act,
                                              dy->dptr(), dy->row_stride(), out->mut_dptr(),
                                              out->row_stride(), 0, rows, nullptr);
    }
    OFX_KERNEL_CHECK(rc == OFX_OK,
                     EdgeOpName(WHICH) << " kernel failed (" << rc << "): " << ofx_last_error());
  }
};

template <EdgeOp WHICH>
size_t InferEdgeTmpSize(user_op::InferSizeContext* ctx) {
  const user_op::TensorDesc& row_ptr = ctx->InputTensorDesc("a_csr_row_ptr", 0);
  const user_op::TensorDesc& col_idx = ctx->InputTensorDesc("a_csr_col_idx", 0);
  const user_op::TensorDesc& b = ctx->InputTensorDesc("b", 0);
  const int idx_dt = DtCode(row_ptr.data_type()), val_dt = DtCode(b.data_type());
  const int64_t rows = row_ptr.shape().At(0) - 1, nnz = col_idx.shape().At(0);
  const int64_t n = b.shape().At(1);
  size_t bytes = 0;
  int rc;
  if (WHICH == EdgeOp::kForward)
    rc = ofx_spmm_csr_edge_workspace_size(idx_dt, val_dt, rows, b.shape().At(0), n, nnz, nullptr,
                                          &bytes);
  else if (WHICH == EdgeOp::kGradE)  // d(e) runs over the narrow SDDMM's items
    rc = ofx_sddmm_csr_heads_workspace_size(idx_dt, val_dt, rows, 1, n, nnz, &bytes);
  else
    rc = ofx_spmm_csr_edge_grad_b_workspace_size(idx_dt, val_dt,
                                                 ctx->InputTensorDesc("dy", 0).shape().At(0), rows,
                                                 n, nnz, nullptr, &bytes);
  return rc == OFX_OK ? bytes : 0;
}

}  // namespace

#define REGISTER_EDGE_KERNELS(op, which, out)                                                   \
  REGISTER_CSR_KERNEL_ALL_DTYPES(op, out, "a_csr_row_ptr", DeviceType::kCPU, NoTmp,             \
                                 SpmmCsrEdgeKernel<DeviceType::kCPU, which>)                    \
  REGISTER_CSR_KERNEL_ALL_DTYPES(op, out, "a_csr_row_ptr", DeviceType::kHIP,                    \
                                 InferEdgeTmpSize<which>, SpmmCsrEdgeKernel<DeviceType::kHIP, which>)

REGISTER_EDGE_KERNELS("spmm_csr_edge", EdgeOp::kForward, "out")
REGISTER_EDGE_KERNELS("spmm_csr_edge_grad_e", EdgeOp::kGradE, "de")
REGISTER_EDGE_KERNELS("spmm_csr_edge_grad_b", EdgeOp::kGradB, "db")

}  // namespace oneflow

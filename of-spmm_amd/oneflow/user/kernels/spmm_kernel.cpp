/*
 * spmm_kernel.cpp — kernels of ops "spmm_csr", "fused_spmm_csr" and "spmm_csr_gathered" for
 * DeviceType::kCPU and DeviceType::kHIP: one class template over the three.
 *
 * Pattern of a OneFlow user kernel with a row-range cache (csr_kernel_util.h), following
 * oneflow/user/kernels/unsorted_segment_sum_kernel.cpp:46-78 (OpKernelCache holding
 * [lower, upper) from the out SBP, BalancedSplitter via GetTensorSliceView4ParallelId,
 * oneflow/core/job/nd_sbp_util.cpp:98-104) and :146-205 (tmp buffer via SetInferTmpSizeFn).
 * The device work is the C-ABI: ofx_spmm_csr (HIP, async on the op's stream) and
 * ofx_spmm_csr_cpu (host).  Kernel errors are fatal CHECKs as in
 * oneflow/user/kernels/matrix_vector_product_kernel.cpp:98-109.
 */
#include "oneflow/core/framework/framework.h"
#include "oneflow/core/functional/spmm_functor.h"
#include "oneflow/user/kernels/csr_kernel_util.h"
#include "oneflow/user/kernels/spmm_plan_state.h"
#include "ofx_spmm.h"

namespace oneflow {

bool SpmmCsrPlanStateStats(user_op::OpKernelState* state, int64_t* entries, int64_t* plans,
                           int64_t* hits, bool release) {
  auto* s = dynamic_cast<SpmmCsrPlanState*>(state);
  if (s == nullptr) return false;
  if (release) s->Release();
  s->Stats(entries, plans, hits);
  return true;
}

namespace {

// The static plan of an spmm_csr-family launch: key and workspace size from the launch's
// shapes, row range and schedule; the plan built by ofx_spmm_csr_plan.
void UseStaticSpmmPlan(StaticPlanLaunch* launch, SpmmCsrPlanState* plans, int64_t static_csr,
                       ep::HipStream* hs, const void* row_ptr, int idx_dt, int val_dt, int64_t m,
                       int64_t k, int64_t n, int64_t nnz, int64_t row_begin, int64_t row_end,
                       const char* op_name, ofx_spmm_options* opts) {
  if (row_end <= row_begin || n <= 0) return;
  size_t need = 0;
  const int rc = ofx_spmm_csr_workspace_size(idx_dt, val_dt, m, k, n, nnz, opts, &need);
  OFX_KERNEL_CHECK(rc == OFX_OK, op_name << " workspace query failed: " << ofx_last_error());
  void* stream = hs->hip_stream();
  const SpmmCsrPlanState::Key key{static_csr, row_ptr, plans->key_on_stream() ? stream : nullptr,
                                  hs->device_index(), idx_dt, val_dt, m, k, n, nnz, row_begin,
                                  row_end, opts->split_threshold, opts->chunk,
                                  opts->heavy_threshold, opts->range_nnz};
  launch->Use(key, need, op_name, [&](void* sws, size_t bytes) {
    return ofx_spmm_csr_plan(stream, idx_dt, val_dt, m, k, n, nnz, row_ptr, row_begin, row_end,
                             sws, bytes, opts);
  }, opts);
}

// The ops of the family: they differ in the inputs beside the CSR and b.
//   "spmm_csr": none.
//   "fused_spmm_csr": bias (optional T[N]) and attr relu, the fused epilogue (ofx_spmm_csr_fused
//     with NULL / none == ofx_spmm_csr).
//   "spmm_csr_gathered": values_perm, out = A @ b with nonzero j's value
//     a_csr_values[values_perm[j]] (the d(b) gradient with learnable values).  HIP reads the values
//     through the permutation inside the SpMM (ofx_spmm_csr_gathered); the CPU kernel gathers them
//     into its tmp buffer first and runs the kCPU SpMM on the copy (same bits).
enum class SpmmOp { kPlain, kFused, kGathered };
constexpr const char* kSpmmOpName[] = {"spmm_csr", "fused_spmm_csr", "spmm_csr_gathered"};

template <DeviceType device_type, SpmmOp op>
class SpmmCsrFamilyKernel final : public user_op::OpKernel, public user_op::CudaGraphSupport {
 public:
  SpmmCsrFamilyKernel() = default;
  ~SpmmCsrFamilyKernel() override = default;

  std::shared_ptr<user_op::OpKernelCache> InitOpKernelCache(
      user_op::KernelCacheContext* ctx) const override {
    return CreateCsrRowRangeCache(ctx);
  }

  // The plans of static CSRs (HIP only: the kCPU kernel has no work list).  The fused epilogue
  // does not change the work list; the gathered op's CSR is the autograd's cached A^T, static
  // while its cache entry lives.
  std::shared_ptr<user_op::OpKernelState> CreateOpKernelState(
      user_op::KernelInitContext* ctx) const override {
    if (device_type != DeviceType::kHIP) return nullptr;
    return std::make_shared<SpmmCsrPlanState>(!ctx->has_stream_name_hint());
  }

  bool AlwaysComputeWhenAllOutputsEmpty() const override { return false; }

 private:
  using user_op::OpKernel::Compute;
  void Compute(user_op::KernelComputeContext* ctx, user_op::OpKernelState* state,
               const user_op::OpKernelCache* cache) const override {
    const char* op_name = kSpmmOpName[static_cast<int>(op)];
    TestHookCompute(op_name);
    const user_op::Tensor* row_ptr = ctx->Tensor4ArgNameAndIndex("a_csr_row_ptr", 0);
    const user_op::Tensor* col_idx = ctx->Tensor4ArgNameAndIndex("a_csr_col_idx", 0);
    const user_op::Tensor* values = ctx->Tensor4ArgNameAndIndex("a_csr_values", 0);
    const user_op::Tensor* b = ctx->Tensor4ArgNameAndIndex("b", 0);
    user_op::Tensor* out = ctx->Tensor4ArgNameAndIndex("out", 0);
    const user_op::Tensor* bias =
        op == SpmmOp::kFused ? ctx->Tensor4ArgNameAndIndex("bias", 0) : nullptr;
    const user_op::Tensor* perm =
        op == SpmmOp::kGathered ? ctx->Tensor4ArgNameAndIndex("values_perm", 0) : nullptr;
    const int act = op == SpmmOp::kFused && ctx->Attr<bool>("relu") ? OFX_ACT_RELU : OFX_ACT_NONE;
    const int64_t m = ctx->Attr<int64_t>("a_num_rows");
    const int64_t k = ctx->Attr<int64_t>("a_num_cols");
    OFX_KERNEL_CHECK(b->shape_view().NumAxes() == 2, "b Numdims should be equal to 2. ");
    OFX_KERNEL_CHECK(out->shape_view().NumAxes() == 2, "out Numdims should be equal to 2. ");
    OFX_KERNEL_CHECK(out->data_type() == b->data_type(), "out datatype should be equal to b. ");
    const int64_t n = out->shape_view().At(1);
    const int64_t nnz = col_idx->shape_view().elem_cnt();
    CsrRowRange rows = RowRangeOf(cache, m, out->shape_view().At(0));
    if (bias != nullptr)
      OFX_KERNEL_CHECK(bias->shape_view().elem_cnt() == n && bias->data_type() == b->data_type(),
                       "bias must be [" << n << "] of b's dtype");
    const int idx_dt = DtCode(row_ptr->data_type());
    const int val_dt = DtCode(values->data_type());
    const void* bias_ptr = bias ? bias->dptr() : nullptr;
    const TmpBuffer tmp(ctx);
    int rc;
    if (device_type == DeviceType::kHIP) {
      ep::HipStream* hs = ctx->stream()->As<ep::HipStream>();
      auto* plans = dynamic_cast<SpmmCsrPlanState*>(state);
      const int64_t static_csr = ctx->Attr<int64_t>("static_csr");
      StaticPlanLaunch launch(plans, hs->IsGraphCapturing(), tmp.ptr, tmp.bytes);
      if (plans != nullptr && static_csr != 0)
        UseStaticSpmmPlan(&launch, plans, static_csr, hs, row_ptr->dptr(), idx_dt, val_dt, m, k, n,
                          nnz, rows.begin, rows.end, op_name, &rows.opts);
      if (perm != nullptr)
        rc = ofx_spmm_csr_gathered(hs->hip_stream(), idx_dt, val_dt, m, k, n, nnz, row_ptr->dptr(),
                                   col_idx->dptr(), values->dptr(), perm->dptr(), b->dptr(),
                                   b->row_stride(), out->mut_dptr(), out->row_stride(), rows.begin,
                                   rows.end, launch.ws(), launch.ws_bytes(), &rows.opts);
      else
        rc = ofx_spmm_csr_fused(hs->hip_stream(), idx_dt, val_dt, m, k, n, nnz, row_ptr->dptr(),
                                col_idx->dptr(), values->dptr(), b->dptr(), b->row_stride(),
                                out->mut_dptr(), out->row_stride(), rows.begin, rows.end, bias_ptr,
                                act, launch.ws(), launch.ws_bytes(), &rows.opts);
      launch.Launched(rc);
    } else {
      const void* vals = values->dptr();
      rc = OFX_OK;
      if (perm != nullptr) {
        const size_t vbytes = (size_t)nnz * (size_t)GetSizeOfDataType(values->data_type());
        OFX_KERNEL_CHECK(nnz == 0 || tmp.bytes >= vbytes, "tmp buffer smaller than the values");
        rc = ofx_gather_values_host(idx_dt, val_dt, nnz, perm->dptr(), vals, tmp.ptr);
        vals = tmp.ptr;
      }
      if (rc == OFX_OK)
        rc = ofx_spmm_csr_fused_cpu(ctx->stream()->As<ep::CpuStream>()->num_threads(), idx_dt,
                                    val_dt, m, k, n, nnz, row_ptr->dptr(), col_idx->dptr(), vals,
                                    b->dptr(), b->row_stride(), out->mut_dptr(), out->row_stride(),
                                    rows.begin, rows.end, bias_ptr, act, &rows.opts);
    }
    OFX_KERNEL_CHECK(rc == OFX_OK, op_name << " kernel failed (" << rc << "): " << ofx_last_error());
  }
};

template <DeviceType device_type>
using SpmmCsrKernel = SpmmCsrFamilyKernel<device_type, SpmmOp::kPlain>;
template <DeviceType device_type>
using FusedSpmmCsrKernel = SpmmCsrFamilyKernel<device_type, SpmmOp::kFused>;
template <DeviceType device_type>
using SpmmCsrGatheredKernel = SpmmCsrFamilyKernel<device_type, SpmmOp::kGathered>;

size_t InferSpmmCsrGatheredCpuTmpSize(user_op::InferSizeContext* ctx) {
  const user_op::TensorDesc& values = ctx->InputTensorDesc("a_csr_values", 0);
  return (size_t)values.shape().elem_cnt() * (size_t)GetSizeOfDataType(values.data_type());
}

// Workspace for the physical width with the logical width's schedule (as Compute launches it).
size_t InferSpmmCsrTmpSize(user_op::InferSizeContext* ctx) {
  const user_op::TensorDesc& row_ptr = ctx->InputTensorDesc("a_csr_row_ptr", 0);
  const user_op::TensorDesc& col_idx = ctx->InputTensorDesc("a_csr_col_idx", 0);
  const user_op::TensorDesc& b = ctx->InputTensorDesc("b", 0);
  const ofx_spmm_options o = LogicalWidthOptions(ctx->LogicalTensorDesc4ArgNameAndIndex("out", 0));
  size_t bytes = 0;
  const int rc = ofx_spmm_csr_workspace_size(
      DtCode(row_ptr.data_type()), DtCode(b.data_type()), ctx->Attr<int64_t>("a_num_rows"),
      ctx->Attr<int64_t>("a_num_cols"), b.shape().At(1), col_idx.shape().At(0), &o, &bytes);
  return rc == OFX_OK ? bytes : 0;
}

}  // namespace

REGISTER_CSR_KERNEL_ALL_DTYPES("spmm_csr", "out", "a_csr_row_ptr", DeviceType::kCPU, NoTmp,
                               SpmmCsrKernel<DeviceType::kCPU>)
REGISTER_CSR_KERNEL_ALL_DTYPES("spmm_csr", "out", "a_csr_row_ptr", DeviceType::kHIP, InferSpmmCsrTmpSize,
                               SpmmCsrKernel<DeviceType::kHIP>)
REGISTER_CSR_KERNEL_ALL_DTYPES("fused_spmm_csr", "out", "a_csr_row_ptr", DeviceType::kCPU, NoTmp,
                               FusedSpmmCsrKernel<DeviceType::kCPU>)
REGISTER_CSR_KERNEL_ALL_DTYPES("fused_spmm_csr", "out", "a_csr_row_ptr", DeviceType::kHIP, InferSpmmCsrTmpSize,
                               FusedSpmmCsrKernel<DeviceType::kHIP>)
REGISTER_CSR_KERNEL_ALL_DTYPES("spmm_csr_gathered", "out", "a_csr_row_ptr", DeviceType::kCPU, InferSpmmCsrGatheredCpuTmpSize,
                               SpmmCsrGatheredKernel<DeviceType::kCPU>)
REGISTER_CSR_KERNEL_ALL_DTYPES("spmm_csr_gathered", "out", "a_csr_row_ptr", DeviceType::kHIP, InferSpmmCsrTmpSize,
                               SpmmCsrGatheredKernel<DeviceType::kHIP>)

}  // namespace oneflow

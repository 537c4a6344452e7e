// csr_kernel_util.h — what the kernel files of the CSR ops share: the C-ABI's dtype code of a
// DataType, the tmp buffer of a launch, the tmp-size function of a kernel without one, the
// row-range cache of the ops whose out is split by rows, and the registration of a kernel class
// over the supported value x index dtypes.
#ifndef OFX_ONEFLOW_USER_KERNELS_CSR_KERNEL_UTIL_H_
#define OFX_ONEFLOW_USER_KERNELS_CSR_KERNEL_UTIL_H_

#include "oneflow/core/framework/framework.h"
#include "ofx_spmm.h"

namespace oneflow {

// DataType values are the OFX_DT_* codes of include/ofx_spmm.h.
inline int DtCode(DataType dt) { return static_cast<int>(dt); }

inline size_t NoTmp(user_op::InferSizeContext*) { return 0; }

// The op's "tmp_buffer" (the C-ABI's workspace): NULL and 0 bytes when the call has none.
struct TmpBuffer {
  explicit TmpBuffer(user_op::KernelComputeContext* ctx) {
    if (user_op::Tensor* tmp = ctx->Tensor4ArgNameAndIndex("tmp_buffer", 0)) {
      ptr = tmp->mut_dptr();
      bytes = (size_t)tmp->shape_view().elem_cnt();
    }
  }
  void* ptr = nullptr;
  size_t bytes = 0;
};

// Row range [lower, upper) of this rank's physical out and the logical width N ("spmm_csr" and
// its family, "spmm_csr_reduce").  The range follows unsorted_segment_sum_kernel.cpp:59-78:
// GetTensorSliceView4ParallelId over out's nd_sbp and the placement hierarchy (1-D:
// BalancedSplitter; 2-D: e.g. (S(0), S(1)) rows x columns).  The logical N fixes the hub-row
// schedule: split = default_split(N) whatever slice of the columns this rank computes, so a
// column-split rank's bits equal the single-device op's.
class CsrRowRangeCache final : public user_op::OpKernelCache {
 public:
  CsrRowRangeCache(int64_t lower, int64_t upper, int64_t logical_n)
      : lower_(lower), upper_(upper), logical_n_(logical_n) {}
  ~CsrRowRangeCache() override = default;
  int64_t lower() const { return lower_; }
  int64_t upper() const { return upper_; }
  int64_t logical_n() const { return logical_n_; }

 private:
  const int64_t lower_;
  const int64_t upper_;
  const int64_t logical_n_;
};

inline std::shared_ptr<user_op::OpKernelCache> CreateCsrRowRangeCache(
    user_op::KernelCacheContext* ctx) {
  const Shape& shape = ctx->LogicalTensorDesc4ArgNameAndIndex("out", 0)->shape();
  int64_t lower = 0, upper = shape.At(0);
  if (ctx->parallel_ctx().parallel_num() > 1) {
    const TensorSliceView view =
        GetTensorSliceView4ParallelId(*ctx->parallel_desc().hierarchy(),
                                      ctx->NdSbp4ArgNameAndIndex("out", 0), shape,
                                      ctx->parallel_ctx().parallel_id());
    lower = view.At(0).begin();
    upper = view.At(0).end();
  }
  return std::make_shared<CsrRowRangeCache>(lower, upper, shape.At(1));
}

// Options with the contract's schedule for logical width N; for the logical out of a tmp-size
// query (NULL: a local op, whose physical width is the logical one: the defaults).  Compute
// launches with the former (RowRangeOf) what the tmp-size function sized with the latter.
inline ofx_spmm_options LogicalWidthOptions(int64_t logical_n) {
  ofx_spmm_options o = OFX_SPMM_OPTIONS_INIT;
  o.split_threshold = ofx_spmm_default_split(logical_n);
  return o;
}
inline ofx_spmm_options LogicalWidthOptions(const user_op::TensorDesc* out_logical) {
  if (out_logical != nullptr) return LogicalWidthOptions(out_logical->shape().At(1));
  return OFX_SPMM_OPTIONS_INIT;
}

// A Compute's rows [begin, end) of the m-row matrix and its options, from the kernel's cache (none:
// all rows, default options); out must hold exactly those rows.
struct CsrRowRange {
  int64_t begin, end;
  ofx_spmm_options opts;
};
inline CsrRowRange RowRangeOf(const user_op::OpKernelCache* cache, int64_t m, int64_t out_rows) {
  const auto* range = dynamic_cast<const CsrRowRangeCache*>(cache);
  OFX_KERNEL_CHECK(cache == nullptr || range != nullptr, "unexpected kernel cache type");
  CsrRowRange r{0, m, OFX_SPMM_OPTIONS_INIT};
  if (range != nullptr) {
    r.begin = range->lower();
    r.end = range->upper();
    r.opts = LogicalWidthOptions(range->logical_n());
  }
  OFX_KERNEL_CHECK(out_rows == r.end - r.begin,
                   "out rows " << out_rows << " != row range " << r.end - r.begin);
  return r;
}

// The tmp buffer of an SDDMM over the op's CSR at b's width ("sddmm_csr", and d(values) of the
// max / min reductions, the masked SDDMM).
inline size_t InferSddmmTmpSize(user_op::InferSizeContext* ctx) {
  const user_op::TensorDesc& row_ptr = ctx->InputTensorDesc("a_csr_row_ptr", 0);
  const user_op::TensorDesc& col_idx = ctx->InputTensorDesc("a_csr_col_idx", 0);
  const user_op::TensorDesc& b = ctx->InputTensorDesc("b", 0);
  size_t bytes = 0;
  const int rc = ofx_sddmm_csr_workspace_size(DtCode(row_ptr.data_type()), DtCode(b.data_type()),
                                              ctx->Attr<int64_t>("a_num_rows"), b.shape().At(1),
                                              col_idx.shape().At(0), &bytes);
  return rc == OFX_OK ? bytes : 0;
}

}  // namespace oneflow

// One registration of kernel class __VA_ARGS__ for op `op` on `device`, matched on the dtype of
// output `outname` and of index input `idxname`, with tmp-size function `tmp_fn`.
#define REGISTER_CSR_KERNEL(op, outname, idxname, device, tmp_fn, dtype, itype, ...)          \
  REGISTER_USER_KERNEL(op)                                                                   \
      .SetCreateFn<__VA_ARGS__>()                                                            \
      .SetIsMatchedHob((user_op::HobDeviceType() == device)                                  \
                       && (user_op::HobDataType(outname, 0) == dtype)                        \
                       && (user_op::HobDataType(idxname, 0) == itype))                       \
      .SetInferTmpSizeFn(tmp_fn);

// The same over the four value dtypes x two index dtypes.
#define REGISTER_CSR_KERNEL_ALL_DTYPES(op, outname, idxname, device, tmp_fn, ...)             \
  REGISTER_CSR_KERNEL(op, outname, idxname, device, tmp_fn, kFloat, kInt32, __VA_ARGS__)      \
  REGISTER_CSR_KERNEL(op, outname, idxname, device, tmp_fn, kFloat, kInt64, __VA_ARGS__)      \
  REGISTER_CSR_KERNEL(op, outname, idxname, device, tmp_fn, kDouble, kInt32, __VA_ARGS__)     \
  REGISTER_CSR_KERNEL(op, outname, idxname, device, tmp_fn, kDouble, kInt64, __VA_ARGS__)     \
  REGISTER_CSR_KERNEL(op, outname, idxname, device, tmp_fn, kFloat16, kInt32, __VA_ARGS__)    \
  REGISTER_CSR_KERNEL(op, outname, idxname, device, tmp_fn, kFloat16, kInt64, __VA_ARGS__)    \
  REGISTER_CSR_KERNEL(op, outname, idxname, device, tmp_fn, kBFloat16, kInt32, __VA_ARGS__)   \
  REGISTER_CSR_KERNEL(op, outname, idxname, device, tmp_fn, kBFloat16, kInt64, __VA_ARGS__)

#endif  // OFX_ONEFLOW_USER_KERNELS_CSR_KERNEL_UTIL_H_

// csr_kernel_util.h — what the kernel files of the CSR ops share: the C-ABI's dtype code of a
// DataType, the tmp buffer of a launch, the tmp-size function of a kernel without one, and the
// registration of a kernel class over the supported value x index dtypes.
#ifndef OFX_ONEFLOW_USER_KERNELS_CSR_KERNEL_UTIL_H_
#define OFX_ONEFLOW_USER_KERNELS_CSR_KERNEL_UTIL_H_

#include "oneflow/core/framework/framework.h"

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

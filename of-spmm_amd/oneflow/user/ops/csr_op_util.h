// csr_op_util.h — what the op files of the CSR ops share: the names of the CSR inputs, the check
// of the CSR structure, the index / value dtype checks, the requires_grad=false modifier of the
// index inputs and the all-broadcast SBP signature.  Error kinds and wording as in spmm_op.cpp
// (templates oneflow/user/ops/matrix_vector_product_op.cpp:73-107,
// unsorted_segment_sum_op.cpp:21-80).
#ifndef OFX_ONEFLOW_USER_OPS_CSR_OP_UTIL_H_
#define OFX_ONEFLOW_USER_OPS_CSR_OP_UTIL_H_

#include <initializer_list>

#include "oneflow/core/framework/framework.h"

namespace oneflow {

constexpr const char* kRowPtr = "a_csr_row_ptr";
constexpr const char* kColIdx = "a_csr_col_idx";
constexpr const char* kValues = "a_csr_values";

// row_ptr 1-D with at least one element (*m = its elements - 1), col_idx 1-D (*nnz its elements).
inline Maybe<void> CheckCsrStructure(user_op::InferContext* ctx, int64_t* m, int64_t* nnz) {
  const Shape& rp = ctx->InputShape(kRowPtr, 0);
  const Shape& ci = ctx->InputShape(kColIdx, 0);
  CHECK_EQ_OR_RETURN(rp.NumAxes(), 1)
      << Error::RuntimeError() << kRowPtr << " should be 1-D, got shape " << rp.ToString();
  CHECK_GE_OR_RETURN(rp.At(0), 1)
      << Error::RuntimeError() << kRowPtr << " should have a_num_rows + 1 elements. ";
  CHECK_EQ_OR_RETURN(ci.NumAxes(), 1)
      << Error::RuntimeError() << kColIdx << " should be 1-D, got shape " << ci.ToString();
  *m = rp.At(0) - 1;
  *nnz = ci.At(0);
  return Maybe<void>::Ok();
}

// `first` is int32 or int64 and every input of `rest` has its dtype.
inline Maybe<void> CheckIndexDTypes(user_op::InferContext* ctx, const char* first = kRowPtr,
                                    std::initializer_list<const char*> rest = {kColIdx}) {
  const DataType index_dtype = ctx->InputDType(first, 0);
  CHECK_OR_RETURN(IsIndexDataType(index_dtype))
      << Error::TypeError() << first << " should be int32 or int64, got "
      << DataType_Name(index_dtype);
  for (const char* name : rest)
    CHECK_EQ_OR_RETURN(ctx->InputDType(name, 0), index_dtype)
        << Error::TypeError() << name << " should have the dtype of " << first << ". ";
  return Maybe<void>::Ok();
}

inline Maybe<void> CheckValueDType(DataType dtype, const char* op) {
  CHECK_OR_RETURN(dtype == kFloat || dtype == kDouble || dtype == kFloat16 || dtype == kBFloat16)
      << Error::TypeError() << op << " supports float, double, float16, bfloat16; got "
      << DataType_Name(dtype);
  return Maybe<void>::Ok();
}

inline Maybe<void> IndexInputsNoGrad(const user_op::GetInputArgModifier& GetInputArgModifierFn) {
  for (const char* name : {kRowPtr, kColIdx}) {
    user_op::InputArgModifier* modifier = GetInputArgModifierFn(name, 0);
    CHECK_NOTNULL_OR_RETURN(modifier);
    modifier->set_requires_grad(false);
  }
  return Maybe<void>::Ok();
}

// The one signature of an op that cannot be split: the CSR and every arg of `rest` broadcast.
inline Maybe<void> BroadcastAll(user_op::SbpContext* ctx, std::initializer_list<const char*> rest) {
  auto builder = ctx->NewBuilder();
  builder.Broadcast(user_op::OpArg(kRowPtr, 0)).Broadcast(user_op::OpArg(kColIdx, 0));
  for (const char* name : rest) builder.Broadcast(user_op::OpArg(name, 0));
  builder.Build();
  return Maybe<void>::Ok();
}

}  // namespace oneflow

#endif  // OFX_ONEFLOW_USER_OPS_CSR_OP_UTIL_H_

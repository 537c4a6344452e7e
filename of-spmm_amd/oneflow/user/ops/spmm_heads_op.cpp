/*
 * spmm_heads_op.cpp — ops "spmm_csr_heads" and "sddmm_csr_heads": the multi-head SpMM and SDDMM
 * of graph attention (GAT, graph transformers), each the other's gradient.
 *
 *   spmm_csr_heads(a_csr_row_ptr[M+1], a_csr_col_idx[nnz], a_csr_values[nnz,H], b[K,N];
 *                  a_num_rows, a_num_cols) -> out[M,N]
 *       out[r, h*D + c] = sum over the row's nonzeros j of values[j, h] * b[col[j], h*D + c]
 *   sddmm_csr_heads(a_csr_row_ptr[M+1], a_csr_col_idx[nnz], a[M,N], b[K,N]; num_heads)
 *                  -> out[nnz,H]
 *       out[j, h] = <a[row(j), h*D:(h+1)*D], b[col(j), h*D:(h+1)*D]>
 * with D = N / H; head h is columns [h*D, (h+1)*D).  Conventions and error wording of
 * sddmm_op.cpp / edge_softmax_op.cpp.
 *
 * SBP: all-broadcast only (row-split execution across ranks is not offered for these ops).
 */
#include "oneflow/core/framework/framework.h"
#include "oneflow/core/framework/op_generated.h"
#include "oneflow/user/ops/csr_op_util.h"

namespace oneflow {

// ---- spmm_csr_heads -------------------------------------------------------------------------------
/* static */ Maybe<void> SpmmCsrHeadsOp::InferLogicalTensorDesc(user_op::InferContext* ctx) {
  int64_t m = 0, nnz = 0;
  JUST(CheckCsrStructure(ctx, &m, &nnz));
  CHECK_EQ_OR_RETURN(m, ctx->Attr<int64_t>("a_num_rows"))
      << Error::RuntimeError() << kRowPtr << " should have a_num_rows + 1 elements. ";
  const int64_t k = ctx->Attr<int64_t>("a_num_cols");
  CHECK_GE_OR_RETURN(k, 0) << Error::RuntimeError() << "a_num_cols must be non-negative. ";
  const Shape& v = ctx->InputShape("a_csr_values", 0);
  const Shape& b = ctx->InputShape("b", 0);
  CHECK_EQ_OR_RETURN(v.NumAxes(), 2)
      << Error::RuntimeError() << "a_csr_values should be 2-D [nnz, heads], got shape "
      << v.ToString();
  CHECK_EQ_OR_RETURN(v.At(0), nnz)
      << Error::RuntimeError() << "a_csr_values should have nnz (as a_csr_col_idx) rows. ";
  CHECK_EQ_OR_RETURN(b.NumAxes(), 2) << Error::RuntimeError() << "b should be 2-D. ";
  CHECK_EQ_OR_RETURN(b.At(0), k) << Error::RuntimeError() << "b should have a_num_cols rows. ";
  const int64_t heads = v.At(1);
  CHECK_GE_OR_RETURN(heads, 1) << Error::RuntimeError() << "a_csr_values should have at least one head. ";
  CHECK_EQ_OR_RETURN(b.At(1) % heads, 0)
      << Error::RuntimeError() << "b's columns (" << b.At(1) << ") should be a multiple of the "
      << "number of heads (" << heads << "). ";
  ctx->SetOutputShape("out", 0, Shape({m, b.At(1)}));
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> SpmmCsrHeadsOp::InferPhysicalTensorDesc(user_op::InferContext* ctx) {
  return InferLogicalTensorDesc(ctx);
}
/* static */ Maybe<void> SpmmCsrHeadsOp::GetSbp(user_op::SbpContext* ctx) {
  return BroadcastAll(ctx, {kValues, "b", "out"});
}
/* static */ Maybe<void> SpmmCsrHeadsOp::InferDataType(user_op::InferContext* ctx) {
  JUST(CheckIndexDTypes(ctx));
  const DataType dtype = ctx->InputDType("b", 0);
  CHECK_EQ_OR_RETURN(ctx->InputDType("a_csr_values", 0), dtype)
      << Error::TypeError() << "a_csr_values datatype should be equal to b. ";
  JUST(CheckValueDType(dtype, "spmm_csr_heads"));
  ctx->SetOutputDType("out", 0, dtype);
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> SpmmCsrHeadsOp::ModifyInputArg(
    const user_op::GetInputArgModifier& GetInputArgModifierFn, const user_op::UserOpConfWrapper&) {
  return IndexInputsNoGrad(GetInputArgModifierFn);
}

// ---- sddmm_csr_heads ------------------------------------------------------------------------------
/* static */ Maybe<void> SddmmCsrHeadsOp::InferLogicalTensorDesc(user_op::InferContext* ctx) {
  int64_t m = 0, nnz = 0;
  JUST(CheckCsrStructure(ctx, &m, &nnz));
  const Shape& a = ctx->InputShape("a", 0);
  const Shape& b = ctx->InputShape("b", 0);
  CHECK_EQ_OR_RETURN(a.NumAxes(), 2) << Error::RuntimeError() << "a should be 2-D. ";
  CHECK_EQ_OR_RETURN(b.NumAxes(), 2) << Error::RuntimeError() << "b should be 2-D. ";
  CHECK_EQ_OR_RETURN(a.At(0), m) << Error::RuntimeError() << "a should have a_num_rows rows. ";
  CHECK_EQ_OR_RETURN(a.At(1), b.At(1))
      << Error::RuntimeError() << "a and b should have the same number of columns. ";
  const int64_t heads = ctx->Attr<int64_t>("num_heads");
  CHECK_GE_OR_RETURN(heads, 1) << Error::RuntimeError() << "num_heads must be positive. ";
  CHECK_EQ_OR_RETURN(b.At(1) % heads, 0)
      << Error::RuntimeError() << "b's columns (" << b.At(1) << ") should be a multiple of "
      << "num_heads (" << heads << "). ";
  ctx->SetOutputShape("out", 0, Shape({nnz, heads}));
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> SddmmCsrHeadsOp::InferPhysicalTensorDesc(user_op::InferContext* ctx) {
  return InferLogicalTensorDesc(ctx);
}
/* static */ Maybe<void> SddmmCsrHeadsOp::GetSbp(user_op::SbpContext* ctx) {
  return BroadcastAll(ctx, {"a", "b", "out"});
}
/* static */ Maybe<void> SddmmCsrHeadsOp::InferDataType(user_op::InferContext* ctx) {
  JUST(CheckIndexDTypes(ctx));
  const DataType dtype = ctx->InputDType("b", 0);
  CHECK_EQ_OR_RETURN(ctx->InputDType("a", 0), dtype)
      << Error::TypeError() << "a datatype should be equal to b. ";
  JUST(CheckValueDType(dtype, "sddmm_csr_heads"));
  ctx->SetOutputDType("out", 0, dtype);
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> SddmmCsrHeadsOp::ModifyInputArg(
    const user_op::GetInputArgModifier& GetInputArgModifierFn, const user_op::UserOpConfWrapper&) {
  return IndexInputsNoGrad(GetInputArgModifierFn);
}

}  // namespace oneflow

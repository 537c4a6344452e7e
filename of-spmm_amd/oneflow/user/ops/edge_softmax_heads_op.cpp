/*
 * edge_softmax_heads_op.cpp — op "edge_softmax_csr_heads" (the multi-head scores of a CSR's
 * nonzeros normalised over each row, every head on its own: the step between sddmm_csr_heads and
 * spmm_csr_heads of multi-head graph attention) and its gradient op.
 *
 *   edge_softmax_csr_heads(a_csr_row_ptr[M+1], a_csr_col_idx[nnz], e[nnz,H]) -> out[nnz,H]
 *   edge_softmax_csr_heads_grad(a_csr_row_ptr[M+1], a_csr_col_idx[nnz], y[nnz,H], dy[nnz,H])
 *       -> dx[nnz,H],  dx[j,h] = y[j,h] * (dy[j,h] - sum over j's row of y[:,h] * dy[:,h]).
 * The number of rows is a_csr_row_ptr's length - 1; a_csr_col_idx is taken for its shape only.
 * Every head has the bits of edge_softmax_csr(_grad) on its column.  Conventions and error wording
 * of edge_softmax_op.cpp / spmm_heads_op.cpp.
 *
 * SBP: all-broadcast only, as edge_softmax_csr: a split along nnz would cut rows.  (A split along
 * the heads would be sound, but the neighbouring ops offer none, so it would only add boxing.)
 */
#include "oneflow/core/framework/framework.h"
#include "oneflow/core/framework/op_generated.h"
#include "oneflow/user/ops/csr_op_util.h"

namespace oneflow {

namespace {

Maybe<void> CheckPerNonzeroHeads(user_op::InferContext* ctx, const char* name, int64_t nnz,
                                 int64_t* heads) {
  const Shape& s = ctx->InputShape(name, 0);
  CHECK_EQ_OR_RETURN(s.NumAxes(), 2)
      << Error::RuntimeError() << name << " should be 2-D [nnz, heads], got shape " << s.ToString();
  CHECK_EQ_OR_RETURN(s.At(0), nnz)
      << Error::RuntimeError() << name << " should have nnz (as a_csr_col_idx) rows. ";
  *heads = s.At(1);
  return Maybe<void>::Ok();
}

}  // namespace

// ---- edge_softmax_csr_heads -----------------------------------------------------------------------
/* static */ Maybe<void> EdgeSoftmaxCsrHeadsOp::InferLogicalTensorDesc(user_op::InferContext* ctx) {
  int64_t m = 0, nnz = 0, heads = 0;
  JUST(CheckCsrStructure(ctx, &m, &nnz));
  JUST(CheckPerNonzeroHeads(ctx, "e", nnz, &heads));
  ctx->SetOutputShape("out", 0, Shape({nnz, heads}));
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> EdgeSoftmaxCsrHeadsOp::InferPhysicalTensorDesc(
    user_op::InferContext* ctx) {
  return InferLogicalTensorDesc(ctx);
}
/* static */ Maybe<void> EdgeSoftmaxCsrHeadsOp::GetSbp(user_op::SbpContext* ctx) {
  // all-broadcast only: a split along nnz would cut rows
  return BroadcastAll(ctx, {"e", "out"});
}
/* static */ Maybe<void> EdgeSoftmaxCsrHeadsOp::InferDataType(user_op::InferContext* ctx) {
  JUST(CheckIndexDTypes(ctx));
  const DataType dtype = ctx->InputDType("e", 0);
  JUST(CheckValueDType(dtype, "edge_softmax_csr_heads"));
  ctx->SetOutputDType("out", 0, dtype);
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> EdgeSoftmaxCsrHeadsOp::ModifyInputArg(
    const user_op::GetInputArgModifier& GetInputArgModifierFn, const user_op::UserOpConfWrapper&) {
  return IndexInputsNoGrad(GetInputArgModifierFn);
}

// ---- edge_softmax_csr_heads_grad ------------------------------------------------------------------
/* static */ Maybe<void> EdgeSoftmaxCsrHeadsGradOp::InferLogicalTensorDesc(
    user_op::InferContext* ctx) {
  int64_t m = 0, nnz = 0, heads = 0, heads_dy = 0;
  JUST(CheckCsrStructure(ctx, &m, &nnz));
  JUST(CheckPerNonzeroHeads(ctx, "y", nnz, &heads));
  JUST(CheckPerNonzeroHeads(ctx, "dy", nnz, &heads_dy));
  CHECK_EQ_OR_RETURN(heads_dy, heads)
      << Error::RuntimeError() << "dy should have the number of heads of y (" << heads_dy << " vs "
      << heads << "). ";
  ctx->SetOutputShape("dx", 0, Shape({nnz, heads}));
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> EdgeSoftmaxCsrHeadsGradOp::InferPhysicalTensorDesc(
    user_op::InferContext* ctx) {
  return InferLogicalTensorDesc(ctx);
}
/* static */ Maybe<void> EdgeSoftmaxCsrHeadsGradOp::GetSbp(user_op::SbpContext* ctx) {
  // all-broadcast only, as the forward: the sum runs over the whole row
  return BroadcastAll(ctx, {"y", "dy", "dx"});
}
/* static */ Maybe<void> EdgeSoftmaxCsrHeadsGradOp::InferDataType(user_op::InferContext* ctx) {
  JUST(CheckIndexDTypes(ctx));
  const DataType dtype = ctx->InputDType("y", 0);
  JUST(CheckValueDType(dtype, "edge_softmax_csr_heads_grad"));
  CHECK_EQ_OR_RETURN(ctx->InputDType("dy", 0), dtype)
      << Error::TypeError() << "dy datatype should be equal to y. ";
  ctx->SetOutputDType("dx", 0, dtype);
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> EdgeSoftmaxCsrHeadsGradOp::ModifyInputArg(
    const user_op::GetInputArgModifier& GetInputArgModifierFn, const user_op::UserOpConfWrapper&) {
  return IndexInputsNoGrad(GetInputArgModifierFn);
}

}  // namespace oneflow

/*
 * edge_softmax_op.cpp — op "edge_softmax_csr" (the scores of a CSR's nonzeros normalised over each
 * row: DGL's edge_softmax, PyG's softmax(src, ptr=row_ptr)) and its gradient op.
 *
 *   edge_softmax_csr(a_csr_row_ptr[M+1], a_csr_col_idx[nnz], e[nnz]) -> out[nnz]
 *   edge_softmax_csr_grad(a_csr_row_ptr[M+1], a_csr_col_idx[nnz], y[nnz], dy[nnz]) -> dx[nnz]
 *       dx[j] = y[j] * (dy[j] - sum over j's row of y * dy), from the forward's stored y.
 * The number of rows is a_csr_row_ptr's length - 1; a_csr_col_idx is taken for its shape only
 * (the kernels do not read it).  Conventions and error wording of sddmm_op.cpp /
 * spmm_reduce_op.cpp.
 *
 * SBP: all-broadcast only.  A split along nnz would cut rows (a row's maximum and sum need all of
 * its nonzeros), and there is no other axis; row-split execution across ranks is not offered.
 */
#include "oneflow/core/framework/framework.h"
#include "oneflow/core/framework/op_generated.h"
#include "oneflow/user/ops/csr_op_util.h"

namespace oneflow {

namespace {

Maybe<void> CheckPerNonzero(user_op::InferContext* ctx, const char* name, int64_t nnz) {
  const Shape& s = ctx->InputShape(name, 0);
  CHECK_EQ_OR_RETURN(s.NumAxes(), 1)
      << Error::RuntimeError() << name << " should be 1-D, got shape " << s.ToString();
  CHECK_EQ_OR_RETURN(s.At(0), nnz)
      << Error::RuntimeError() << name << " should have nnz (as a_csr_col_idx) elements. ";
  return Maybe<void>::Ok();
}

}  // namespace

// ---- edge_softmax_csr -----------------------------------------------------------------------------
/* static */ Maybe<void> EdgeSoftmaxCsrOp::InferLogicalTensorDesc(user_op::InferContext* ctx) {
  int64_t m = 0, nnz = 0;
  JUST(CheckCsrStructure(ctx, &m, &nnz));
  JUST(CheckPerNonzero(ctx, "e", nnz));
  ctx->SetOutputShape("out", 0, Shape({nnz}));
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> EdgeSoftmaxCsrOp::InferPhysicalTensorDesc(user_op::InferContext* ctx) {
  return InferLogicalTensorDesc(ctx);
}
/* static */ Maybe<void> EdgeSoftmaxCsrOp::GetSbp(user_op::SbpContext* ctx) {
  // all-broadcast only: a split along nnz would cut rows
  return BroadcastAll(ctx, {"e", "out"});
}
/* static */ Maybe<void> EdgeSoftmaxCsrOp::InferDataType(user_op::InferContext* ctx) {
  JUST(CheckIndexDTypes(ctx));
  const DataType dtype = ctx->InputDType("e", 0);
  JUST(CheckValueDType(dtype, "edge_softmax_csr"));
  ctx->SetOutputDType("out", 0, dtype);
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> EdgeSoftmaxCsrOp::ModifyInputArg(
    const user_op::GetInputArgModifier& GetInputArgModifierFn, const user_op::UserOpConfWrapper&) {
  return IndexInputsNoGrad(GetInputArgModifierFn);
}

// ---- edge_softmax_csr_grad ------------------------------------------------------------------------
/* static */ Maybe<void> EdgeSoftmaxCsrGradOp::InferLogicalTensorDesc(user_op::InferContext* ctx) {
  int64_t m = 0, nnz = 0;
  JUST(CheckCsrStructure(ctx, &m, &nnz));
  JUST(CheckPerNonzero(ctx, "y", nnz));
  JUST(CheckPerNonzero(ctx, "dy", nnz));
  ctx->SetOutputShape("dx", 0, Shape({nnz}));
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> EdgeSoftmaxCsrGradOp::InferPhysicalTensorDesc(user_op::InferContext* ctx) {
  return InferLogicalTensorDesc(ctx);
}
/* static */ Maybe<void> EdgeSoftmaxCsrGradOp::GetSbp(user_op::SbpContext* ctx) {
  // all-broadcast only, as the forward: d_r sums over the whole row
  return BroadcastAll(ctx, {"y", "dy", "dx"});
}
/* static */ Maybe<void> EdgeSoftmaxCsrGradOp::InferDataType(user_op::InferContext* ctx) {
  JUST(CheckIndexDTypes(ctx));
  const DataType dtype = ctx->InputDType("y", 0);
  JUST(CheckValueDType(dtype, "edge_softmax_csr_grad"));
  CHECK_EQ_OR_RETURN(ctx->InputDType("dy", 0), dtype)
      << Error::TypeError() << "dy datatype should be equal to y. ";
  ctx->SetOutputDType("dx", 0, dtype);
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> EdgeSoftmaxCsrGradOp::ModifyInputArg(
    const user_op::GetInputArgModifier& GetInputArgModifierFn, const user_op::UserOpConfWrapper&) {
  return IndexInputsNoGrad(GetInputArgModifierFn);
}

}  // namespace oneflow

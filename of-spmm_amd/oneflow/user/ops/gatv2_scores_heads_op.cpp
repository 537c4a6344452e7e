/*
 * gatv2_scores_heads_op.cpp — op "gatv2_scores_csr_heads" (the attention scores of a GATv2 layer
 * over a CSR: the LeakyReLU sits between the gather and the dot product with the attention vector)
 * and its gradient op.
 *
 *   gatv2_scores_csr_heads(a_csr_row_ptr[M+1], a_csr_col_idx[nnz], x_row[M,H*D], x_col[K,H*D],
 *                          att[H*D]; num_heads, negative_slope) -> out[nnz,H]
 *       out[j, h] = sum over c of att[h*D + c] *
 *                   LeakyReLU(x_row[row(j), h*D + c] + x_col[a_csr_col_idx[j], h*D + c])
 *   gatv2_scores_csr_heads_grad(a_csr_row_ptr, a_csr_col_idx, x_row, x_col, att, dy[nnz,H];
 *                               num_heads, negative_slope, with_att) -> d_x[M,H*D], p[M,H*D]
 *       d_x = the gradient in x_row; p (with_att != 0; otherwise [0, H*D]) = the per-row terms
 *       whose column sum is the gradient in att.  (The gradient in x_col is the same op on the
 *       transposed CSR with x_row and x_col exchanged and dy gathered by the transpose's perm.)
 * The number of rows is a_csr_row_ptr's length - 1, the number of columns x_col's rows.
 * Conventions and error wording of gat_softmax_heads_op.cpp.
 *
 * SBP: all-broadcast only (a split along heads is out of scope: INTEGRATION.md §14).
 */
#include "oneflow/core/framework/framework.h"
#include "oneflow/core/framework/op_generated.h"
#include "oneflow/user/ops/csr_op_util.h"

namespace oneflow {

namespace {

// x_row [M, N], x_col [K, N], att [N] with N a multiple of num_heads: *n = N, *heads = H.
Maybe<void> CheckScoreInputs(user_op::InferContext* ctx, int64_t m, int64_t* n, int64_t* heads) {
  const Shape& xr = ctx->InputShape("x_row", 0);
  const Shape& xc = ctx->InputShape("x_col", 0);
  const Shape& att = ctx->InputShape("att", 0);
  CHECK_EQ_OR_RETURN(xr.NumAxes(), 2)
      << Error::RuntimeError() << "x_row should be 2-D [M, heads * D], got shape " << xr.ToString();
  CHECK_EQ_OR_RETURN(xc.NumAxes(), 2)
      << Error::RuntimeError() << "x_col should be 2-D [K, heads * D], got shape " << xc.ToString();
  CHECK_EQ_OR_RETURN(att.NumAxes(), 1)
      << Error::RuntimeError() << "att should be 1-D [heads * D], got shape " << att.ToString();
  CHECK_EQ_OR_RETURN(xr.At(0), m) << Error::RuntimeError() << "x_row should have a_num_rows rows. ";
  CHECK_EQ_OR_RETURN(xc.At(1), xr.At(1))
      << Error::RuntimeError() << "x_row and x_col should have the same number of columns ("
      << xr.At(1) << " vs " << xc.At(1) << "). ";
  CHECK_EQ_OR_RETURN(att.At(0), xr.At(1))
      << Error::RuntimeError() << "att should have x_row's number of columns (" << att.At(0)
      << " vs " << xr.At(1) << "). ";
  *heads = ctx->Attr<int64_t>("num_heads");
  CHECK_GE_OR_RETURN(*heads, 1) << Error::RuntimeError() << "num_heads must be positive. ";
  CHECK_EQ_OR_RETURN(xr.At(1) % *heads, 0)
      << Error::RuntimeError() << "x_row's columns (" << xr.At(1) << ") should be a multiple of "
      << "num_heads (" << *heads << "). ";
  *n = xr.At(1);
  return Maybe<void>::Ok();
}

Maybe<void> CheckValueDTypes(user_op::InferContext* ctx, const char* op,
                             std::initializer_list<const char*> rest, DataType* out) {
  JUST(CheckIndexDTypes(ctx));
  const DataType dtype = ctx->InputDType("x_row", 0);
  JUST(CheckValueDType(dtype, op));
  for (const char* name : rest)
    CHECK_EQ_OR_RETURN(ctx->InputDType(name, 0), dtype)
        << Error::TypeError() << name << " datatype should be equal to x_row. ";
  *out = dtype;
  return Maybe<void>::Ok();
}

}  // namespace

// ---- gatv2_scores_csr_heads ------------------------------------------------------------------------
/* static */ Maybe<void> Gatv2ScoresCsrHeadsOp::InferLogicalTensorDesc(user_op::InferContext* ctx) {
  int64_t m = 0, nnz = 0, n = 0, heads = 0;
  JUST(CheckCsrStructure(ctx, &m, &nnz));
  JUST(CheckScoreInputs(ctx, m, &n, &heads));
  ctx->SetOutputShape("out", 0, Shape({nnz, heads}));
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> Gatv2ScoresCsrHeadsOp::InferPhysicalTensorDesc(user_op::InferContext* ctx) {
  return InferLogicalTensorDesc(ctx);
}
/* static */ Maybe<void> Gatv2ScoresCsrHeadsOp::GetSbp(user_op::SbpContext* ctx) {
  return BroadcastAll(ctx, {"x_row", "x_col", "att", "out"});
}
/* static */ Maybe<void> Gatv2ScoresCsrHeadsOp::InferDataType(user_op::InferContext* ctx) {
  DataType dtype = kFloat;
  JUST(CheckValueDTypes(ctx, "gatv2_scores_csr_heads", {"x_col", "att"}, &dtype));
  ctx->SetOutputDType("out", 0, dtype);
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> Gatv2ScoresCsrHeadsOp::ModifyInputArg(
    const user_op::GetInputArgModifier& GetInputArgModifierFn, const user_op::UserOpConfWrapper&) {
  return IndexInputsNoGrad(GetInputArgModifierFn);
}

// ---- gatv2_scores_csr_heads_grad -------------------------------------------------------------------
/* static */ Maybe<void> Gatv2ScoresCsrHeadsGradOp::InferLogicalTensorDesc(
    user_op::InferContext* ctx) {
  int64_t m = 0, nnz = 0, n = 0, heads = 0;
  JUST(CheckCsrStructure(ctx, &m, &nnz));
  JUST(CheckScoreInputs(ctx, m, &n, &heads));
  const Shape& dy = ctx->InputShape("dy", 0);
  CHECK_EQ_OR_RETURN(dy.NumAxes(), 2)
      << Error::RuntimeError() << "dy should be 2-D [nnz, heads], got shape " << dy.ToString();
  CHECK_EQ_OR_RETURN(dy.At(0), nnz)
      << Error::RuntimeError() << "dy should have nnz (as a_csr_col_idx) rows. ";
  CHECK_EQ_OR_RETURN(dy.At(1), heads)
      << Error::RuntimeError() << "dy should have num_heads columns (" << dy.At(1) << " vs "
      << heads << "). ";
  ctx->SetOutputShape("d_x", 0, Shape({m, n}));
  ctx->SetOutputShape("p", 0, Shape({ctx->Attr<int64_t>("with_att") != 0 ? m : 0, n}));
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> Gatv2ScoresCsrHeadsGradOp::InferPhysicalTensorDesc(
    user_op::InferContext* ctx) {
  return InferLogicalTensorDesc(ctx);
}
/* static */ Maybe<void> Gatv2ScoresCsrHeadsGradOp::GetSbp(user_op::SbpContext* ctx) {
  return BroadcastAll(ctx, {"x_row", "x_col", "att", "dy", "d_x", "p"});
}
/* static */ Maybe<void> Gatv2ScoresCsrHeadsGradOp::InferDataType(user_op::InferContext* ctx) {
  DataType dtype = kFloat;
  JUST(CheckValueDTypes(ctx, "gatv2_scores_csr_heads_grad", {"x_col", "att", "dy"}, &dtype));
  ctx->SetOutputDType("d_x", 0, dtype);
  ctx->SetOutputDType("p", 0, dtype);
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> Gatv2ScoresCsrHeadsGradOp::ModifyInputArg(
    const user_op::GetInputArgModifier& GetInputArgModifierFn, const user_op::UserOpConfWrapper&) {
  return IndexInputsNoGrad(GetInputArgModifierFn);
}

}  // namespace oneflow

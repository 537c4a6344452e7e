/*
 * gat_softmax_heads_op.cpp — op "gat_softmax_csr_heads" (the attention weights of a GAT layer over
 * a CSR: additive scores, LeakyReLU and the per-row softmax, every head on its own, in one kernel)
 * and its gradient op.
 *
 *   gat_softmax_csr_heads(a_csr_row_ptr[M+1], a_csr_col_idx[nnz], s_row[M,H], s_col[K,H];
 *                         negative_slope) -> out[nnz,H]
 *       out[:, h] = edge_softmax_csr_heads(e)[:, h],
 *       e[j, h] = LeakyReLU(s_row[row(j), h] + s_col[a_csr_col_idx[j], h]) rounded to the dtype
 *   gat_softmax_csr_heads_grad(a_csr_row_ptr, a_csr_col_idx, s_row, s_col, y[nnz,H], dy[nnz,H];
 *                              negative_slope) -> ds[nnz,H], d_row[M,H]
 *       ds = edge_softmax_csr_heads_grad(y, dy) times LeakyReLU's derivative at the recomputed
 *       sum, d_row[r, h] = the sum of ds[:, h] over r's nonzeros.  (The gradient in s_col is
 *       spmm_csr_heads on the transposed CSR with values ds and b = ones [M, H].)
 * The number of rows is a_csr_row_ptr's length - 1, the number of columns s_col's rows.
 * Conventions and error wording of edge_softmax_heads_op.cpp.
 *
 * SBP: all-broadcast only, as edge_softmax_csr_heads: a split along nnz would cut rows.
 */
#include "oneflow/core/framework/framework.h"
#include "oneflow/core/framework/op_generated.h"
#include "oneflow/user/ops/csr_op_util.h"

namespace oneflow {

namespace {

// s_row [M, H] and s_col [K, H]: *heads = H.
Maybe<void> CheckScoreTerms(user_op::InferContext* ctx, int64_t m, int64_t* heads) {
  const Shape& sr = ctx->InputShape("s_row", 0);
  const Shape& sc = ctx->InputShape("s_col", 0);
  CHECK_EQ_OR_RETURN(sr.NumAxes(), 2)
      << Error::RuntimeError() << "s_row should be 2-D [M, heads], got shape " << sr.ToString();
  CHECK_EQ_OR_RETURN(sc.NumAxes(), 2)
      << Error::RuntimeError() << "s_col should be 2-D [K, heads], got shape " << sc.ToString();
  CHECK_EQ_OR_RETURN(sr.At(0), m) << Error::RuntimeError() << "s_row should have a_num_rows rows. ";
  CHECK_EQ_OR_RETURN(sc.At(1), sr.At(1))
      << Error::RuntimeError() << "s_col should have the number of heads of s_row (" << sc.At(1)
      << " vs " << sr.At(1) << "). ";
  *heads = sr.At(1);
  return Maybe<void>::Ok();
}

Maybe<void> CheckPerNonzeroHeads(user_op::InferContext* ctx, const char* name, int64_t nnz,
                                 int64_t heads) {
  const Shape& s = ctx->InputShape(name, 0);
  CHECK_EQ_OR_RETURN(s.NumAxes(), 2)
      << Error::RuntimeError() << name << " should be 2-D [nnz, heads], got shape " << s.ToString();
  CHECK_EQ_OR_RETURN(s.At(0), nnz)
      << Error::RuntimeError() << name << " should have nnz (as a_csr_col_idx) rows. ";
  CHECK_EQ_OR_RETURN(s.At(1), heads)
      << Error::RuntimeError() << name << " should have the number of heads of s_row (" << s.At(1)
      << " vs " << heads << "). ";
  return Maybe<void>::Ok();
}

Maybe<void> CheckValueDTypes(user_op::InferContext* ctx, const char* op,
                             std::initializer_list<const char*> rest, DataType* out) {
  JUST(CheckIndexDTypes(ctx));
  const DataType dtype = ctx->InputDType("s_row", 0);
  JUST(CheckValueDType(dtype, op));
  for (const char* name : rest)
    CHECK_EQ_OR_RETURN(ctx->InputDType(name, 0), dtype)
        << Error::TypeError() << name << " datatype should be equal to s_row. ";
  *out = dtype;
  return Maybe<void>::Ok();
}

}  // namespace

// ---- gat_softmax_csr_heads -------------------------------------------------------------------------
/* static */ Maybe<void> GatSoftmaxCsrHeadsOp::InferLogicalTensorDesc(user_op::InferContext* ctx) {
  int64_t m = 0, nnz = 0, heads = 0;
  JUST(CheckCsrStructure(ctx, &m, &nnz));
  JUST(CheckScoreTerms(ctx, m, &heads));
  ctx->SetOutputShape("out", 0, Shape({nnz, heads}));
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> GatSoftmaxCsrHeadsOp::InferPhysicalTensorDesc(user_op::InferContext* ctx) {
  return InferLogicalTensorDesc(ctx);
}
/* static */ Maybe<void> GatSoftmaxCsrHeadsOp::GetSbp(user_op::SbpContext* ctx) {
  // all-broadcast only: a split along nnz would cut rows
  return BroadcastAll(ctx, {"s_row", "s_col", "out"});
}
/* static */ Maybe<void> GatSoftmaxCsrHeadsOp::InferDataType(user_op::InferContext* ctx) {
  DataType dtype = kFloat;
  JUST(CheckValueDTypes(ctx, "gat_softmax_csr_heads", {"s_col"}, &dtype));
  ctx->SetOutputDType("out", 0, dtype);
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> GatSoftmaxCsrHeadsOp::ModifyInputArg(
    const user_op::GetInputArgModifier& GetInputArgModifierFn, const user_op::UserOpConfWrapper&) {
  return IndexInputsNoGrad(GetInputArgModifierFn);
}

// ---- gat_softmax_csr_heads_grad --------------------------------------------------------------------
/* static */ Maybe<void> GatSoftmaxCsrHeadsGradOp::InferLogicalTensorDesc(
    user_op::InferContext* ctx) {
  int64_t m = 0, nnz = 0, heads = 0;
  JUST(CheckCsrStructure(ctx, &m, &nnz));
  JUST(CheckScoreTerms(ctx, m, &heads));
  JUST(CheckPerNonzeroHeads(ctx, "y", nnz, heads));
  JUST(CheckPerNonzeroHeads(ctx, "dy", nnz, heads));
  ctx->SetOutputShape("ds", 0, Shape({nnz, heads}));
  ctx->SetOutputShape("d_row", 0, Shape({m, heads}));
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> GatSoftmaxCsrHeadsGradOp::InferPhysicalTensorDesc(
    user_op::InferContext* ctx) {
  return InferLogicalTensorDesc(ctx);
}
/* static */ Maybe<void> GatSoftmaxCsrHeadsGradOp::GetSbp(user_op::SbpContext* ctx) {
  // all-broadcast only, as the forward: both sums run over the whole row
  return BroadcastAll(ctx, {"s_row", "s_col", "y", "dy", "ds", "d_row"});
}
/* static */ Maybe<void> GatSoftmaxCsrHeadsGradOp::InferDataType(user_op::InferContext* ctx) {
  DataType dtype = kFloat;
  JUST(CheckValueDTypes(ctx, "gat_softmax_csr_heads_grad", {"s_col", "y", "dy"}, &dtype));
  ctx->SetOutputDType("ds", 0, dtype);
  ctx->SetOutputDType("d_row", 0, dtype);
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> GatSoftmaxCsrHeadsGradOp::ModifyInputArg(
    const user_op::GetInputArgModifier& GetInputArgModifierFn, const user_op::UserOpConfWrapper&) {
  return IndexInputsNoGrad(GetInputArgModifierFn);
}

}  // namespace oneflow

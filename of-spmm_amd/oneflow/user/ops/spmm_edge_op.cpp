/*
 * spmm_edge_op.cpp — ops "spmm_csr_edge", "spmm_csr_edge_grad_e" and "spmm_csr_edge_grad_b": the
 * SpMM over per-edge feature vectors (the message sums of GINE, CFConv, MPNN; DGL's u_add_e /
 * u_mul_e + sum) and its two gradients.
 *
 *   spmm_csr_edge(a_csr_row_ptr[M+1], a_csr_col_idx[nnz], e[nnz,N], b[K,N];
 *                 a_num_rows, a_num_cols, op, act) -> out[M,N]
 *       out[r, n] = sum over the row's nonzeros j of act(b[col[j], n] op e[j, n])
 *   spmm_csr_edge_grad_e(a_csr_row_ptr, a_csr_col_idx, e, b, dy[M,N]; op, act) -> de[nnz,N]
 *   spmm_csr_edge_grad_b(a_csr_row_ptr[K+1], a_csr_col_idx[nnz], perm[nnz], e, b, dy[M,N];
 *                        op, act) -> db[K,N]       (the CSR inputs are A^T's, of csr_transpose)
 * op: OFX_EDGE_MUL / OFX_EDGE_ADD, act: OFX_ACT_NONE / OFX_ACT_RELU (include/ofx_spmm.h).
 * Conventions and error wording of spmm_heads_op.cpp.
 *
 * SBP: all-broadcast only, as spmm_csr_heads (row-split execution across ranks is not offered).
 */
#include "oneflow/core/framework/framework.h"
#include "oneflow/core/framework/op_generated.h"
#include "oneflow/user/ops/csr_op_util.h"
#include "ofx_spmm.h"

namespace oneflow {

namespace {

// e [nnz, N] and b [., N] of one width; op and act known codes.  *n: the width.
Maybe<void> CheckEdgeOperands(user_op::InferContext* ctx, int64_t nnz, int64_t* n) {
  const Shape& e = ctx->InputShape("e", 0);
  const Shape& b = ctx->InputShape("b", 0);
  CHECK_EQ_OR_RETURN(e.NumAxes(), 2)
      << Error::RuntimeError() << "e should be 2-D [nnz, N], got shape " << e.ToString();
  CHECK_EQ_OR_RETURN(e.At(0), nnz)
      << Error::RuntimeError() << "e should have nnz (as a_csr_col_idx) rows. ";
  CHECK_EQ_OR_RETURN(b.NumAxes(), 2) << Error::RuntimeError() << "b should be 2-D. ";
  CHECK_EQ_OR_RETURN(e.At(1), b.At(1))
      << Error::RuntimeError() << "e and b should have the same number of columns. ";
  const int64_t op = ctx->Attr<int64_t>("op"), act = ctx->Attr<int64_t>("act");
  CHECK_OR_RETURN(op == OFX_EDGE_MUL || op == OFX_EDGE_ADD)
      << Error::RuntimeError() << "op should be 0 (mul) or 1 (add), got " << op;
  CHECK_OR_RETURN(act == OFX_ACT_NONE || act == OFX_ACT_RELU)
      << Error::RuntimeError() << "act should be 0 (none) or 1 (relu), got " << act;
  *n = b.At(1);
  return Maybe<void>::Ok();
}

// Every value input has b's dtype, one of the four; `out` gets it.
Maybe<void> InferEdgeDType(user_op::InferContext* ctx, const char* op,
                           std::initializer_list<const char*> inputs, const char* out) {
  const DataType dtype = ctx->InputDType("b", 0);
  for (const char* name : inputs)
    CHECK_EQ_OR_RETURN(ctx->InputDType(name, 0), dtype)
        << Error::TypeError() << name << " datatype should be equal to b. ";
  JUST(CheckValueDType(dtype, op));
  ctx->SetOutputDType(out, 0, dtype);
  return Maybe<void>::Ok();
}

}  // namespace

// ---- spmm_csr_edge --------------------------------------------------------------------------------
/* static */ Maybe<void> SpmmCsrEdgeOp::InferLogicalTensorDesc(user_op::InferContext* ctx) {
  int64_t m = 0, nnz = 0, n = 0;
  JUST(CheckCsrStructure(ctx, &m, &nnz));
  CHECK_EQ_OR_RETURN(m, ctx->Attr<int64_t>("a_num_rows"))
      << Error::RuntimeError() << kRowPtr << " should have a_num_rows + 1 elements. ";
  JUST(CheckEdgeOperands(ctx, nnz, &n));
  CHECK_EQ_OR_RETURN(ctx->InputShape("b", 0).At(0), ctx->Attr<int64_t>("a_num_cols"))
      << Error::RuntimeError() << "b should have a_num_cols rows. ";
  ctx->SetOutputShape("out", 0, Shape({m, n}));
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> SpmmCsrEdgeOp::InferPhysicalTensorDesc(user_op::InferContext* ctx) {
  return InferLogicalTensorDesc(ctx);
}
/* static */ Maybe<void> SpmmCsrEdgeOp::GetSbp(user_op::SbpContext* ctx) {
  return BroadcastAll(ctx, {"e", "b", "out"});
}
/* static */ Maybe<void> SpmmCsrEdgeOp::InferDataType(user_op::InferContext* ctx) {
  JUST(CheckIndexDTypes(ctx));
  return InferEdgeDType(ctx, "spmm_csr_edge", {"e"}, "out");
}
/* static */ Maybe<void> SpmmCsrEdgeOp::ModifyInputArg(
    const user_op::GetInputArgModifier& GetInputArgModifierFn, const user_op::UserOpConfWrapper&) {
  return IndexInputsNoGrad(GetInputArgModifierFn);
}

// ---- spmm_csr_edge_grad_e -------------------------------------------------------------------------
/* static */ Maybe<void> SpmmCsrEdgeGradEOp::InferLogicalTensorDesc(user_op::InferContext* ctx) {
  int64_t m = 0, nnz = 0, n = 0;
  JUST(CheckCsrStructure(ctx, &m, &nnz));
  JUST(CheckEdgeOperands(ctx, nnz, &n));
  const Shape& dy = ctx->InputShape("dy", 0);
  CHECK_OR_RETURN(dy.NumAxes() == 2 && dy.At(0) == m && dy.At(1) == n)
      << Error::RuntimeError() << "dy should be [a_num_rows, N], got shape " << dy.ToString();
  ctx->SetOutputShape("de", 0, Shape({nnz, n}));
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> SpmmCsrEdgeGradEOp::InferPhysicalTensorDesc(user_op::InferContext* ctx) {
  return InferLogicalTensorDesc(ctx);
}
/* static */ Maybe<void> SpmmCsrEdgeGradEOp::GetSbp(user_op::SbpContext* ctx) {
  return BroadcastAll(ctx, {"e", "b", "dy", "de"});
}
/* static */ Maybe<void> SpmmCsrEdgeGradEOp::InferDataType(user_op::InferContext* ctx) {
  JUST(CheckIndexDTypes(ctx));
  return InferEdgeDType(ctx, "spmm_csr_edge_grad_e", {"e", "dy"}, "de");
}
/* static */ Maybe<void> SpmmCsrEdgeGradEOp::ModifyInputArg(
    const user_op::GetInputArgModifier& GetInputArgModifierFn, const user_op::UserOpConfWrapper&) {
  return IndexInputsNoGrad(GetInputArgModifierFn);
}

// ---- spmm_csr_edge_grad_b -------------------------------------------------------------------------
/* static */ Maybe<void> SpmmCsrEdgeGradBOp::InferLogicalTensorDesc(user_op::InferContext* ctx) {
  int64_t k = 0, nnz = 0, n = 0;
  JUST(CheckCsrStructure(ctx, &k, &nnz));  // A^T: k rows
  JUST(CheckEdgeOperands(ctx, nnz, &n));
  const Shape& perm = ctx->InputShape("perm", 0);
  CHECK_OR_RETURN(perm.NumAxes() == 1 && perm.At(0) == nnz)
      << Error::RuntimeError() << "perm should have nnz (as a_csr_col_idx) elements. ";
  CHECK_EQ_OR_RETURN(ctx->InputShape("b", 0).At(0), k)
      << Error::RuntimeError() << "b should have as many rows as the transposed CSR. ";
  const Shape& dy = ctx->InputShape("dy", 0);
  CHECK_OR_RETURN(dy.NumAxes() == 2 && dy.At(1) == n)
      << Error::RuntimeError() << "dy should be [M, N], got shape " << dy.ToString();
  ctx->SetOutputShape("db", 0, Shape({k, n}));
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> SpmmCsrEdgeGradBOp::InferPhysicalTensorDesc(user_op::InferContext* ctx) {
  return InferLogicalTensorDesc(ctx);
}
/* static */ Maybe<void> SpmmCsrEdgeGradBOp::GetSbp(user_op::SbpContext* ctx) {
  return BroadcastAll(ctx, {"perm", "e", "b", "dy", "db"});
}
/* static */ Maybe<void> SpmmCsrEdgeGradBOp::InferDataType(user_op::InferContext* ctx) {
  JUST(CheckIndexDTypes(ctx, kRowPtr, {kColIdx, "perm"}));
  return InferEdgeDType(ctx, "spmm_csr_edge_grad_b", {"e", "dy"}, "db");
}
/* static */ Maybe<void> SpmmCsrEdgeGradBOp::ModifyInputArg(
    const user_op::GetInputArgModifier& GetInputArgModifierFn, const user_op::UserOpConfWrapper&) {
  JUST(IndexInputsNoGrad(GetInputArgModifierFn));
  user_op::InputArgModifier* modifier = GetInputArgModifierFn("perm", 0);
  CHECK_NOTNULL_OR_RETURN(modifier);
  modifier->set_requires_grad(false);
  return Maybe<void>::Ok();
}

}  // namespace oneflow

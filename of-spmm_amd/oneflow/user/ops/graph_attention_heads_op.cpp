/*
 * graph_attention_heads_op.cpp — op "graph_attention_csr_heads": dot-product graph attention over
 * a CSR for H heads of width D as one op (one fused kernel for the rows below the SpMM's hub
 * threshold; hub rows in follow-up launches of the same kernel call).
 *
 *   graph_attention_csr_heads(a_csr_row_ptr[M+1], a_csr_col_idx[nnz], q[M,N], k[K,N], v[K,N];
 *                             num_heads) -> out[M,N], attn[nnz,H]
 *       attn = edge_softmax_csr_heads(sddmm_csr_heads(q, k)),  out = spmm_csr_heads(attn, v)
 * with D = N / H; head h is columns [h*D, (h+1)*D).  Both outputs have the bits of that
 * composition.  Conventions and error wording of spmm_heads_op.cpp.
 *
 * SBP: all-broadcast only (row-split execution across ranks is not offered for this op).
 */
#include "oneflow/core/framework/framework.h"
#include "oneflow/core/framework/op_generated.h"
#include "oneflow/user/ops/csr_op_util.h"

namespace oneflow {

/* static */ Maybe<void> GraphAttentionCsrHeadsOp::InferLogicalTensorDesc(
    user_op::InferContext* ctx) {
  int64_t m = 0, nnz = 0;
  JUST(CheckCsrStructure(ctx, &m, &nnz));
  const Shape& q = ctx->InputShape("q", 0);
  const Shape& k = ctx->InputShape("k", 0);
  const Shape& v = ctx->InputShape("v", 0);
  CHECK_EQ_OR_RETURN(q.NumAxes(), 2) << Error::RuntimeError() << "q should be 2-D. ";
  CHECK_EQ_OR_RETURN(k.NumAxes(), 2) << Error::RuntimeError() << "k should be 2-D. ";
  CHECK_EQ_OR_RETURN(v.NumAxes(), 2) << Error::RuntimeError() << "v should be 2-D. ";
  CHECK_EQ_OR_RETURN(q.At(0), m) << Error::RuntimeError() << "q should have a_num_rows rows. ";
  CHECK_EQ_OR_RETURN(q.At(1), k.At(1))
      << Error::RuntimeError() << "q and k should have the same number of columns. ";
  CHECK_EQ_OR_RETURN(v.At(1), k.At(1))
      << Error::RuntimeError() << "v and k should have the same number of columns. ";
  CHECK_EQ_OR_RETURN(v.At(0), k.At(0))
      << Error::RuntimeError() << "v and k should have the same number of rows. ";
  const int64_t heads = ctx->Attr<int64_t>("num_heads");
  CHECK_GE_OR_RETURN(heads, 1) << Error::RuntimeError() << "num_heads must be positive. ";
  CHECK_EQ_OR_RETURN(k.At(1) % heads, 0)
      << Error::RuntimeError() << "k's columns (" << k.At(1) << ") should be a multiple of "
      << "num_heads (" << heads << "). ";
  ctx->SetOutputShape("out", 0, Shape({m, k.At(1)}));
  ctx->SetOutputShape("attn", 0, Shape({nnz, heads}));
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> GraphAttentionCsrHeadsOp::InferPhysicalTensorDesc(
    user_op::InferContext* ctx) {
  return InferLogicalTensorDesc(ctx);
}
/* static */ Maybe<void> GraphAttentionCsrHeadsOp::GetSbp(user_op::SbpContext* ctx) {
  return BroadcastAll(ctx, {"q", "k", "v", "out", "attn"});
}
/* static */ Maybe<void> GraphAttentionCsrHeadsOp::InferDataType(user_op::InferContext* ctx) {
  JUST(CheckIndexDTypes(ctx));
  const DataType dtype = ctx->InputDType("k", 0);
  CHECK_EQ_OR_RETURN(ctx->InputDType("q", 0), dtype)
      << Error::TypeError() << "q datatype should be equal to k. ";
  CHECK_EQ_OR_RETURN(ctx->InputDType("v", 0), dtype)
      << Error::TypeError() << "v datatype should be equal to k. ";
  JUST(CheckValueDType(dtype, "graph_attention_csr_heads"));
  ctx->SetOutputDType("out", 0, dtype);
  ctx->SetOutputDType("attn", 0, dtype);
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> GraphAttentionCsrHeadsOp::ModifyInputArg(
    const user_op::GetInputArgModifier& GetInputArgModifierFn, const user_op::UserOpConfWrapper&) {
  return IndexInputsNoGrad(GetInputArgModifierFn);
}

}  // namespace oneflow

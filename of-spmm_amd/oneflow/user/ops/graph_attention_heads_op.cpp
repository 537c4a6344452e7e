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

namespace oneflow {

namespace {

constexpr const char* kRowPtr = "a_csr_row_ptr";
constexpr const char* kColIdx = "a_csr_col_idx";

}  // namespace

/* static */ Maybe<void> GraphAttentionCsrHeadsOp::InferLogicalTensorDesc(
    user_op::InferContext* ctx) {
  const Shape& rp = ctx->InputShape(kRowPtr, 0);
  const Shape& ci = ctx->InputShape(kColIdx, 0);
  CHECK_EQ_OR_RETURN(rp.NumAxes(), 1)
      << Error::RuntimeError() << kRowPtr << " should be 1-D, got shape " << rp.ToString();
  CHECK_GE_OR_RETURN(rp.At(0), 1)
      << Error::RuntimeError() << kRowPtr << " should have a_num_rows + 1 elements. ";
  CHECK_EQ_OR_RETURN(ci.NumAxes(), 1)
      << Error::RuntimeError() << kColIdx << " should be 1-D, got shape " << ci.ToString();
  const int64_t m = rp.At(0) - 1, nnz = ci.At(0);
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
  ctx->NewBuilder()
      .Broadcast(user_op::OpArg(kRowPtr, 0))
      .Broadcast(user_op::OpArg(kColIdx, 0))
      .Broadcast(user_op::OpArg("q", 0))
      .Broadcast(user_op::OpArg("k", 0))
      .Broadcast(user_op::OpArg("v", 0))
      .Broadcast(user_op::OpArg("out", 0))
      .Broadcast(user_op::OpArg("attn", 0))
      .Build();
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> GraphAttentionCsrHeadsOp::InferDataType(user_op::InferContext* ctx) {
  const DataType index_dtype = ctx->InputDType(kRowPtr, 0);
  CHECK_OR_RETURN(IsIndexDataType(index_dtype))
      << Error::TypeError() << kRowPtr << " should be int32 or int64, got "
      << DataType_Name(index_dtype);
  CHECK_EQ_OR_RETURN(ctx->InputDType(kColIdx, 0), index_dtype)
      << Error::TypeError() << kColIdx << " should have the dtype of " << kRowPtr << ". ";
  const DataType dtype = ctx->InputDType("k", 0);
  CHECK_EQ_OR_RETURN(ctx->InputDType("q", 0), dtype)
      << Error::TypeError() << "q datatype should be equal to k. ";
  CHECK_EQ_OR_RETURN(ctx->InputDType("v", 0), dtype)
      << Error::TypeError() << "v datatype should be equal to k. ";
  CHECK_OR_RETURN(dtype == kFloat || dtype == kDouble || dtype == kFloat16 || dtype == kBFloat16)
      << Error::TypeError()
      << "graph_attention_csr_heads supports float, double, float16, bfloat16; got "
      << DataType_Name(dtype);
  ctx->SetOutputDType("out", 0, dtype);
  ctx->SetOutputDType("attn", 0, dtype);
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> GraphAttentionCsrHeadsOp::ModifyInputArg(
    const user_op::GetInputArgModifier& GetInputArgModifierFn, const user_op::UserOpConfWrapper&) {
  for (const char* name : {kRowPtr, kColIdx}) {
    user_op::InputArgModifier* modifier = GetInputArgModifierFn(name, 0);
    CHECK_NOTNULL_OR_RETURN(modifier);
    modifier->set_requires_grad(false);
  }
  return Maybe<void>::Ok();
}

}  // namespace oneflow

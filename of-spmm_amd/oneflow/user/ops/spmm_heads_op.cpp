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

namespace oneflow {

namespace {

constexpr const char* kRowPtr = "a_csr_row_ptr";
constexpr const char* kColIdx = "a_csr_col_idx";

Maybe<void> CheckStructure(user_op::InferContext* ctx, int64_t* m, int64_t* nnz) {
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

Maybe<void> CheckDTypes(user_op::InferContext* ctx, const char* other, const char* op,
                        DataType* dtype) {
  const DataType index_dtype = ctx->InputDType(kRowPtr, 0);
  CHECK_OR_RETURN(IsIndexDataType(index_dtype))
      << Error::TypeError() << kRowPtr << " should be int32 or int64, got "
      << DataType_Name(index_dtype);
  CHECK_EQ_OR_RETURN(ctx->InputDType(kColIdx, 0), index_dtype)
      << Error::TypeError() << kColIdx << " should have the dtype of " << kRowPtr << ". ";
  *dtype = ctx->InputDType("b", 0);
  CHECK_EQ_OR_RETURN(ctx->InputDType(other, 0), *dtype)
      << Error::TypeError() << other << " datatype should be equal to b. ";
  CHECK_OR_RETURN(*dtype == kFloat || *dtype == kDouble || *dtype == kFloat16 ||
                  *dtype == kBFloat16)
      << Error::TypeError() << op << " supports float, double, float16, bfloat16; got "
      << DataType_Name(*dtype);
  return Maybe<void>::Ok();
}

Maybe<void> IndexInputsNoGrad(const user_op::GetInputArgModifier& GetInputArgModifierFn) {
  for (const char* name : {kRowPtr, kColIdx}) {
    user_op::InputArgModifier* modifier = GetInputArgModifierFn(name, 0);
    CHECK_NOTNULL_OR_RETURN(modifier);
    modifier->set_requires_grad(false);
  }
  return Maybe<void>::Ok();
}

Maybe<void> BroadcastAll(user_op::SbpContext* ctx, const char* x, const char* y) {
  ctx->NewBuilder()
      .Broadcast(user_op::OpArg(kRowPtr, 0))
      .Broadcast(user_op::OpArg(kColIdx, 0))
      .Broadcast(user_op::OpArg(x, 0))
      .Broadcast(user_op::OpArg(y, 0))
      .Broadcast(user_op::OpArg("out", 0))
      .Build();
  return Maybe<void>::Ok();
}

}  // namespace

// ---- spmm_csr_heads -------------------------------------------------------------------------------
/* static */ Maybe<void> SpmmCsrHeadsOp::InferLogicalTensorDesc(user_op::InferContext* ctx) {
  int64_t m = 0, nnz = 0;
  JUST(CheckStructure(ctx, &m, &nnz));
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
  return BroadcastAll(ctx, "a_csr_values", "b");
}
/* static */ Maybe<void> SpmmCsrHeadsOp::InferDataType(user_op::InferContext* ctx) {
  DataType dtype;
  JUST(CheckDTypes(ctx, "a_csr_values", "spmm_csr_heads", &dtype));
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
  JUST(CheckStructure(ctx, &m, &nnz));
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
  return BroadcastAll(ctx, "a", "b");
}
/* static */ Maybe<void> SddmmCsrHeadsOp::InferDataType(user_op::InferContext* ctx) {
  DataType dtype;
  JUST(CheckDTypes(ctx, "a", "sddmm_csr_heads", &dtype));
  ctx->SetOutputDType("out", 0, dtype);
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> SddmmCsrHeadsOp::ModifyInputArg(
    const user_op::GetInputArgModifier& GetInputArgModifierFn, const user_op::UserOpConfWrapper&) {
  return IndexInputsNoGrad(GetInputArgModifierFn);
}

}  // namespace oneflow

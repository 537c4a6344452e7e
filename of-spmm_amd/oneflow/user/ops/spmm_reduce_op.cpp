/*
 * spmm_reduce_op.cpp — op "spmm_csr_reduce" (sum / mean / max / min aggregation of the CSR x dense
 * product, with the arg output of max / min) and the gradient ops of max / min.
 *
 *   spmm_csr_reduce(a_csr_row_ptr, a_csr_col_idx, a_csr_values, b[K,N]; reduce) -> out[M,N], arg
 *       arg[M,N] in the index dtype holds the winning global nonzero index for max / min and is an
 *       empty [0,N] tensor for sum / mean.
 *   spmm_csr_reduce_grad_b(at_row_ptr[K+1], at_col_idx[nnz], at_perm[nnz], a_csr_values[nnz],
 *                          arg[M,N], dy[M,N]) -> out[K,N]
 *       d(b) of max / min on A^T's structure (csr_transpose), selecting the winning entries.
 *   spmm_csr_reduce_grad_values(a_csr_row_ptr, a_csr_col_idx, arg[M,N], dy[M,N], b[K,N]) -> out[nnz]
 *       d(values) of max / min: the masked SDDMM.
 * Conventions and error wording of spmm_op.cpp / sddmm_op.cpp (templates
 * oneflow/user/ops/matrix_vector_product_op.cpp:73-107, unsorted_segment_sum_op.cpp:21-80).  The
 * shim's attribute map holds integers, so attr `reduce` (a string in the ODS record,
 * oneflow/ir/spmm_csr.td) is carried as its OFX_REDUCE_* code.
 *
 * SBP signatures of spmm_csr_reduce, as spmm_csr's (arg follows out; it holds global nonzero
 * indices, so a row split needs no fix-up):
 *   A parts B, b B,    out / arg S(0)
 *   A parts B, b S(1), out / arg S(1)
 */
#include "oneflow/core/framework/framework.h"
#include "oneflow/core/framework/op_generated.h"
#include "oneflow/user/ops/csr_op_util.h"
#include "ofx_spmm.h"

namespace oneflow {

namespace {

bool HasArg(int64_t reduce) { return reduce == OFX_REDUCE_MAX || reduce == OFX_REDUCE_MIN; }

Maybe<void> Check1D(user_op::InferContext* ctx, const char* name, int64_t elems, const char* what) {
  const Shape& s = ctx->InputShape(name, 0);
  CHECK_EQ_OR_RETURN(s.NumAxes(), 1)
      << Error::RuntimeError() << name << " should be 1-D, got shape " << s.ToString();
  if (elems >= 0)
    CHECK_EQ_OR_RETURN(s.At(0), elems)
        << Error::RuntimeError() << name << " should have " << what << " elements. ";
  return Maybe<void>::Ok();
}

Maybe<void> Check2D(user_op::InferContext* ctx, const char* name, int64_t rows, const char* what) {
  const Shape& s = ctx->InputShape(name, 0);
  CHECK_EQ_OR_RETURN(s.NumAxes(), 2)
      << Error::RuntimeError() << name << " should be 2-D, got shape " << s.ToString();
  CHECK_EQ_OR_RETURN(s.At(0), rows) << Error::RuntimeError() << name << " should have " << what
                                    << " rows. ";
  return Maybe<void>::Ok();
}

Maybe<void> CheckSizes(user_op::InferContext* ctx) {
  CHECK_GE_OR_RETURN(ctx->Attr<int64_t>("a_num_rows"), 0)
      << Error::RuntimeError() << "a_num_rows must be non-negative. ";
  CHECK_GE_OR_RETURN(ctx->Attr<int64_t>("a_num_cols"), 0)
      << Error::RuntimeError() << "a_num_cols must be non-negative. ";
  return Maybe<void>::Ok();
}

}  // namespace

// ---- spmm_csr_reduce ----------------------------------------------------------------------------
/* static */ Maybe<void> SpmmCsrReduceOp::InferLogicalTensorDesc(user_op::InferContext* ctx) {
  JUST(CheckSizes(ctx));
  const int64_t m = ctx->Attr<int64_t>("a_num_rows");
  const int64_t k = ctx->Attr<int64_t>("a_num_cols");
  const int64_t reduce = ctx->Attr<int64_t>("reduce");
  CHECK_OR_RETURN(reduce >= OFX_REDUCE_SUM && reduce <= OFX_REDUCE_MIN)
      << Error::RuntimeError() << "reduce should be sum, mean, max or min. ";
  JUST(Check1D(ctx, kRowPtr, m + 1, "a_num_rows + 1"));
  JUST(Check1D(ctx, kColIdx, -1, ""));
  JUST(Check1D(ctx, kValues, ctx->InputShape(kColIdx, 0).At(0), "nnz (as a_csr_col_idx)"));
  const Shape& b = ctx->InputShape("b", 0);
  CHECK_EQ_OR_RETURN(b.NumAxes(), 2)
      << Error::RuntimeError() << "b should be 2-D, got shape " << b.ToString();
  CHECK_EQ_OR_RETURN(b.At(0), k)
      << Error::RuntimeError() << "Dim K should be equal to b's dim0 (a_num_cols). ";
  ctx->SetOutputShape("out", 0, Shape({m, b.At(1)}));
  ctx->SetOutputShape("arg", 0, Shape({HasArg(reduce) ? m : 0, b.At(1)}));
  return Maybe<void>::Ok();
}

// Physical out / arg of a global op: GetPhysicalShape from their nd_sbp and the placement, as
// spmm_csr's out (spmm_op.cpp InferPhysicalOut4SpmmCsr).
/* static */ Maybe<void> SpmmCsrReduceOp::InferPhysicalTensorDesc(user_op::InferContext* ctx) {
  JUST(InferLogicalTensorDesc(ctx));
  if (ctx->parallel_ctx().parallel_num() == 1) return Maybe<void>::Ok();
  for (const char* name : {"out", "arg"}) {
    const user_op::TensorDesc* logical = ctx->LogicalTensorDesc4ArgNameAndIndex(name, 0);
    CHECK_NOTNULL_OR_RETURN(logical) << Error::RuntimeError() << "no logical desc for " << name;
    Shape physical;
    JUST(GetPhysicalShape(logical->shape(), ctx->NdSbp4ArgNameAndIndex(name, 0),
                          ctx->parallel_desc(), ctx->parallel_ctx(), &physical));
    CHECK_EQ_OR_RETURN(physical.At(1), ctx->InputShape("b", 0).At(1))
        << Error::RuntimeError() << "physical b has " << ctx->InputShape("b", 0).At(1)
        << " columns but " << name << "'s slice has " << physical.At(1);
    ctx->SetOutputShape(name, 0, physical);
  }
  return Maybe<void>::Ok();
}

/* static */ Maybe<void> SpmmCsrReduceOp::GetSbp(user_op::SbpContext* ctx) {
  ctx->NewBuilder()
      .Broadcast(user_op::OpArg(kRowPtr, 0))
      .Broadcast(user_op::OpArg(kColIdx, 0))
      .Broadcast(user_op::OpArg(kValues, 0))
      .Broadcast(user_op::OpArg("b", 0))
      .Split(user_op::OpArg("out", 0), 0)
      .Split(user_op::OpArg("arg", 0), 0)
      .Build();
  ctx->NewBuilder()
      .Broadcast(user_op::OpArg(kRowPtr, 0))
      .Broadcast(user_op::OpArg(kColIdx, 0))
      .Broadcast(user_op::OpArg(kValues, 0))
      .Split(user_op::OpArg("b", 0), 1)
      .Split(user_op::OpArg("out", 0), 1)
      .Split(user_op::OpArg("arg", 0), 1)
      .Build();
  return Maybe<void>::Ok();
}

/* static */ Maybe<void> SpmmCsrReduceOp::InferDataType(user_op::InferContext* ctx) {
  JUST(CheckIndexDTypes(ctx, kRowPtr, {kColIdx}));
  const DataType dtype = ctx->InputDType("b", 0);
  CHECK_EQ_OR_RETURN(ctx->InputDType(kValues, 0), dtype)
      << Error::TypeError() << "a_csr_values datatype should be equal to b. ";
  JUST(CheckValueDType(dtype, "spmm_csr_reduce"));
  ctx->SetOutputDType("out", 0, dtype);
  ctx->SetOutputDType("arg", 0, ctx->InputDType(kRowPtr, 0));
  return Maybe<void>::Ok();
}

/* static */ Maybe<void> SpmmCsrReduceOp::ModifyInputArg(
    const user_op::GetInputArgModifier& GetInputArgModifierFn, const user_op::UserOpConfWrapper&) {
  return IndexInputsNoGrad(GetInputArgModifierFn);
}

// ---- spmm_csr_reduce_grad_b -----------------------------------------------------------------------
/* static */ Maybe<void> SpmmCsrReduceGradBOp::InferLogicalTensorDesc(user_op::InferContext* ctx) {
  JUST(CheckSizes(ctx));
  const int64_t m = ctx->Attr<int64_t>("a_num_rows");
  const int64_t k = ctx->Attr<int64_t>("a_num_cols");
  JUST(Check1D(ctx, "at_row_ptr", k + 1, "a_num_cols + 1"));
  JUST(Check1D(ctx, "at_col_idx", -1, ""));
  const int64_t nnz = ctx->InputShape("at_col_idx", 0).At(0);
  JUST(Check1D(ctx, "at_perm", nnz, "nnz (as at_col_idx)"));
  JUST(Check1D(ctx, kValues, nnz, "nnz (as at_col_idx)"));
  JUST(Check2D(ctx, "arg", m, "a_num_rows"));
  JUST(Check2D(ctx, "dy", m, "a_num_rows"));
  CHECK_EQ_OR_RETURN(ctx->InputShape("arg", 0).At(1), ctx->InputShape("dy", 0).At(1))
      << Error::RuntimeError() << "arg and dy should have the same number of columns. ";
  ctx->SetOutputShape("out", 0, Shape({k, ctx->InputShape("dy", 0).At(1)}));
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> SpmmCsrReduceGradBOp::InferPhysicalTensorDesc(user_op::InferContext* ctx) {
  return InferLogicalTensorDesc(ctx);
}
/* static */ Maybe<void> SpmmCsrReduceGradBOp::GetSbp(user_op::SbpContext* ctx) {
  // Split N: every column is selected and summed on its own.
  ctx->NewBuilder()
      .Broadcast(user_op::OpArg("at_row_ptr", 0))
      .Broadcast(user_op::OpArg("at_col_idx", 0))
      .Broadcast(user_op::OpArg("at_perm", 0))
      .Broadcast(user_op::OpArg(kValues, 0))
      .Split(user_op::OpArg("arg", 0), 1)
      .Split(user_op::OpArg("dy", 0), 1)
      .Split(user_op::OpArg("out", 0), 1)
      .Build();
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> SpmmCsrReduceGradBOp::InferDataType(user_op::InferContext* ctx) {
  JUST(CheckIndexDTypes(ctx, "at_row_ptr", {"at_col_idx", "at_perm", "arg"}));
  const DataType dtype = ctx->InputDType("dy", 0);
  CHECK_EQ_OR_RETURN(ctx->InputDType(kValues, 0), dtype)
      << Error::TypeError() << "a_csr_values datatype should be equal to dy. ";
  JUST(CheckValueDType(dtype, "spmm_csr_reduce_grad_b"));
  ctx->SetOutputDType("out", 0, dtype);
  return Maybe<void>::Ok();
}

// ---- spmm_csr_reduce_grad_values ------------------------------------------------------------------
/* static */ Maybe<void> SpmmCsrReduceGradValuesOp::InferLogicalTensorDesc(
    user_op::InferContext* ctx) {
  JUST(CheckSizes(ctx));
  const int64_t m = ctx->Attr<int64_t>("a_num_rows");
  const int64_t k = ctx->Attr<int64_t>("a_num_cols");
  JUST(Check1D(ctx, kRowPtr, m + 1, "a_num_rows + 1"));
  JUST(Check1D(ctx, kColIdx, -1, ""));
  JUST(Check2D(ctx, "arg", m, "a_num_rows"));
  JUST(Check2D(ctx, "dy", m, "a_num_rows"));
  JUST(Check2D(ctx, "b", k, "a_num_cols"));
  const int64_t n = ctx->InputShape("b", 0).At(1);
  CHECK_OR_RETURN(ctx->InputShape("arg", 0).At(1) == n && ctx->InputShape("dy", 0).At(1) == n)
      << Error::RuntimeError() << "arg, dy and b should have the same number of columns. ";
  ctx->SetOutputShape("out", 0, Shape({ctx->InputShape(kColIdx, 0).At(0)}));
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> SpmmCsrReduceGradValuesOp::InferPhysicalTensorDesc(
    user_op::InferContext* ctx) {
  return InferLogicalTensorDesc(ctx);
}
/* static */ Maybe<void> SpmmCsrReduceGradValuesOp::GetSbp(user_op::SbpContext* ctx) {
  // Split N: partial dot products sum to the whole, as sddmm_csr.
  ctx->NewBuilder()
      .Broadcast(user_op::OpArg(kRowPtr, 0))
      .Broadcast(user_op::OpArg(kColIdx, 0))
      .Split(user_op::OpArg("arg", 0), 1)
      .Split(user_op::OpArg("dy", 0), 1)
      .Split(user_op::OpArg("b", 0), 1)
      .PartialSum(user_op::OpArg("out", 0))
      .Build();
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> SpmmCsrReduceGradValuesOp::InferDataType(user_op::InferContext* ctx) {
  JUST(CheckIndexDTypes(ctx, kRowPtr, {kColIdx, "arg"}));
  const DataType dtype = ctx->InputDType("b", 0);
  CHECK_EQ_OR_RETURN(ctx->InputDType("dy", 0), dtype)
      << Error::TypeError() << "dy datatype should be equal to b. ";
  JUST(CheckValueDType(dtype, "spmm_csr_reduce_grad_values"));
  ctx->SetOutputDType("out", 0, dtype);
  return Maybe<void>::Ok();
}

}  // namespace oneflow

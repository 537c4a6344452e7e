/*
 * spmm_multi_op.cpp — op "spmm_csr_multi": several aggregators (sum, mean, max, min, var, std) of
 * the messages values[j] * b[col[j], :] of every row from one walk of the CSR (Principal
 * Neighbourhood Aggregation, PyG's MultiAggregation).
 *
 *   spmm_csr_multi(a_csr_row_ptr[M+1], a_csr_col_idx[nnz], a_csr_values[nnz], b[K,N];
 *                  a_num_rows, a_num_cols, aggr_mask, eps) -> out[M, A*N], arg_max, arg_min
 *       out holds the A requested aggregators (aggr_mask: an OR of OFX_AGGR_*, include/ofx_spmm.h)
 *       as column blocks of width N in ascending bit order: PyG's concatenation, [M, A, N] viewed
 *       flat.  arg_max / arg_min [M,N] in the index dtype hold the winning global nonzero index of
 *       max / min and are empty [0,N] tensors without that aggregator.
 * Conventions and error wording of spmm_reduce_op.cpp.
 *
 * SBP: the row split of spmm_csr_reduce (A's parts and b broadcast, out and the args S(0); the
 * args hold global nonzero indices, so a row split needs no fix-up).  Its column split is not
 * offered: out's columns are A blocks of b's, so a slice of b's columns is not a slice of out's.
 */
#include "oneflow/core/framework/framework.h"
#include "oneflow/core/framework/op_generated.h"
#include "oneflow/user/ops/csr_op_util.h"
#include "ofx_spmm.h"

namespace oneflow {

namespace {

constexpr int64_t kAllAggrs = OFX_AGGR_SUM | OFX_AGGR_MEAN | OFX_AGGR_MAX | OFX_AGGR_MIN |
                              OFX_AGGR_VAR | OFX_AGGR_STD;
constexpr const char* kOuts[] = {"out", "arg_max", "arg_min"};

Maybe<void> Check1D(user_op::InferContext* ctx, const char* name, int64_t elems, const char* what) {
  const Shape& s = ctx->InputShape(name, 0);
  CHECK_EQ_OR_RETURN(s.NumAxes(), 1)
      << Error::RuntimeError() << name << " should be 1-D, got shape " << s.ToString();
  if (elems >= 0)
    CHECK_EQ_OR_RETURN(s.At(0), elems)
        << Error::RuntimeError() << name << " should have " << what << " elements. ";
  return Maybe<void>::Ok();
}

}  // namespace

/* static */ Maybe<void> SpmmCsrMultiOp::InferLogicalTensorDesc(user_op::InferContext* ctx) {
  const int64_t m = ctx->Attr<int64_t>("a_num_rows");
  const int64_t k = ctx->Attr<int64_t>("a_num_cols");
  CHECK_OR_RETURN(m >= 0 && k >= 0)
      << Error::RuntimeError() << "a_num_rows and a_num_cols must be non-negative. ";
  const int64_t mask = ctx->Attr<int64_t>("aggr_mask");
  CHECK_OR_RETURN(mask != 0 && (mask & ~kAllAggrs) == 0)
      << Error::RuntimeError() << "aggr_mask should be a non-empty OR of OFX_AGGR_*, got " << mask;
  const double eps = ctx->Attr<double>("eps");
  CHECK_OR_RETURN(eps >= 0.0 && eps <= 1.79769313486231570e308)
      << Error::RuntimeError() << "eps should be finite and >= 0, got " << eps;
  JUST(Check1D(ctx, kRowPtr, m + 1, "a_num_rows + 1"));
  JUST(Check1D(ctx, kColIdx, -1, ""));
  JUST(Check1D(ctx, kValues, ctx->InputShape(kColIdx, 0).At(0), "nnz (as a_csr_col_idx)"));
  const Shape& b = ctx->InputShape("b", 0);
  CHECK_EQ_OR_RETURN(b.NumAxes(), 2)
      << Error::RuntimeError() << "b should be 2-D, got shape " << b.ToString();
  CHECK_EQ_OR_RETURN(b.At(0), k)
      << Error::RuntimeError() << "Dim K should be equal to b's dim0 (a_num_cols). ";
  const int64_t n = b.At(1);
  ctx->SetOutputShape("out", 0, Shape({m, __builtin_popcountll(mask) * n}));
  ctx->SetOutputShape("arg_max", 0, Shape({(mask & OFX_AGGR_MAX) ? m : 0, n}));
  ctx->SetOutputShape("arg_min", 0, Shape({(mask & OFX_AGGR_MIN) ? m : 0, n}));
  return Maybe<void>::Ok();
}

// Physical outputs of a global op: this rank's rows (GetPhysicalShape, as spmm_csr_reduce's).
/* static */ Maybe<void> SpmmCsrMultiOp::InferPhysicalTensorDesc(user_op::InferContext* ctx) {
  JUST(InferLogicalTensorDesc(ctx));
  if (ctx->parallel_ctx().parallel_num() == 1) return Maybe<void>::Ok();
  for (const char* name : kOuts) {
    const user_op::TensorDesc* logical = ctx->LogicalTensorDesc4ArgNameAndIndex(name, 0);
    CHECK_NOTNULL_OR_RETURN(logical) << Error::RuntimeError() << "no logical desc for " << name;
    Shape physical;
    JUST(GetPhysicalShape(logical->shape(), ctx->NdSbp4ArgNameAndIndex(name, 0),
                          ctx->parallel_desc(), ctx->parallel_ctx(), &physical));
    ctx->SetOutputShape(name, 0, physical);
  }
  return Maybe<void>::Ok();
}

/* static */ Maybe<void> SpmmCsrMultiOp::GetSbp(user_op::SbpContext* ctx) {
  ctx->NewBuilder()
      .Broadcast(user_op::OpArg(kRowPtr, 0))
      .Broadcast(user_op::OpArg(kColIdx, 0))
      .Broadcast(user_op::OpArg(kValues, 0))
      .Broadcast(user_op::OpArg("b", 0))
      .Split(user_op::OpArg("out", 0), 0)
      .Split(user_op::OpArg("arg_max", 0), 0)
      .Split(user_op::OpArg("arg_min", 0), 0)
      .Build();
  return Maybe<void>::Ok();
}

/* static */ Maybe<void> SpmmCsrMultiOp::InferDataType(user_op::InferContext* ctx) {
  JUST(CheckIndexDTypes(ctx, kRowPtr, {kColIdx}));
  const DataType dtype = ctx->InputDType("b", 0);
  CHECK_EQ_OR_RETURN(ctx->InputDType(kValues, 0), dtype)
      << Error::TypeError() << "a_csr_values datatype should be equal to b. ";
  JUST(CheckValueDType(dtype, "spmm_csr_multi"));
  ctx->SetOutputDType("out", 0, dtype);
  ctx->SetOutputDType("arg_max", 0, ctx->InputDType(kRowPtr, 0));
  ctx->SetOutputDType("arg_min", 0, ctx->InputDType(kRowPtr, 0));
  return Maybe<void>::Ok();
}

/* static */ Maybe<void> SpmmCsrMultiOp::ModifyInputArg(
    const user_op::GetInputArgModifier& GetInputArgModifierFn, const user_op::UserOpConfWrapper&) {
  return IndexInputsNoGrad(GetInputArgModifierFn);
}

}  // namespace oneflow

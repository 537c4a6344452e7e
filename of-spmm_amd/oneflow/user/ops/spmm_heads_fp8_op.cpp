/*
 * spmm_heads_fp8_op.cpp — op "spmm_csr_heads_fp8": the multi-head SpMM of spmm_heads_op.cpp over
 * a feature table stored in OCP FP8 with an optional f32 scale per row of it.
 *
 *   spmm_csr_heads_fp8(a_csr_row_ptr[M+1], a_csr_col_idx[nnz], a_csr_values[nnz,H], b[K,N] uint8,
 *                      b_scale[K] float (optional); a_num_rows, a_num_cols, b_format) -> out[M,N]
 *       out[r, h*D + c] = sum over the row's nonzeros j of
 *                         (values[j, h] * b_scale[col[j]]) * dequant(b[col[j], h*D + c])
 * with D = N / H; b holds the FP8 codes as kUInt8 (DataType has no 8-bit float) and b_format names
 * the format (OFX_FP8_E4M3 = 1, OFX_FP8_E5M2 = 2).  out has the dtype of a_csr_values: float,
 * float16 or bfloat16.  Conventions and error wording of spmm_heads_op.cpp.
 *
 * SBP: all-broadcast only, as spmm_csr_heads.
 */
#include "oneflow/core/framework/framework.h"
#include "oneflow/core/framework/op_generated.h"
#include "oneflow/user/ops/csr_op_util.h"
#include "ofx_spmm.h"

namespace oneflow {

/* static */ Maybe<void> SpmmCsrHeadsFp8Op::InferLogicalTensorDesc(user_op::InferContext* ctx) {
  int64_t m = 0, nnz = 0;
  JUST(CheckCsrStructure(ctx, &m, &nnz));
  CHECK_EQ_OR_RETURN(m, ctx->Attr<int64_t>("a_num_rows"))
      << Error::RuntimeError() << kRowPtr << " should have a_num_rows + 1 elements. ";
  const int64_t k = ctx->Attr<int64_t>("a_num_cols");
  CHECK_GE_OR_RETURN(k, 0) << Error::RuntimeError() << "a_num_cols must be non-negative. ";
  const int64_t fmt = ctx->Attr<int64_t>("b_format");
  CHECK_OR_RETURN(fmt == OFX_FP8_E4M3 || fmt == OFX_FP8_E5M2)
      << Error::RuntimeError() << "b_format should be 1 (e4m3fn) or 2 (e5m2), got " << fmt << ". ";
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
  if (ctx->has_input("b_scale", 0)) {
    const Shape& s = ctx->InputShape("b_scale", 0);
    CHECK_OR_RETURN(s.NumAxes() == 1 && s.At(0) == k)
        << Error::RuntimeError() << "b_scale should be 1-D with a_num_cols elements, got shape "
        << s.ToString();
  }
  ctx->SetOutputShape("out", 0, Shape({m, b.At(1)}));
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> SpmmCsrHeadsFp8Op::InferPhysicalTensorDesc(user_op::InferContext* ctx) {
  return InferLogicalTensorDesc(ctx);
}
/* static */ Maybe<void> SpmmCsrHeadsFp8Op::GetSbp(user_op::SbpContext* ctx) {
  if (ctx->user_op_conf().has_input("b_scale", 0))
    return BroadcastAll(ctx, {kValues, "b", "b_scale", "out"});
  return BroadcastAll(ctx, {kValues, "b", "out"});
}
/* static */ Maybe<void> SpmmCsrHeadsFp8Op::InferDataType(user_op::InferContext* ctx) {
  JUST(CheckIndexDTypes(ctx));
  CHECK_EQ_OR_RETURN(ctx->InputDType("b", 0), kUInt8)
      << Error::TypeError() << "b should hold the FP8 codes as uint8, got "
      << DataType_Name(ctx->InputDType("b", 0));
  if (ctx->has_input("b_scale", 0)) {
    CHECK_EQ_OR_RETURN(ctx->InputDType("b_scale", 0), kFloat)
        << Error::TypeError() << "b_scale should be float, got "
        << DataType_Name(ctx->InputDType("b_scale", 0));
  }
  const DataType dtype = ctx->InputDType("a_csr_values", 0);
  CHECK_OR_RETURN(dtype == kFloat || dtype == kFloat16 || dtype == kBFloat16)
      << Error::TypeError() << "spmm_csr_heads_fp8 supports float, float16, bfloat16; got "
      << DataType_Name(dtype);
  ctx->SetOutputDType("out", 0, dtype);
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> SpmmCsrHeadsFp8Op::ModifyInputArg(
    const user_op::GetInputArgModifier& GetInputArgModifierFn,
    const user_op::UserOpConfWrapper&) {
  JUST(IndexInputsNoGrad(GetInputArgModifierFn));
  // the quantised table is a constant of the op: integer codes have no gradient
  user_op::InputArgModifier* modifier = GetInputArgModifierFn("b", 0);
  CHECK_NOTNULL_OR_RETURN(modifier);
  modifier->set_requires_grad(false);
  return Maybe<void>::Ok();
}

}  // namespace oneflow

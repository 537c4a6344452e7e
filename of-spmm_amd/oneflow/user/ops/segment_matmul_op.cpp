/*
 * segment_matmul_op.cpp — ops "segment_matmul" and "segment_matmul_grad_w": the typed linear
 * transform over rows sorted by type (RGCN, HGT, HeteroLinear; PyG's segment_matmul, DGL's
 * segment_mm / gather_mm over sorted types) and its gradient in w.
 *
 *   segment_matmul(x[R,F_in], w[T*F_in,F_out] (trans_w: [T*F_out,F_in]), seg_ptr[T+1],
 *                  idx[S] (optional); trans_w) -> out[S,F_out]
 *       out[i, :] = x[row(i), :] @ W[t] for seg_ptr[t] <= i < seg_ptr[t+1], row(i) = idx[i] or i
 *   segment_matmul_grad_w(x[R,F_in], dy[S,F_out], seg_ptr[T+1], idx[S] (optional); parts)
 *       -> dw[T*F_in,F_out]
 * w and dw are the [T, ., .] stacks viewed 2-D (tensors of this layer are 1-D or 2-D).  The
 * gradient in x is segment_matmul on dy with trans_w (and, with idx, a sum over equal idx through
 * spmm_csr): no op of its own.  Conventions and error wording of spmm_heads_op.cpp.
 *
 * SBP: all-broadcast only.
 */
#include "oneflow/core/framework/framework.h"
#include "oneflow/core/framework/op_generated.h"
#include "oneflow/user/ops/csr_op_util.h"
#include "ofx_spmm.h"

namespace oneflow {

namespace {

// x 2-D, seg_ptr 1-D with T + 1 >= 2 elements, idx (when present) 1-D; *s: the output rows.
Maybe<void> CheckSegmentInputs(user_op::InferContext* ctx, int64_t* t, int64_t* s) {
  const Shape& x = ctx->InputShape("x", 0);
  const Shape& sp = ctx->InputShape("seg_ptr", 0);
  CHECK_EQ_OR_RETURN(x.NumAxes(), 2)
      << Error::RuntimeError() << "x should be 2-D [R, F_in], got shape " << x.ToString();
  CHECK_OR_RETURN(sp.NumAxes() == 1 && sp.At(0) >= 2)
      << Error::RuntimeError() << "seg_ptr should be 1-D with T + 1 >= 2 elements, got shape "
      << sp.ToString();
  *t = sp.At(0) - 1;
  *s = x.At(0);
  if (ctx->has_input("idx", 0)) {
    const Shape& idx = ctx->InputShape("idx", 0);
    CHECK_EQ_OR_RETURN(idx.NumAxes(), 1)
        << Error::RuntimeError() << "idx should be 1-D [S], got shape " << idx.ToString();
    *s = idx.At(0);
  }
  return Maybe<void>::Ok();
}

// seg_ptr int32 / int64, idx of its dtype; every value input of x's dtype, one of the three.
Maybe<void> InferSegmentDType(user_op::InferContext* ctx, const char* op, const char* other,
                              const char* out) {
  if (ctx->has_input("idx", 0))
    JUST(CheckIndexDTypes(ctx, "seg_ptr", {"idx"}));
  else
    JUST(CheckIndexDTypes(ctx, "seg_ptr", {}));
  const DataType dtype = ctx->InputDType("x", 0);
  CHECK_EQ_OR_RETURN(ctx->InputDType(other, 0), dtype)
      << Error::TypeError() << other << " datatype should be equal to x. ";
  CHECK_OR_RETURN(dtype == kFloat || dtype == kFloat16 || dtype == kBFloat16)
      << Error::TypeError() << op << " supports float, float16, bfloat16; got x of "
      << DataType_Name(dtype);
  ctx->SetOutputDType(out, 0, dtype);
  return Maybe<void>::Ok();
}

Maybe<void> BroadcastEvery(user_op::SbpContext* ctx, std::initializer_list<const char*> args) {
  auto builder = ctx->NewBuilder();
  for (const char* name : args) builder.Broadcast(user_op::OpArg(name, 0));
  if (ctx->user_op_conf().has_input("idx", 0)) builder.Broadcast(user_op::OpArg("idx", 0));
  builder.Build();
  return Maybe<void>::Ok();
}

Maybe<void> SegmentIndexNoGrad(const user_op::GetInputArgModifier& GetInputArgModifierFn) {
  user_op::InputArgModifier* modifier = GetInputArgModifierFn("seg_ptr", 0);
  CHECK_NOTNULL_OR_RETURN(modifier);
  modifier->set_requires_grad(false);
  if (user_op::InputArgModifier* idx = GetInputArgModifierFn("idx", 0))
    idx->set_requires_grad(false);
  return Maybe<void>::Ok();
}

}  // namespace

// ---- segment_matmul -------------------------------------------------------------------------------
/* static */ Maybe<void> SegmentMatmulOp::InferLogicalTensorDesc(user_op::InferContext* ctx) {
  int64_t t = 0, s = 0;
  JUST(CheckSegmentInputs(ctx, &t, &s));
  const Shape& x = ctx->InputShape("x", 0);
  const Shape& w = ctx->InputShape("w", 0);
  const bool trans = ctx->Attr<int64_t>("trans_w") != 0;
  CHECK_OR_RETURN(w.NumAxes() == 2 && w.At(0) % t == 0 && w.At(0) >= t && w.At(1) >= 1)
      << Error::RuntimeError() << "w should be [T * " << (trans ? "F_out, F_in" : "F_in, F_out")
      << "] with T = " << t << " as seg_ptr, got shape " << w.ToString();
  const int64_t f_in = trans ? w.At(1) : w.At(0) / t, f_out = trans ? w.At(0) / t : w.At(1);
  CHECK_EQ_OR_RETURN(x.At(1), f_in)
      << Error::RuntimeError() << "x should have F_in = " << f_in << " columns as w"
      << (trans ? " (trans_w)" : "") << ", got shape " << x.ToString();
  ctx->SetOutputShape("out", 0, Shape({s, f_out}));
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> SegmentMatmulOp::InferPhysicalTensorDesc(user_op::InferContext* ctx) {
  return InferLogicalTensorDesc(ctx);
}
/* static */ Maybe<void> SegmentMatmulOp::GetSbp(user_op::SbpContext* ctx) {
  return BroadcastEvery(ctx, {"x", "w", "seg_ptr", "out"});
}
/* static */ Maybe<void> SegmentMatmulOp::InferDataType(user_op::InferContext* ctx) {
  return InferSegmentDType(ctx, "segment_matmul", "w", "out");
}
/* static */ Maybe<void> SegmentMatmulOp::ModifyInputArg(
    const user_op::GetInputArgModifier& GetInputArgModifierFn, const user_op::UserOpConfWrapper&) {
  return SegmentIndexNoGrad(GetInputArgModifierFn);
}

// ---- segment_matmul_grad_w ------------------------------------------------------------------------
/* static */ Maybe<void> SegmentMatmulGradWOp::InferLogicalTensorDesc(user_op::InferContext* ctx) {
  int64_t t = 0, s = 0;
  JUST(CheckSegmentInputs(ctx, &t, &s));
  const Shape& x = ctx->InputShape("x", 0);
  const Shape& dy = ctx->InputShape("dy", 0);
  CHECK_OR_RETURN(dy.NumAxes() == 2 && dy.At(0) == s && dy.At(1) >= 1)
      << Error::RuntimeError() << "dy should be [S, F_out] with S = " << s << ", got shape "
      << dy.ToString();
  CHECK_GE_OR_RETURN(x.At(1), 1) << Error::RuntimeError() << "x should have F_in >= 1 columns. ";
  CHECK_GE_OR_RETURN(ctx->Attr<int64_t>("parts"), 0)
      << Error::RuntimeError() << "parts should be >= 0 (0: chosen from the shapes). ";
  ctx->SetOutputShape("dw", 0, Shape({t * x.At(1), dy.At(1)}));
  return Maybe<void>::Ok();
}
/* static */ Maybe<void> SegmentMatmulGradWOp::InferPhysicalTensorDesc(user_op::InferContext* ctx) {
  return InferLogicalTensorDesc(ctx);
}
/* static */ Maybe<void> SegmentMatmulGradWOp::GetSbp(user_op::SbpContext* ctx) {
  return BroadcastEvery(ctx, {"x", "dy", "seg_ptr", "dw"});
}
/* static */ Maybe<void> SegmentMatmulGradWOp::InferDataType(user_op::InferContext* ctx) {
  return InferSegmentDType(ctx, "segment_matmul_grad_w", "dy", "dw");
}
/* static */ Maybe<void> SegmentMatmulGradWOp::ModifyInputArg(
    const user_op::GetInputArgModifier& GetInputArgModifierFn, const user_op::UserOpConfWrapper&) {
  return SegmentIndexNoGrad(GetInputArgModifierFn);
}

}  // namespace oneflow

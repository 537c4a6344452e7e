// op_generated.h — the declaration `oneflow_tblgen` would emit for the ODS entry of
// op "spmm_csr" (oneflow/ir/spmm_csr.td; generator tools/oneflow-tblgen/op_schema_header.inc:34-99).
#ifndef OFX_ONEFLOW_SHIM_OP_GENERATED_H_
#define OFX_ONEFLOW_SHIM_OP_GENERATED_H_

#include "oneflow/core/framework/framework.h"

namespace oneflow {

class SpmmCsrOp {
 public:
  static Maybe<void> InferLogicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> InferPhysicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> GetSbp(user_op::SbpContext* ctx);
  static Maybe<void> InferDataType(user_op::InferContext* ctx);
  static Maybe<void> ModifyInputArg(const user_op::GetInputArgModifier& GetInputArgModifierFn,
                                    const user_op::UserOpConfWrapper& conf);
};

// Fused epilogue variant.
class FusedSpmmCsrOp {
 public:
  static Maybe<void> InferLogicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> InferPhysicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> GetSbp(user_op::SbpContext* ctx);
  static Maybe<void> InferDataType(user_op::InferContext* ctx);
  static Maybe<void> ModifyInputArg(const user_op::GetInputArgModifier& GetInputArgModifierFn,
                                    const user_op::UserOpConfWrapper& conf);
};

// Gradient ops of spmm_csr.
class SddmmCsrOp {
 public:
  static Maybe<void> InferLogicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> InferPhysicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> GetSbp(user_op::SbpContext* ctx);
  static Maybe<void> InferDataType(user_op::InferContext* ctx);
};

// d(b) of spmm_csr with A's values read through A^T's perm (learnable edge weights).
class SpmmCsrGatheredOp {
 public:
  static Maybe<void> InferLogicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> InferPhysicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> GetSbp(user_op::SbpContext* ctx);
  static Maybe<void> InferDataType(user_op::InferContext* ctx);
  static Maybe<void> ModifyInputArg(const user_op::GetInputArgModifier& GetInputArgModifierFn,
                                    const user_op::UserOpConfWrapper& conf);
};

class CsrTransposeOp {
 public:
  static Maybe<void> InferLogicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> InferPhysicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> GetSbp(user_op::SbpContext* ctx);
  static Maybe<void> InferDataType(user_op::InferContext* ctx);
};

// Sum / mean / max / min aggregation with the arg output, and the gradient ops of max / min
// (oneflow/user/ops/spmm_reduce_op.cpp).
class SpmmCsrReduceOp {
 public:
  static Maybe<void> InferLogicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> InferPhysicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> GetSbp(user_op::SbpContext* ctx);
  static Maybe<void> InferDataType(user_op::InferContext* ctx);
  static Maybe<void> ModifyInputArg(const user_op::GetInputArgModifier& GetInputArgModifierFn,
                                    const user_op::UserOpConfWrapper& conf);
};

class SpmmCsrReduceGradBOp {
 public:
  static Maybe<void> InferLogicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> InferPhysicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> GetSbp(user_op::SbpContext* ctx);
  static Maybe<void> InferDataType(user_op::InferContext* ctx);
};

class SpmmCsrReduceGradValuesOp {
 public:
  static Maybe<void> InferLogicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> InferPhysicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> GetSbp(user_op::SbpContext* ctx);
  static Maybe<void> InferDataType(user_op::InferContext* ctx);
};

// The scores of a CSR's nonzeros normalised over each row, and its gradient op
// (oneflow/user/ops/edge_softmax_op.cpp).
class EdgeSoftmaxCsrOp {
 public:
  static Maybe<void> InferLogicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> InferPhysicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> GetSbp(user_op::SbpContext* ctx);
  static Maybe<void> InferDataType(user_op::InferContext* ctx);
  static Maybe<void> ModifyInputArg(const user_op::GetInputArgModifier& GetInputArgModifierFn,
                                    const user_op::UserOpConfWrapper& conf);
};

class EdgeSoftmaxCsrGradOp {
 public:
  static Maybe<void> InferLogicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> InferPhysicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> GetSbp(user_op::SbpContext* ctx);
  static Maybe<void> InferDataType(user_op::InferContext* ctx);
  static Maybe<void> ModifyInputArg(const user_op::GetInputArgModifier& GetInputArgModifierFn,
                                    const user_op::UserOpConfWrapper& conf);
};

// The multi-head SpMM and SDDMM of graph attention (oneflow/user/ops/spmm_heads_op.cpp).
class SpmmCsrHeadsOp {
 public:
  static Maybe<void> InferLogicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> InferPhysicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> GetSbp(user_op::SbpContext* ctx);
  static Maybe<void> InferDataType(user_op::InferContext* ctx);
  static Maybe<void> ModifyInputArg(const user_op::GetInputArgModifier& GetInputArgModifierFn,
                                    const user_op::UserOpConfWrapper& conf);
};

class SddmmCsrHeadsOp {
 public:
  static Maybe<void> InferLogicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> InferPhysicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> GetSbp(user_op::SbpContext* ctx);
  static Maybe<void> InferDataType(user_op::InferContext* ctx);
  static Maybe<void> ModifyInputArg(const user_op::GetInputArgModifier& GetInputArgModifierFn,
                                    const user_op::UserOpConfWrapper& conf);
};

// The multi-head edge softmax between them, and its gradient op
// (oneflow/user/ops/edge_softmax_heads_op.cpp).
class EdgeSoftmaxCsrHeadsOp {
 public:
  static Maybe<void> InferLogicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> InferPhysicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> GetSbp(user_op::SbpContext* ctx);
  static Maybe<void> InferDataType(user_op::InferContext* ctx);
  static Maybe<void> ModifyInputArg(const user_op::GetInputArgModifier& GetInputArgModifierFn,
                                    const user_op::UserOpConfWrapper& conf);
};

class EdgeSoftmaxCsrHeadsGradOp {
 public:
  static Maybe<void> InferLogicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> InferPhysicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> GetSbp(user_op::SbpContext* ctx);
  static Maybe<void> InferDataType(user_op::InferContext* ctx);
  static Maybe<void> ModifyInputArg(const user_op::GetInputArgModifier& GetInputArgModifierFn,
                                    const user_op::UserOpConfWrapper& conf);
};

// The fused multi-head graph attention (oneflow/user/ops/graph_attention_heads_op.cpp).
class GraphAttentionCsrHeadsOp {
 public:
  static Maybe<void> InferLogicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> InferPhysicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> GetSbp(user_op::SbpContext* ctx);
  static Maybe<void> InferDataType(user_op::InferContext* ctx);
  static Maybe<void> ModifyInputArg(const user_op::GetInputArgModifier& GetInputArgModifierFn,
                                    const user_op::UserOpConfWrapper& conf);
};

// The attention weights of a GAT layer (additive scores, LeakyReLU, softmax) and their gradient op
// (oneflow/user/ops/gat_softmax_heads_op.cpp).
class GatSoftmaxCsrHeadsOp {
 public:
  static Maybe<void> InferLogicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> InferPhysicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> GetSbp(user_op::SbpContext* ctx);
  static Maybe<void> InferDataType(user_op::InferContext* ctx);
  static Maybe<void> ModifyInputArg(const user_op::GetInputArgModifier& GetInputArgModifierFn,
                                    const user_op::UserOpConfWrapper& conf);
};

class GatSoftmaxCsrHeadsGradOp {
 public:
  static Maybe<void> InferLogicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> InferPhysicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> GetSbp(user_op::SbpContext* ctx);
  static Maybe<void> InferDataType(user_op::InferContext* ctx);
  static Maybe<void> ModifyInputArg(const user_op::GetInputArgModifier& GetInputArgModifierFn,
                                    const user_op::UserOpConfWrapper& conf);
};

// The attention scores of a GATv2 layer (LeakyReLU between the gather and the dot product) and
// their gradient op (oneflow/user/ops/gatv2_scores_heads_op.cpp).
class Gatv2ScoresCsrHeadsOp {
 public:
  static Maybe<void> InferLogicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> InferPhysicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> GetSbp(user_op::SbpContext* ctx);
  static Maybe<void> InferDataType(user_op::InferContext* ctx);
  static Maybe<void> ModifyInputArg(const user_op::GetInputArgModifier& GetInputArgModifierFn,
                                    const user_op::UserOpConfWrapper& conf);
};

class Gatv2ScoresCsrHeadsGradOp {
 public:
  static Maybe<void> InferLogicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> InferPhysicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> GetSbp(user_op::SbpContext* ctx);
  static Maybe<void> InferDataType(user_op::InferContext* ctx);
  static Maybe<void> ModifyInputArg(const user_op::GetInputArgModifier& GetInputArgModifierFn,
                                    const user_op::UserOpConfWrapper& conf);
};

// The multi-head SpMM over an FP8 feature table with an optional scale per row of it
// (oneflow/user/ops/spmm_heads_fp8_op.cpp).
class SpmmCsrHeadsFp8Op {
 public:
  static Maybe<void> InferLogicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> InferPhysicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> GetSbp(user_op::SbpContext* ctx);
  static Maybe<void> InferDataType(user_op::InferContext* ctx);
  static Maybe<void> ModifyInputArg(const user_op::GetInputArgModifier& GetInputArgModifierFn,
                                    const user_op::UserOpConfWrapper& conf);
};

// The S(0) -> B collectives the row-split op's B operand goes through: eager boxing
// (oneflow/user/ops/eager_nccl_ops.cpp:188-233) and the lazy graph's logical collective
// (oneflow/user/ops/nccl_logical_ops.cpp:104-142, ODS OneFlowUserOps.td:5341-5357).
class EagerCclAllGatherOp {
 public:
  static Maybe<void> InferLogicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> InferPhysicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> GetSbp(user_op::SbpContext* ctx);
  static Maybe<void> InferNdSbp(user_op::InferNdSbpFnContext* ctx);
  static Maybe<void> InferDataType(user_op::InferContext* ctx);
};

class _ncclLogicalAllGatherOp {
 public:
  static Maybe<void> InferLogicalTensorDesc(user_op::InferContext* ctx);
  static Maybe<void> GetSbp(user_op::SbpContext* ctx);
  static Maybe<void> InferNdSbp(user_op::InferNdSbpFnContext* ctx);
  static Maybe<void> InferDataType(user_op::InferContext* ctx);
};

}  // namespace oneflow

#endif  // OFX_ONEFLOW_SHIM_OP_GENERATED_H_

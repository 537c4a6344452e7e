// ODS entry for op "spmm_csr" — to be placed in the MATMUL group of
// oneflow/ir/include/OneFlow/OneFlowUserOps.td (group spans :4259-4601 in the reference; same form
// as OneFlow_MatrixVectorProductOp :4402-4414 and the typed attrs of OneFlow_UnsortedSegmentSumOp
// :3278-3295).  oneflow_tblgen turns it into the SpmmCsrOp declaration and REGISTER_USER_OP we
// hand-wrote in of-spmm_amd/oneflow/core/framework/op_generated.{h,cpp}.
def OneFlow_SpmmCsrOp : OneFlow_BaseOp<"spmm_csr", [NoSideEffect, DeclareOpInterfaceMethods<UserOpCompatibleInterface>]> {
  let input = (ins
    OneFlow_Tensor:$a_csr_row_ptr,
    OneFlow_Tensor:$a_csr_col_idx,
    OneFlow_Tensor:$a_csr_values,
    OneFlow_Tensor:$b
  );
  let output = (outs
    OneFlow_Tensor:$out
  );
  // static_csr (0 = off): the caller's promise that the CSR is not rewritten while the op lives,
  // and its name for it; the kernel state then keeps the work-list plan across calls
  // (include/ofx_spmm.h ofx_spmm_attrs)
  let attrs = (ins
    DefaultValuedAttr<SI64Attr, "0">:$a_num_rows,
    DefaultValuedAttr<SI64Attr, "0">:$a_num_cols,
    DefaultValuedAttr<SI64Attr, "0">:$static_csr
  );
  let has_logical_tensor_desc_infer_fn = 1;
  let has_physical_tensor_desc_infer_fn = 1;
  let has_get_sbp_fn = 1;
  let has_data_type_infer_fn = 1;
  let has_input_arg_modify_fn = 1;
}

// Fused epilogue (SURVEY.md §8f row 4): out = relu?(A @ b + bias?), the composition
// spmm_csr -> bias_add -> relu in one kernel.  Optional input as in OneFlowUserOps.td's
// Optional<OneFlow_Tensor> entries (e.g. :5763); bool attr as skip_final_activation of
// fused_matmul_bias_add_relu_dropout.
def OneFlow_FusedSpmmCsrOp : OneFlow_BaseOp<"fused_spmm_csr", [NoSideEffect, AttrSizedOperandSegments, DeclareOpInterfaceMethods<UserOpCompatibleInterface>]> {
  let input = (ins
    OneFlow_Tensor:$a_csr_row_ptr,
    OneFlow_Tensor:$a_csr_col_idx,
    OneFlow_Tensor:$a_csr_values,
    OneFlow_Tensor:$b,
    Optional<OneFlow_Tensor>:$bias
  );
  let output = (outs
    OneFlow_Tensor:$out
  );
  let attrs = (ins
    DefaultValuedAttr<SI64Attr, "0">:$a_num_rows,
    DefaultValuedAttr<SI64Attr, "0">:$a_num_cols,
    DefaultValuedAttr<BoolAttr, "false">:$relu,
    DefaultValuedAttr<SI64Attr, "0">:$static_csr
  );
  let has_logical_tensor_desc_infer_fn = 1;
  let has_physical_tensor_desc_infer_fn = 1;
  let has_get_sbp_fn = 1;
  let has_data_type_infer_fn = 1;
  let has_input_arg_modify_fn = 1;
}

// d(b) of spmm_csr with learnable values (SURVEY.md §8f row 1): out = A @ b where nonzero j's
// value is a_csr_values[values_perm[j]] (A^T's structure, A's values, A^T's perm from
// csr_transpose), so the gradient never writes the gathered copy.
def OneFlow_SpmmCsrGatheredOp : OneFlow_BaseOp<"spmm_csr_gathered", [NoSideEffect, DeclareOpInterfaceMethods<UserOpCompatibleInterface>]> {
  let input = (ins
    OneFlow_Tensor:$a_csr_row_ptr,
    OneFlow_Tensor:$a_csr_col_idx,
    OneFlow_Tensor:$a_csr_values,
    OneFlow_Tensor:$values_perm,
    OneFlow_Tensor:$b
  );
  let output = (outs
    OneFlow_Tensor:$out
  );
  let attrs = (ins
    DefaultValuedAttr<SI64Attr, "0">:$a_num_rows,
    DefaultValuedAttr<SI64Attr, "0">:$a_num_cols,
    DefaultValuedAttr<SI64Attr, "0">:$static_csr
  );
  let has_logical_tensor_desc_infer_fn = 1;
  let has_physical_tensor_desc_infer_fn = 1;
  let has_get_sbp_fn = 1;
  let has_data_type_infer_fn = 1;
  let has_input_arg_modify_fn = 1;
}

// Sum / mean / max / min aggregation (PyG's reduce=, DGL's u_mul_e_max): out = reduce_j
// a_csr_values[j] * b[a_csr_col_idx[j], :], arg = the winning global nonzero index of max / min
// in the index dtype (an empty [0, N] tensor for sum / mean).  String attr as `padding` of
// OneFlow_Conv2DOp's DefaultValuedAttr<StrAttr, ...> entries.
def OneFlow_SpmmCsrReduceOp : OneFlow_BaseOp<"spmm_csr_reduce", [NoSideEffect, DeclareOpInterfaceMethods<UserOpCompatibleInterface>]> {
  let input = (ins
    OneFlow_Tensor:$a_csr_row_ptr,
    OneFlow_Tensor:$a_csr_col_idx,
    OneFlow_Tensor:$a_csr_values,
    OneFlow_Tensor:$b
  );
  let output = (outs
    OneFlow_Tensor:$out,
    OneFlow_Tensor:$arg
  );
  let attrs = (ins
    DefaultValuedAttr<SI64Attr, "0">:$a_num_rows,
    DefaultValuedAttr<SI64Attr, "0">:$a_num_cols,
    DefaultValuedAttr<StrAttr, "\"sum\"">:$reduce
  );
  let has_logical_tensor_desc_infer_fn = 1;
  let has_physical_tensor_desc_infer_fn = 1;
  let has_get_sbp_fn = 1;
  let has_data_type_infer_fn = 1;
  let has_input_arg_modify_fn = 1;
}

// d(b) of spmm_csr_reduce (max / min) on A^T's structure (csr_transpose), selecting the entries
// that won their (row, column): deterministic, in the sum op's order on A^T.
def OneFlow_SpmmCsrReduceGradBOp : OneFlow_BaseOp<"spmm_csr_reduce_grad_b", [NoSideEffect, DeclareOpInterfaceMethods<UserOpCompatibleInterface>]> {
  let input = (ins
    OneFlow_Tensor:$at_row_ptr,
    OneFlow_Tensor:$at_col_idx,
    OneFlow_Tensor:$at_perm,
    OneFlow_Tensor:$a_csr_values,
    OneFlow_Tensor:$arg,
    OneFlow_Tensor:$dy
  );
  let output = (outs
    OneFlow_Tensor:$out
  );
  let attrs = (ins
    DefaultValuedAttr<SI64Attr, "0">:$a_num_rows,
    DefaultValuedAttr<SI64Attr, "0">:$a_num_cols
  );
  let has_logical_tensor_desc_infer_fn = 1;
  let has_physical_tensor_desc_infer_fn = 1;
  let has_get_sbp_fn = 1;
  let has_data_type_infer_fn = 1;
}

// d(values) of spmm_csr_reduce (max / min): the SDDMM of dy and b over the columns each nonzero won.
def OneFlow_SpmmCsrReduceGradValuesOp : OneFlow_BaseOp<"spmm_csr_reduce_grad_values", [NoSideEffect, DeclareOpInterfaceMethods<UserOpCompatibleInterface>]> {
  let input = (ins
    OneFlow_Tensor:$a_csr_row_ptr,
    OneFlow_Tensor:$a_csr_col_idx,
    OneFlow_Tensor:$arg,
    OneFlow_Tensor:$dy,
    OneFlow_Tensor:$b
  );
  let output = (outs
    OneFlow_Tensor:$out
  );
  let attrs = (ins
    DefaultValuedAttr<SI64Attr, "0">:$a_num_rows,
    DefaultValuedAttr<SI64Attr, "0">:$a_num_cols
  );
  let has_logical_tensor_desc_infer_fn = 1;
  let has_physical_tensor_desc_infer_fn = 1;
  let has_get_sbp_fn = 1;
  let has_data_type_infer_fn = 1;
}

// The scores of a CSR's nonzeros normalised over each row (DGL's edge_softmax, PyG's
// softmax(src, ptr=row_ptr)).  No attributes: the row count is a_csr_row_ptr's length - 1;
// a_csr_col_idx is taken for its shape only.  SBP: all-broadcast (a split along nnz would cut rows).
def OneFlow_EdgeSoftmaxCsrOp : OneFlow_BaseOp<"edge_softmax_csr", [NoSideEffect, DeclareOpInterfaceMethods<UserOpCompatibleInterface>]> {
  let input = (ins
    OneFlow_Tensor:$a_csr_row_ptr,
    OneFlow_Tensor:$a_csr_col_idx,
    OneFlow_Tensor:$e
  );
  let output = (outs
    OneFlow_Tensor:$out
  );
  let has_logical_tensor_desc_infer_fn = 1;
  let has_physical_tensor_desc_infer_fn = 1;
  let has_get_sbp_fn = 1;
  let has_data_type_infer_fn = 1;
  let has_input_arg_modify_fn = 1;
}

// Its gradient from the forward's stored output: dx = y * (dy - sum over the row of y * dy).
def OneFlow_EdgeSoftmaxCsrGradOp : OneFlow_BaseOp<"edge_softmax_csr_grad", [NoSideEffect, DeclareOpInterfaceMethods<UserOpCompatibleInterface>]> {
  let input = (ins
    OneFlow_Tensor:$a_csr_row_ptr,
    OneFlow_Tensor:$a_csr_col_idx,
    OneFlow_Tensor:$y,
    OneFlow_Tensor:$dy
  );
  let output = (outs
    OneFlow_Tensor:$dx
  );
  let has_logical_tensor_desc_infer_fn = 1;
  let has_physical_tensor_desc_infer_fn = 1;
  let has_get_sbp_fn = 1;
  let has_data_type_infer_fn = 1;
  let has_input_arg_modify_fn = 1;
}

// The multi-head SpMM of graph attention: a_csr_values is [nnz, H], b is [K, H*D] with head h in
// columns [h*D, (h+1)*D); out[r, h*D + c] = sum_j values[j, h] * b[col[j], h*D + c].  Every head's
// slice has the bits of spmm_csr on that slice.  SBP: all-broadcast.
def OneFlow_SpmmCsrHeadsOp : OneFlow_BaseOp<"spmm_csr_heads", [NoSideEffect, DeclareOpInterfaceMethods<UserOpCompatibleInterface>]> {
  let input = (ins
    OneFlow_Tensor:$a_csr_row_ptr,
    OneFlow_Tensor:$a_csr_col_idx,
    OneFlow_Tensor:$a_csr_values,
    OneFlow_Tensor:$b
  );
  let output = (outs
    OneFlow_Tensor:$out
  );
  let attrs = (ins
    DefaultValuedAttr<SI64Attr, "0">:$a_num_rows,
    DefaultValuedAttr<SI64Attr, "0">:$a_num_cols
  );
  let has_logical_tensor_desc_infer_fn = 1;
  let has_physical_tensor_desc_infer_fn = 1;
  let has_get_sbp_fn = 1;
  let has_data_type_infer_fn = 1;
  let has_input_arg_modify_fn = 1;
}

// The multi-head SDDMM: out[j, h] = <a[row(j), h*D:(h+1)*D], b[col(j), h*D:(h+1)*D]>, out is
// [nnz, num_heads]: the scores of multi-head attention and d(values) of spmm_csr_heads.
def OneFlow_SddmmCsrHeadsOp : OneFlow_BaseOp<"sddmm_csr_heads", [NoSideEffect, DeclareOpInterfaceMethods<UserOpCompatibleInterface>]> {
  let input = (ins
    OneFlow_Tensor:$a_csr_row_ptr,
    OneFlow_Tensor:$a_csr_col_idx,
    OneFlow_Tensor:$a,
    OneFlow_Tensor:$b
  );
  let output = (outs
    OneFlow_Tensor:$out
  );
  let attrs = (ins
    DefaultValuedAttr<SI64Attr, "1">:$num_heads
  );
  let has_logical_tensor_desc_infer_fn = 1;
  let has_physical_tensor_desc_infer_fn = 1;
  let has_get_sbp_fn = 1;
  let has_data_type_infer_fn = 1;
  let has_input_arg_modify_fn = 1;
}

// The multi-head edge softmax between the two: e is [nnz, H] (sddmm_csr_heads's output), out is
// [nnz, H]; every head is normalised over each row on its own and has the bits of edge_softmax_csr
// on its column.  One launch for all heads.  SBP: all-broadcast.
def OneFlow_EdgeSoftmaxCsrHeadsOp : OneFlow_BaseOp<"edge_softmax_csr_heads", [NoSideEffect, DeclareOpInterfaceMethods<UserOpCompatibleInterface>]> {
  let input = (ins
    OneFlow_Tensor:$a_csr_row_ptr,
    OneFlow_Tensor:$a_csr_col_idx,
    OneFlow_Tensor:$e
  );
  let output = (outs
    OneFlow_Tensor:$out
  );
  let has_logical_tensor_desc_infer_fn = 1;
  let has_physical_tensor_desc_infer_fn = 1;
  let has_get_sbp_fn = 1;
  let has_data_type_infer_fn = 1;
  let has_input_arg_modify_fn = 1;
}

// Its gradient from the forward's stored output, per head:
// dx[:, h] = y[:, h] * (dy[:, h] - sum over the row of y[:, h] * dy[:, h]).
def OneFlow_EdgeSoftmaxCsrHeadsGradOp : OneFlow_BaseOp<"edge_softmax_csr_heads_grad", [NoSideEffect, DeclareOpInterfaceMethods<UserOpCompatibleInterface>]> {
  let input = (ins
    OneFlow_Tensor:$a_csr_row_ptr,
    OneFlow_Tensor:$a_csr_col_idx,
    OneFlow_Tensor:$y,
    OneFlow_Tensor:$dy
  );
  let output = (outs
    OneFlow_Tensor:$dx
  );
  let has_logical_tensor_desc_infer_fn = 1;
  let has_physical_tensor_desc_infer_fn = 1;
  let has_get_sbp_fn = 1;
  let has_data_type_infer_fn = 1;
  let has_input_arg_modify_fn = 1;
}

// Dot-product graph attention over a CSR as one op: q is [M, H*D], k and v are
// [K, H*D]; attn [nnz, num_heads] = edge_softmax_csr_heads(sddmm_csr_heads(q, k)) and
// out [M, H*D] = spmm_csr_heads(attn, v), both with the bits of that composition.
// SBP: all-broadcast.
def OneFlow_GraphAttentionCsrHeadsOp : OneFlow_BaseOp<"graph_attention_csr_heads", [NoSideEffect, DeclareOpInterfaceMethods<UserOpCompatibleInterface>]> {
  let input = (ins
    OneFlow_Tensor:$a_csr_row_ptr,
    OneFlow_Tensor:$a_csr_col_idx,
    OneFlow_Tensor:$q,
    OneFlow_Tensor:$k,
    OneFlow_Tensor:$v
  );
  let output = (outs
    OneFlow_Tensor:$out,
    OneFlow_Tensor:$attn
  );
  let attrs = (ins
    DefaultValuedAttr<SI64Attr, "1">:$num_heads
  );
  let has_logical_tensor_desc_infer_fn = 1;
  let has_physical_tensor_desc_infer_fn = 1;
  let has_get_sbp_fn = 1;
  let has_data_type_infer_fn = 1;
  let has_input_arg_modify_fn = 1;
}

// The attention weights of a GAT layer over a CSR: s_row is [M, H], s_col is [K, H]; out [nnz, H]
// = edge_softmax_csr_heads of e[j, h] = LeakyReLU(s_row[row(j), h] + s_col[col[j], h]) rounded to
// the dtype, in one launch; e is never written.  negative_slope must be finite and > 0.
// SBP: all-broadcast.
def OneFlow_GatSoftmaxCsrHeadsOp : OneFlow_BaseOp<"gat_softmax_csr_heads", [NoSideEffect, DeclareOpInterfaceMethods<UserOpCompatibleInterface>]> {
  let input = (ins
    OneFlow_Tensor:$a_csr_row_ptr,
    OneFlow_Tensor:$a_csr_col_idx,
    OneFlow_Tensor:$s_row,
    OneFlow_Tensor:$s_col
  );
  let output = (outs
    OneFlow_Tensor:$out
  );
  let attrs = (ins
    DefaultValuedAttr<F64Attr, "0.2">:$negative_slope
  );
  let has_logical_tensor_desc_infer_fn = 1;
  let has_physical_tensor_desc_infer_fn = 1;
  let has_get_sbp_fn = 1;
  let has_data_type_infer_fn = 1;
  let has_input_arg_modify_fn = 1;
}

// Its gradient from the forward's stored output: ds [nnz, H] = edge_softmax_csr_heads_grad(y, dy)
// times LeakyReLU's derivative at the recomputed sum, and d_row [M, H], the sum of ds over each
// row (the gradient in s_row).
def OneFlow_GatSoftmaxCsrHeadsGradOp : OneFlow_BaseOp<"gat_softmax_csr_heads_grad", [NoSideEffect, DeclareOpInterfaceMethods<UserOpCompatibleInterface>]> {
  let input = (ins
    OneFlow_Tensor:$a_csr_row_ptr,
    OneFlow_Tensor:$a_csr_col_idx,
    OneFlow_Tensor:$s_row,
    OneFlow_Tensor:$s_col,
    OneFlow_Tensor:$y,
    OneFlow_Tensor:$dy
  );
  let output = (outs
    OneFlow_Tensor:$ds,
    OneFlow_Tensor:$d_row
  );
  let attrs = (ins
    DefaultValuedAttr<F64Attr, "0.2">:$negative_slope
  );
  let has_logical_tensor_desc_infer_fn = 1;
  let has_physical_tensor_desc_infer_fn = 1;
  let has_get_sbp_fn = 1;
  let has_data_type_infer_fn = 1;
  let has_input_arg_modify_fn = 1;
}

// The attention scores of a GATv2 layer over a CSR: x_row is [M, H*D], x_col is [K, H*D], att is
// [H*D] with head h in columns [h*D, (h+1)*D); out [nnz, H] with
// out[j, h] = <att[h], LeakyReLU(x_row[row(j), h] + x_col[col[j], h])>, the activated sum rounded
// to the dtype and never written: the bits of sddmm_csr_heads on it.  negative_slope must be
// finite and > 0.  SBP: all-broadcast.
def OneFlow_Gatv2ScoresCsrHeadsOp : OneFlow_BaseOp<"gatv2_scores_csr_heads", [NoSideEffect, DeclareOpInterfaceMethods<UserOpCompatibleInterface>]> {
  let input = (ins
    OneFlow_Tensor:$a_csr_row_ptr,
    OneFlow_Tensor:$a_csr_col_idx,
    OneFlow_Tensor:$x_row,
    OneFlow_Tensor:$x_col,
    OneFlow_Tensor:$att
  );
  let output = (outs
    OneFlow_Tensor:$out
  );
  let attrs = (ins
    DefaultValuedAttr<SI64Attr, "1">:$num_heads,
    DefaultValuedAttr<F64Attr, "0.2">:$negative_slope
  );
  let has_logical_tensor_desc_infer_fn = 1;
  let has_physical_tensor_desc_infer_fn = 1;
  let has_get_sbp_fn = 1;
  let has_data_type_infer_fn = 1;
  let has_input_arg_modify_fn = 1;
}

// Its gradient from the upstream dy [nnz, H]: d_x [M, H*D], the gradient in x_row, and p [M, H*D]
// (with_att; otherwise [0, H*D]), whose column sum is the gradient in att.  Both have the bits of
// spmm_csr_heads over the row's nonzeros on the per-nonzero terms rounded to the dtype.
def OneFlow_Gatv2ScoresCsrHeadsGradOp : OneFlow_BaseOp<"gatv2_scores_csr_heads_grad", [NoSideEffect, DeclareOpInterfaceMethods<UserOpCompatibleInterface>]> {
  let input = (ins
    OneFlow_Tensor:$a_csr_row_ptr,
    OneFlow_Tensor:$a_csr_col_idx,
    OneFlow_Tensor:$x_row,
    OneFlow_Tensor:$x_col,
    OneFlow_Tensor:$att,
    OneFlow_Tensor:$dy
  );
  let output = (outs
    OneFlow_Tensor:$d_x,
    OneFlow_Tensor:$p
  );
  let attrs = (ins
    DefaultValuedAttr<SI64Attr, "1">:$num_heads,
    DefaultValuedAttr<F64Attr, "0.2">:$negative_slope,
    DefaultValuedAttr<SI64Attr, "1">:$with_att
  );
  let has_logical_tensor_desc_infer_fn = 1;
  let has_physical_tensor_desc_infer_fn = 1;
  let has_get_sbp_fn = 1;
  let has_data_type_infer_fn = 1;
  let has_input_arg_modify_fn = 1;
}

// The multi-head SpMM over an FP8 feature table: b holds OCP FP8 codes as uint8 (b_format: 1 =
// e4m3fn, 2 = e5m2), b_scale an optional float scale per row of b;
// out[r, h*D + c] = sum_j (values[j, h] * b_scale[col[j]]) * dequant(b[col[j], h*D + c]) with the
// bits of spmm_csr_heads on the scaled values rounded to the dtype and the dequantised b.  out has
// the dtype of a_csr_values (float, float16, bfloat16).  SBP: all-broadcast.
def OneFlow_SpmmCsrHeadsFp8Op : OneFlow_BaseOp<"spmm_csr_heads_fp8", [NoSideEffect, DeclareOpInterfaceMethods<UserOpCompatibleInterface>]> {
  let input = (ins
    OneFlow_Tensor:$a_csr_row_ptr,
    OneFlow_Tensor:$a_csr_col_idx,
    OneFlow_Tensor:$a_csr_values,
    OneFlow_Tensor:$b,
    Optional<OneFlow_Tensor>:$b_scale
  );
  let output = (outs
    OneFlow_Tensor:$out
  );
  let attrs = (ins
    DefaultValuedAttr<SI64Attr, "0">:$a_num_rows,
    DefaultValuedAttr<SI64Attr, "0">:$a_num_cols,
    DefaultValuedAttr<SI64Attr, "1">:$b_format
  );
  let has_logical_tensor_desc_infer_fn = 1;
  let has_physical_tensor_desc_infer_fn = 1;
  let has_get_sbp_fn = 1;
  let has_data_type_infer_fn = 1;
  let has_input_arg_modify_fn = 1;
}

// The SpMM over per-edge feature vectors: e [nnz, N], b [K, N];
// out[r, n] = sum over the row's nonzeros j of act(b[col[j], n] op e[j, n]) with op 0 = mul,
// 1 = add and act 0 = none, 1 = relu, each message rounded to the dtype before the sum.
// SBP: all-broadcast.
def OneFlow_SpmmCsrEdgeOp : OneFlow_BaseOp<"spmm_csr_edge", [NoSideEffect, DeclareOpInterfaceMethods<UserOpCompatibleInterface>]> {
  let input = (ins
    OneFlow_Tensor:$a_csr_row_ptr,
    OneFlow_Tensor:$a_csr_col_idx,
    OneFlow_Tensor:$e,
    OneFlow_Tensor:$b
  );
  let output = (outs
    OneFlow_Tensor:$out
  );
  let attrs = (ins
    DefaultValuedAttr<SI64Attr, "0">:$a_num_rows,
    DefaultValuedAttr<SI64Attr, "0">:$a_num_cols,
    DefaultValuedAttr<SI64Attr, "0">:$op,
    DefaultValuedAttr<SI64Attr, "0">:$act
  );
  let has_logical_tensor_desc_infer_fn = 1;
  let has_physical_tensor_desc_infer_fn = 1;
  let has_get_sbp_fn = 1;
  let has_data_type_infer_fn = 1;
  let has_input_arg_modify_fn = 1;
}

// Its gradient in e from the upstream dy [M, N]: de [nnz, N].
def OneFlow_SpmmCsrEdgeGradEOp : OneFlow_BaseOp<"spmm_csr_edge_grad_e", [NoSideEffect, DeclareOpInterfaceMethods<UserOpCompatibleInterface>]> {
  let input = (ins
    OneFlow_Tensor:$a_csr_row_ptr,
    OneFlow_Tensor:$a_csr_col_idx,
    OneFlow_Tensor:$e,
    OneFlow_Tensor:$b,
    OneFlow_Tensor:$dy
  );
  let output = (outs
    OneFlow_Tensor:$de
  );
  let attrs = (ins
    DefaultValuedAttr<SI64Attr, "0">:$op,
    DefaultValuedAttr<SI64Attr, "0">:$act
  );
  let has_logical_tensor_desc_infer_fn = 1;
  let has_physical_tensor_desc_infer_fn = 1;
  let has_get_sbp_fn = 1;
  let has_data_type_infer_fn = 1;
  let has_input_arg_modify_fn = 1;
}

// Its gradient in b: db [K, N], summed over the transposed CSR (a_csr_row_ptr [K+1], a_csr_col_idx
// = the rows of A, perm: csr_transpose's outputs) with the bits of spmm_csr on unit values.
def OneFlow_SpmmCsrEdgeGradBOp : OneFlow_BaseOp<"spmm_csr_edge_grad_b", [NoSideEffect, DeclareOpInterfaceMethods<UserOpCompatibleInterface>]> {
  let input = (ins
    OneFlow_Tensor:$a_csr_row_ptr,
    OneFlow_Tensor:$a_csr_col_idx,
    OneFlow_Tensor:$perm,
    OneFlow_Tensor:$e,
    OneFlow_Tensor:$b,
    OneFlow_Tensor:$dy
  );
  let output = (outs
    OneFlow_Tensor:$db
  );
  let attrs = (ins
    DefaultValuedAttr<SI64Attr, "0">:$op,
    DefaultValuedAttr<SI64Attr, "0">:$act
  );
  let has_logical_tensor_desc_infer_fn = 1;
  let has_physical_tensor_desc_infer_fn = 1;
  let has_get_sbp_fn = 1;
  let has_data_type_infer_fn = 1;
  let has_input_arg_modify_fn = 1;
}

// The multi-aggregator SpMM: the aggregators of aggr_mask (bit 0 sum, 1 mean, 2 max, 3 min, 4 var,
// 5 std) of the messages values[j] * b[col[j], :] of every row, from one walk of the CSR, as column
// blocks of width N of out [M, A*N] in ascending bit order; arg_max / arg_min [M, N] (empty without
// max / min) hold the winning global nonzero index.  var = E[p^2] - E[p]^2 clamped at 0 in the
// accumulation type, std = sqrt(var + eps).  SBP: the row split of spmm_csr_reduce.
def OneFlow_SpmmCsrMultiOp : OneFlow_BaseOp<"spmm_csr_multi", [NoSideEffect, DeclareOpInterfaceMethods<UserOpCompatibleInterface>]> {
  let input = (ins
    OneFlow_Tensor:$a_csr_row_ptr,
    OneFlow_Tensor:$a_csr_col_idx,
    OneFlow_Tensor:$a_csr_values,
    OneFlow_Tensor:$b
  );
  let output = (outs
    OneFlow_Tensor:$out,
    OneFlow_Tensor:$arg_max,
    OneFlow_Tensor:$arg_min
  );
  let attrs = (ins
    DefaultValuedAttr<SI64Attr, "0">:$a_num_rows,
    DefaultValuedAttr<SI64Attr, "0">:$a_num_cols,
    DefaultValuedAttr<SI64Attr, "0">:$aggr_mask,
    DefaultValuedAttr<F64Attr, "1e-5">:$eps
  );
  let has_logical_tensor_desc_infer_fn = 1;
  let has_physical_tensor_desc_infer_fn = 1;
  let has_get_sbp_fn = 1;
  let has_data_type_infer_fn = 1;
  let has_input_arg_modify_fn = 1;
}

// The segment matmul: out[i, :] = x[row(i), :] @ W[t] for seg_ptr[t] <= i < seg_ptr[t+1], with
// row(i) = idx[i] (optional input) or i: the typed linear transform of RGCN / HGT / HeteroLinear
// over rows sorted by type.  w is the [T, F_in, F_out] stack viewed [T*F_in, F_out]; with trans_w
// the [T, F_out, F_in] stack viewed [T*F_out, F_in], read as its transpose.  f32 products and sums,
// one rounding; float, float16, bfloat16.  SBP: all-broadcast.
def OneFlow_SegmentMatmulOp : OneFlow_BaseOp<"segment_matmul", [NoSideEffect, DeclareOpInterfaceMethods<UserOpCompatibleInterface>]> {
  let input = (ins
    OneFlow_Tensor:$x,
    OneFlow_Tensor:$w,
    OneFlow_Tensor:$seg_ptr,
    Optional<OneFlow_Tensor>:$idx
  );
  let output = (outs
    OneFlow_Tensor:$out
  );
  let attrs = (ins
    DefaultValuedAttr<SI64Attr, "0">:$trans_w
  );
  let has_logical_tensor_desc_infer_fn = 1;
  let has_physical_tensor_desc_infer_fn = 1;
  let has_get_sbp_fn = 1;
  let has_data_type_infer_fn = 1;
  let has_input_arg_modify_fn = 1;
}

// Its gradient in w from the upstream dy [S, F_out]: dw[t] = the sum over the segment's rows of
// x[row(i), :]^T dy[i, :], as [T*F_in, F_out]; parts: the row parts of the launch (0 = from the
// shapes), whose partial sums are added in ascending order.
def OneFlow_SegmentMatmulGradWOp : OneFlow_BaseOp<"segment_matmul_grad_w", [NoSideEffect, DeclareOpInterfaceMethods<UserOpCompatibleInterface>]> {
  let input = (ins
    OneFlow_Tensor:$x,
    OneFlow_Tensor:$dy,
    OneFlow_Tensor:$seg_ptr,
    Optional<OneFlow_Tensor>:$idx
  );
  let output = (outs
    OneFlow_Tensor:$dw
  );
  let attrs = (ins
    DefaultValuedAttr<SI64Attr, "0">:$parts
  );
  let has_logical_tensor_desc_infer_fn = 1;
  let has_physical_tensor_desc_infer_fn = 1;
  let has_get_sbp_fn = 1;
  let has_data_type_infer_fn = 1;
  let has_input_arg_modify_fn = 1;
}

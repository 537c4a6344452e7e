"""oneflow_spmm — MI355X-native `spmm_csr` operator with OneFlow's user-op surface.

    import oneflow_spmm as flow_spmm
    out = flow_spmm.spmm(row_ptr, col_idx, values, num_rows, num_cols, b)   # oneflow.spmm
    out = flow_spmm._C.spmm_csr(...)                                          # oneflow._C.spmm_csr
`spmm` is differentiable in the values and in b (autograd.py: SDDMM and A^T @ dC).
    out = flow_spmm.spmm(..., reduce="max")            # "sum" (default), "mean", "max", "min"
    out, arg = flow_spmm.spmm_reduce(..., reduce="max")  # arg: the winning nonzero per element
    y = flow_spmm.edge_softmax(row_ptr, col_idx, e)    # softmax of per-edge scores over each row
Multi-head graph attention (q, k, v as [rows, H, D]; scores and weights as [nnz, H]):
    e = flow_spmm.sddmm(row_ptr, col_idx, q, k)        # [nnz, H], one launch for all heads
    w = flow_spmm.edge_softmax(row_ptr, col_idx, e)    # [nnz, H], one launch for all heads
    out = flow_spmm.spmm(row_ptr, col_idx, w, M, K, v) # [M, H, D], one launch for all heads
or the three through one op (one fused kernel for the rows below the hub threshold), with the same
bits and the same gradients:
    out = flow_spmm.graph_attention(row_ptr, col_idx, q, k, v)   # return_attention=True: (out, w)
The original GAT layer (additive scores s_row [M, H] + s_col [K, H], LeakyReLU, softmax) in one launch:
    w = flow_spmm.gat_softmax(row_ptr, col_idx, s_row, s_col, negative_slope=0.2)   # [nnz, H]
    out = flow_spmm.gat_attention(row_ptr, col_idx, s_row, s_col, v)                 # [M, H, D]
GATv2 (x_row [M, H, D], x_col [K, H, D], att [H, D]; LeakyReLU between the gather and the dot product):
    e = flow_spmm.gatv2_scores(row_ptr, col_idx, x_row, x_col, att, negative_slope=0.2)   # [nnz, H]
    w = flow_spmm.gatv2_softmax(row_ptr, col_idx, x_row, x_col, att)                 # [nnz, H]
    out = flow_spmm.gatv2_attention(row_ptr, col_idx, x_row, x_col, att)             # [M, H, D]
A feature table stored in FP8 (torch.float8_e4m3fn / float8_e5m2) with a float32 scale per row:
    b_q, b_scale = flow_spmm.quantize_rows_fp8(b)                                    # one-off
    out = flow_spmm.spmm_fp8(row_ptr, col_idx, values, M, K, b_q, b_scale)           # [M, N] / [M, H, D]
A mini-batch: at most `fanout` sampled in-neighbours of each seed node, as a CSR the ops above take:
    rp_s, ci_s, eid = flow_spmm.sample_neighbors(row_ptr, col_idx, seeds, fanout, seed=0)
Graph mode (UserKernel's CUDA-graph branch) is the compiled job's native hipGraph executable:
`ccl.SpmmJob(..., graph=True)` over `ofx_spmm_job_set_graph`.

Re-exports mirror python/oneflow/__init__.py:158-160 (`from oneflow._C import ... as mv`).
"""
from . import _C, _lib, autograd, build, ops, sampling, synth  # noqa: F401
from ._C import spmm_csr, spmm_csr_reduce
from ._lib import OfxError
from .autograd import (csr_transpose, edge_softmax, fused_spmm, gat_attention, gat_softmax,
                       gatv2_attention, gatv2_scores, gatv2_softmax, graph_attention,
                       quantize_rows_fp8, sddmm, spmm, spmm_fp8, spmm_reduce)
from .build import coo_to_csr
from .sampling import sample_blocks, sample_neighbors

__version__ = _lib.LIB.ofx_version().decode()

__all__ = ["spmm", "spmm_fp8", "quantize_rows_fp8", "spmm_reduce", "edge_softmax", "graph_attention", "gat_softmax", "gat_attention", "gatv2_scores", "gatv2_softmax", "gatv2_attention", "fused_spmm", "spmm_csr", "spmm_csr_reduce", "sddmm", "csr_transpose", "OfxError", "ops", "synth", "autograd", "coo_to_csr", "sample_neighbors", "sample_blocks", "sampling", "_C"]

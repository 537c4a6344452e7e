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
A feature vector per edge (e [nnz, N]; GINE with op="add", act="relu"; CFConv / MPNN with op="mul"):
    out = flow_spmm.spmm_edge(row_ptr, col_idx, e, M, K, b, op="mul", act=None)      # [M, N]
Several aggregators of the same messages from one gather (PNA, PyG's MultiAggregation):
    out = flow_spmm.spmm_multi(row_ptr, col_idx, values, M, K, b,
                               aggrs=("mean", "max", "min", "std"), eps=1e-5)        # [M, A, N]
A typed linear transform over rows sorted by type (RGCN, HGT, HeteroLinear; idx gathers the rows):
    out = flow_spmm.segment_matmul(x, w, seg_ptr, idx=None, trans_w=False)           # [S, F_out]
A mini-batch: at most `fanout` sampled in-neighbours of each seed node, as a CSR the ops above take:
    rp_s, ci_s, eid = flow_spmm.sample_neighbors(row_ptr, col_idx, seeds, fanout, seed=0)
and its block: the distinct ids of seeds and columns in order, and both relabelled to positions in it:
    src, col_local, seed_pos = flow_spmm.compact_block(seeds, ci_s, num_nodes)
The subgraph induced by a node set (ClusterGCN, GraphSAINT, ShaDow batches), relabelled to the set:
    src, rp_s, col_local, eid, node_pos = flow_spmm.node_subgraph(row_ptr, col_idx, nodes)
Random walks, uniform or with node2vec's p and q, and the subgraph they induce (GraphSAINT-RW):
    walks, eid = flow_spmm.random_walk(row_ptr, col_idx, starts, length, p=1.0, q=1.0, seed=0)
    src, rp_s, col_local, eid, node_pos = flow_spmm.random_walk_subgraph(row_ptr, col_idx, starts, 2)
The k largest (or smallest) entries of every row, as a CSR the ops take (sparse attention, kNN graphs):
    rp_s, ci_s, eid = flow_spmm.row_topk(row_ptr, col_idx, scores, k)                # scores[eid]
The product of two CSR matrices as a CSR with ascending rows (two-hop and metapath graphs, diffusion):
    rp_c, ci_c, v_c = flow_spmm.spgemm(rp_a, ci_a, v_a, rp_b, ci_b, v_b, n)          # A [M, K] @ B [K, n]
Graph mode (UserKernel's CUDA-graph branch) is the compiled job's native hipGraph executable:
`ccl.SpmmJob(..., graph=True)` over `ofx_spmm_job_set_graph`.

Re-exports mirror python/oneflow/__init__.py:158-160 (`from oneflow._C import ... as mv`).
"""
from . import _C, _lib, autograd, build, ops, sampling, synth  # noqa: F401
from ._C import spmm_csr, spmm_csr_reduce
from ._lib import OfxError
from .autograd import (csr_transpose, edge_softmax, fused_spmm, gat_attention, gat_softmax,
                       gatv2_attention, gatv2_scores, gatv2_softmax, graph_attention,
                       quantize_rows_fp8, sddmm, segment_matmul, spmm, spmm_edge, spmm_fp8,
                       spmm_multi, spmm_reduce)
from .build import coo_to_csr, spgemm
from .sampling import (compact_block, node_subgraph, random_walk, random_walk_subgraph, row_topk,
                       sample_blocks, sample_neighbors)

__version__ = _lib.LIB.ofx_version().decode()

__all__ = ["spmm", "segment_matmul", "spmm_edge", "spmm_multi", "spmm_fp8", "quantize_rows_fp8", "spmm_reduce", "edge_softmax", "graph_attention", "gat_softmax", "gat_attention", "gatv2_scores", "gatv2_softmax", "gatv2_attention", "fused_spmm", "spmm_csr", "spmm_csr_reduce", "sddmm", "csr_transpose", "OfxError", "ops", "synth", "autograd", "coo_to_csr", "spgemm", "sample_neighbors", "sample_blocks", "compact_block", "node_subgraph", "random_walk", "random_walk_subgraph", "row_topk", "sampling", "_C"]

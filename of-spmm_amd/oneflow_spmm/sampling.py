"""Neighbour sampling over CSR: the step that makes a mini-batch.  HIP kernels on
GPU tensors (csrc/sample_neighbors.hip), the kCPU kernel on CPU tensors
(csrc/sample_neighbors_cpu.cpp); integers only, the same arrays from both.

The sampled CSR feeds the ops as it is: its rows are the seeds, its columns stay global node ids,
so `spmm(rp_s, ci_s, vals, S, K, b)` runs on the full feature table (FP8 tables included) and the
edge ids select the sampled entries of any per-edge tensor, `values[edge_ids]`."""
from __future__ import annotations

import ctypes

import torch

from ._C import current_stream_handle, dtype_code
from ._lib import LIB, check

MAX_FANOUT = 64


def sample_neighbors(row_ptr: torch.Tensor, col_idx: torch.Tensor, seeds: torch.Tensor, fanout: int,
                     *, seed: int = 0, return_edge_ids: bool = True, num_threads: int = 0):
    """Returns (row_ptr_s [S+1], col_idx_s [nnz_s], edge_ids [nnz_s] or None): row i holds
    min(deg, fanout) entries of row seeds[i], in ascending position order (a sorted CSR stays
    sorted), col_idx_s = col_idx[edge_ids].  A row longer than `fanout` keeps a uniform subset
    without replacement (Floyd's algorithm over philox4x32-10 keyed by `seed`, taken mod 2^64, and
    the node id): a node's sample under one seed does not depend on the batch, and the CPU and the
    GPU give the same arrays.  1 <= fanout <= 64.  The three index tensors share one dtype (int32 or
    int64) and one device, which chooses the kernel; num_threads is the kCPU kernel's (0: OpenMP's
    own count)."""
    for name, t in (("row_ptr", row_ptr), ("col_idx", col_idx), ("seeds", seeds)):
        if not isinstance(t, torch.Tensor) or t.dim() != 1:
            raise RuntimeError(f"sample_neighbors: {name} must be a 1-D tensor")
    if row_ptr.numel() < 1:
        raise RuntimeError("sample_neighbors: row_ptr must hold at least one entry")
    if not (row_ptr.dtype == col_idx.dtype == seeds.dtype):
        raise TypeError("sample_neighbors: row_ptr, col_idx and seeds must have the same index dtype")
    if not (row_ptr.device == col_idx.device == seeds.device):
        raise RuntimeError("sample_neighbors: row_ptr, col_idx and seeds must be on one device")
    row_ptr, col_idx, seeds = row_ptr.contiguous(), col_idx.contiguous(), seeds.contiguous()
    if col_idx.numel() == 0:  # a graph without edges: never read, but the C-ABI refuses NULL
        col_idx = col_idx.new_zeros(1)
    it, dev = row_ptr.dtype, row_ptr.device
    idt = dtype_code(it)
    m, s = row_ptr.numel() - 1, seeds.numel()
    fanout = int(fanout)
    bound = s * min(max(fanout, 0), MAX_FANOUT)
    seed = ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    out_rp = torch.empty(s + 1, dtype=it, device=dev)
    out_ci = torch.empty(bound, dtype=it, device=dev)
    out_eid = torch.empty(bound, dtype=it, device=dev) if return_edge_ids else None
    # outputs of `bound` entries are passed even when empty: NULL is for "no edge ids" alone
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    if dev.type == "cpu":
        cnt = ctypes.c_int64(0)
        check(LIB.ofx_sample_neighbors_cpu(int(num_threads), idt, m, s, ptr(row_ptr), ptr(col_idx),
                                           ptr(seeds), fanout, seed, ptr(out_rp), ptr(out_ci),
                                           ptr(out_eid), ctypes.byref(cnt)), "sample_neighbors")
        n_out = cnt.value
    else:
        ws_bytes = ctypes.c_size_t(0)
        check(LIB.ofx_sample_neighbors_workspace_size(idt, s, ctypes.byref(ws_bytes)),
              "sample_neighbors")
        ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8, device=dev)
        scalars = torch.zeros(2, dtype=torch.int64, device=dev)  # [nnz_s, bad flag]
        check(LIB.ofx_sample_neighbors(current_stream_handle(row_ptr), idt, m, s, ptr(row_ptr),
                                       ptr(col_idx), ptr(seeds), fanout, seed, ptr(out_rp),
                                       ptr(out_ci), ptr(out_eid), scalars.data_ptr(),
                                       scalars.data_ptr() + 8, ws.data_ptr(), ws_bytes.value),
              "sample_neighbors")
        n_out, bad = (int(x) for x in scalars.tolist())
        if bad:
            raise RuntimeError(f"sample_neighbors: a seed outside [0, {m}), or a row whose degree "
                               "is outside [0, 2^31)")
    return out_rp, out_ci[:n_out], (out_eid[:n_out] if out_eid is not None else None)


def sample_blocks(row_ptr: torch.Tensor, col_idx: torch.Tensor, seeds: torch.Tensor, fanouts, *,
                  seed: int = 0):
    """The blocks of a multi-layer mini-batch, input layer first.  `fanouts` is given input layer
    first too (GraphSAGE's order) and layer l draws with seed + l: the last layer samples from
    `seeds`, each earlier one from the source nodes of the layer after it.  A block is
    (row_ptr_s, col_local, edge_ids, src, seed_pos):
      src       sorted unique global ids of the block's seeds and sampled neighbours: its inputs
      col_local the block's columns as positions in src; seed_pos the block's seeds likewise
    so that one layer is `spmm(row_ptr_s, col_local, vals, len(seed_pos), len(src), h_src)` with
    h_src the features of src, and the next layer's h_src is that result (its rows are this block's
    seeds, which are the next block's src).  Plain torch around `sample_neighbors`."""
    blocks = []
    cur = seeds
    fanouts = list(fanouts)
    for layer in reversed(range(len(fanouts))):  # from the output layer outwards
        rp_s, ci_s, eid = sample_neighbors(row_ptr, col_idx, cur, fanouts[layer], seed=seed + layer)
        src = torch.unique(torch.cat((cur, ci_s)))
        col_local = torch.searchsorted(src, ci_s).to(ci_s.dtype)
        seed_pos = torch.searchsorted(src, cur)
        blocks.append((rp_s, col_local, eid, src, seed_pos))
        cur = src
    return blocks[::-1]

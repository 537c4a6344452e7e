"""Neighbour sampling over CSR, block compaction, the subgraph induced by a node set, random walks
and per-row top-k selection: the steps that make a mini-batch or prune a graph (DESIGN.md §3k, §3l,
§3m, §3n, §3o).  HIP kernels on GPU tensors (csrc/sample_neighbors.hip, csrc/compact_ids.hip,
csrc/node_subgraph.hip, csrc/random_walk.hip, csrc/row_topk.hip), the kCPU kernels on CPU tensors
(csrc/sample_neighbors_cpu.cpp, csrc/compact_ids_cpu.cpp, csrc/node_subgraph_cpu.cpp,
csrc/random_walk_cpu.cpp, csrc/row_topk_cpu.cpp); integers only, the same arrays from both.

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


def compact_block(seeds: torch.Tensor, cols: torch.Tensor, num_nodes: int, *, num_threads: int = 0):
    """Returns (src, col_local, seed_pos) for node ids in [0, num_nodes): src holds the distinct
    values of seeds ∪ cols in ascending order, col_local[j] is the position of cols[j] in src (both
    in the input dtype) and seed_pos[i] the position of seeds[i] (int64): what
    `torch.unique(torch.cat((seeds, cols)))` and two `torch.searchsorted` calls give, from a bitmap
    over the node ids with rank and select instead of a sort.  seeds and cols are 1-D, share one
    index dtype (int32 or int64) and one device, which chooses the kernel; either may be empty.
    0 <= num_nodes < 2^31 and len(seeds) + len(cols) < 2^31.  An id outside [0, num_nodes) raises
    RuntimeError ("outside"); it is never used as an address.  num_threads is the kCPU kernel's
    (0: OpenMP's own count) and does not change the result."""
    for name, t in (("seeds", seeds), ("cols", cols)):
        if not isinstance(t, torch.Tensor) or t.dim() != 1:
            raise RuntimeError(f"compact_block: {name} must be a 1-D tensor")
    if seeds.dtype != cols.dtype:
        raise TypeError("compact_block: seeds and cols must have the same index dtype")
    if seeds.device != cols.device:
        raise RuntimeError("compact_block: seeds and cols must be on one device")
    seeds, cols = seeds.contiguous(), cols.contiguous()
    it, dev = seeds.dtype, seeds.device
    idt = dtype_code(it)
    num_nodes, s, e = int(num_nodes), seeds.numel(), cols.numel()
    ws_bytes = ctypes.c_size_t(0)
    if dev.type != "cpu":  # refuses bad sizes before anything is allocated
        check(LIB.ofx_compact_ids_workspace_size(idt, num_nodes, s, e, ctypes.byref(ws_bytes)),
              "compact_block")
    src = torch.empty(max(min(s + e, num_nodes), 0), dtype=it, device=dev)
    col_local = torch.empty(e, dtype=it, device=dev)
    seed_pos = torch.empty(s, dtype=torch.int64, device=dev)
    ptr = lambda t: t.data_ptr() if t.numel() else None  # noqa: E731
    if dev.type == "cpu":
        cnt = ctypes.c_int64(0)
        check(LIB.ofx_compact_ids_cpu(int(num_threads), idt, num_nodes, s, ptr(seeds), e, ptr(cols),
                                      ptr(src), ptr(seed_pos), ptr(col_local), ctypes.byref(cnt)),
              "compact_block")
        count = cnt.value
    else:
        ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8, device=dev)
        scalars = torch.zeros(2, dtype=torch.int64, device=dev)  # [count, bad flag]
        check(LIB.ofx_compact_ids(current_stream_handle(seeds), idt, num_nodes, s, ptr(seeds), e,
                                  ptr(cols), ptr(src), ptr(seed_pos), ptr(col_local),
                                  scalars.data_ptr(), scalars.data_ptr() + 8, ws.data_ptr(),
                                  ws_bytes.value), "compact_block")
        count, bad = (int(x) for x in scalars.tolist())
        if bad:
            raise RuntimeError(f"compact_block: an id outside [0, {num_nodes})")
    return src[:count], col_local, seed_pos


def node_subgraph(row_ptr: torch.Tensor, col_idx: torch.Tensor, nodes: torch.Tensor, *,
                  return_edge_ids: bool = True, num_threads: int = 0):
    """The subgraph induced by a node set (ClusterGCN, GraphSAINT's node sampler, ShaDow batches).
    Returns (src, row_ptr_s, col_local, edge_ids, node_pos): src holds the distinct values of
    `nodes` in ascending order; row r of the CSR (row_ptr_s [C+1], col_local) belongs to node
    src[r] and keeps, in their order, the entries of that row of the input whose column is a member
    of src, as positions in src; edge_ids holds their places in col_idx (ascending over the whole
    output, None with return_edge_ids=False) and node_pos[i] (int64) is the position of nodes[i] in
    src.  So `spmm(row_ptr_s, col_local, values[edge_ids], C, C, h[src])` is a layer on the batch.
    The other outputs are in the input dtype.  `nodes` is 1-D, in any order, may repeat and may be
    empty; row_ptr, col_idx and nodes share one index dtype (int32 or int64) and one device, which
    chooses the kernel.  A column outside [0, M) (a non-square CSR) is no member and is dropped.  An
    id in nodes outside [0, M), or a selected row whose entry range is no row's, raises RuntimeError
    ("outside"); neither is ever used as an address.  M, nnz and len(nodes) are below 2^31.
    num_threads is the kCPU kernel's (0: OpenMP's own count) and does not change the result."""
    for name, t in (("row_ptr", row_ptr), ("col_idx", col_idx), ("nodes", nodes)):
        if not isinstance(t, torch.Tensor) or t.dim() != 1:
            raise RuntimeError(f"node_subgraph: {name} must be a 1-D tensor")
    if row_ptr.numel() < 1:
        raise RuntimeError("node_subgraph: row_ptr must hold at least one entry")
    if not (row_ptr.dtype == col_idx.dtype == nodes.dtype):
        raise TypeError("node_subgraph: row_ptr, col_idx and nodes must have the same index dtype")
    if not (row_ptr.device == col_idx.device == nodes.device):
        raise RuntimeError("node_subgraph: row_ptr, col_idx and nodes must be on one device")
    row_ptr, col_idx, nodes = row_ptr.contiguous(), col_idx.contiguous(), nodes.contiguous()
    it, dev = row_ptr.dtype, row_ptr.device
    idt = dtype_code(it)
    m, nnz, s = row_ptr.numel() - 1, col_idx.numel(), nodes.numel()
    ws_bytes = ctypes.c_size_t(0)
    if dev.type != "cpu":  # refuses bad sizes before anything is allocated
        check(LIB.ofx_node_subgraph_workspace_size(idt, m, nnz, s, ctypes.byref(ws_bytes)),
              "node_subgraph")
    src = torch.empty(min(s, m), dtype=it, device=dev)
    node_pos = torch.empty(s, dtype=torch.int64, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
    new = lambda n: torch.empty(n, dtype=it, device=dev)  # noqa: E731
    if dev.type == "cpu":
        counts = (ctypes.c_int64 * 2)(0, 0)
        rp_s = new(min(s, m) + 1)
        check(LIB.ofx_node_subgraph_count_cpu(int(num_threads), idt, m, nnz, s, ptr(row_ptr),
                                              ptr(col_idx), ptr(nodes), ptr(src), ptr(node_pos),
                                              ptr(rp_s), counts), "node_subgraph")
        count, nnz_s = counts[0], counts[1]
        src, rp_s = src[:count], rp_s[:count + 1]
        col_local, eid = new(nnz_s), (new(nnz_s) if return_edge_ids else None)
        check(LIB.ofx_node_subgraph_fill_cpu(int(num_threads), idt, m, nnz, s, count, nnz_s,
                                             ptr(row_ptr), ptr(col_idx), ptr(src), ptr(rp_s),
                                             ptr(col_local), ptr(eid)), "node_subgraph")
        return src, rp_s, col_local, eid, node_pos
    stream = current_stream_handle(row_ptr)
    ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8, device=dev)
    scalars = torch.zeros(3, dtype=torch.int64, device=dev)  # [C, nnz_s, bad flag]
    check(LIB.ofx_node_subgraph_count(stream, idt, m, nnz, s, ptr(row_ptr), ptr(col_idx), ptr(nodes),
                                      ptr(src), ptr(node_pos), scalars.data_ptr(),
                                      scalars.data_ptr() + 16, ws.data_ptr(), ws_bytes.value),
          "node_subgraph")
    count, nnz_s, bad = (int(x) for x in scalars.tolist())  # the one read-back
    if bad:
        raise RuntimeError(f"node_subgraph: a node outside [0, {m}), or a selected row whose "
                           f"degree is outside [0, 2^31) or whose entries are outside [0, {nnz})")
    src = src[:count]
    rp_s, col_local = new(count + 1), new(nnz_s)
    eid = new(nnz_s) if return_edge_ids else None
    check(LIB.ofx_node_subgraph_fill(stream, idt, m, nnz, s, count, nnz_s, ptr(row_ptr), ptr(col_idx),
                                     ptr(src), ptr(rp_s), ptr(col_local), ptr(eid), ws.data_ptr(),
                                     ws_bytes.value), "node_subgraph")
    return src, rp_s, col_local, eid, node_pos


def random_walk(row_ptr: torch.Tensor, col_idx: torch.Tensor, starts: torch.Tensor, length: int, *,
                p: float = 1.0, q: float = 1.0, seed: int = 0, return_edge_ids: bool = False,
                num_threads: int = 0):
    """Returns (walks [S, length + 1], edge_ids [S, length] or None): walks[i, 0] = starts[i] and
    every further entry a neighbour of the one before, drawn uniformly (p == q == 1) or with
    node2vec's bias against the node two steps back: weight 1/p for returning to it, 1 for one of
    its neighbours, 1/q for any other node, by rejection over philox4x32-10 keyed by `seed` (taken
    mod 2^64) and counted by the walk's index i, the step and the attempt.  edge_ids holds each
    step's place in col_idx.  A walk that reaches a node without a row or without entries ends:
    the rest of its row is -1 in both outputs.  `starts` may repeat (every walk is its own) and may
    be empty; a walk depends on (seed, i, starts[i]) alone, and the CPU and the GPU give the same
    arrays.  1 <= length <= 65535; p and q finite and > 0.  The three index tensors are 1-D and share
    one dtype (int32 or int64) and one device, which chooses the kernel; the outputs have both.  A
    start outside [0, M), or a row a walk reads whose degree is outside [0, 2^31) or whose entries
    are outside [0, nnz), raises RuntimeError ("outside"); neither is ever used as an address.  The
    neighbour test assumes rows with ascending columns (what `coo_to_csr` emits).  num_threads is
    the kCPU kernel's (0: OpenMP's own count) and does not change the result."""
    for name, t in (("row_ptr", row_ptr), ("col_idx", col_idx), ("starts", starts)):
        if not isinstance(t, torch.Tensor) or t.dim() != 1:
            raise RuntimeError(f"random_walk: {name} must be a 1-D tensor")
    if row_ptr.numel() < 1:
        raise RuntimeError("random_walk: row_ptr must hold at least one entry")
    if not (row_ptr.dtype == col_idx.dtype == starts.dtype):
        raise TypeError("random_walk: row_ptr, col_idx and starts must have the same index dtype")
    if not (row_ptr.device == col_idx.device == starts.device):
        raise RuntimeError("random_walk: row_ptr, col_idx and starts must be on one device")
    row_ptr, col_idx, starts = row_ptr.contiguous(), col_idx.contiguous(), starts.contiguous()
    it, dev = row_ptr.dtype, row_ptr.device
    idt = dtype_code(it)
    m, nnz, s = row_ptr.numel() - 1, col_idx.numel(), starts.numel()
    length = int(length)
    steps = min(max(length, 0), 65535)  # the entry refuses a length outside [1, 65535]
    seed = ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    walks = torch.empty((s, steps + 1), dtype=it, device=dev)
    eid = torch.empty((s, steps), dtype=it, device=dev) if return_edge_ids else None
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
    if dev.type == "cpu":
        check(LIB.ofx_random_walk_cpu(int(num_threads), idt, m, nnz, s, ptr(row_ptr), ptr(col_idx),
                                      ptr(starts), length, float(p), float(q), seed, ptr(walks),
                                      ptr(eid)), "random_walk")
        return walks, eid
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    check(LIB.ofx_random_walk(current_stream_handle(row_ptr), idt, m, nnz, s, ptr(row_ptr),
                              ptr(col_idx), ptr(starts), length, float(p), float(q), seed,
                              ptr(walks), ptr(eid), bad.data_ptr()), "random_walk")
    if int(bad.item()):  # the one read-back
        raise RuntimeError(f"random_walk: a start outside [0, {m}), or a walk read a row whose "
                           f"degree is outside [0, 2^31) or whose entries are outside [0, {nnz})")
    return walks, eid


def random_walk_subgraph(row_ptr: torch.Tensor, col_idx: torch.Tensor, starts: torch.Tensor,
                         length: int, *, p: float = 1.0, q: float = 1.0, seed: int = 0,
                         return_edge_ids: bool = True, num_threads: int = 0):
    """GraphSAINT's random-walk batch: `node_subgraph` of the nodes the walks of `random_walk`
    visit (the entries >= 0 of `walks`, flattened), with its five outputs."""
    walks, _ = random_walk(row_ptr, col_idx, starts, length, p=p, q=q, seed=seed,
                           num_threads=num_threads)
    nodes = walks.reshape(-1)
    return node_subgraph(row_ptr, col_idx, nodes[nodes >= 0], return_edge_ids=return_edge_ids,
                         num_threads=num_threads)


def row_topk(row_ptr: torch.Tensor, col_idx: torch.Tensor, values: torch.Tensor, k: int, *,
             largest: bool = True, num_threads: int = 0):
    """Returns (row_ptr_s [M+1], col_idx_s [nnz_s], edge_ids [nnz_s]): row i keeps the min(deg, k)
    entries of row i with the largest values (the smallest with largest=False), in ascending
    position order (a sorted CSR stays sorted and the ops take the result as it is); edge_ids holds
    their places in col_idx, col_idx_s = col_idx[edge_ids], and the kept values are
    `values[edge_ids]`, which carries the gradient.  Sparse attention between `sddmm` and
    `edge_softmax`, kNN graphs, pruned diffusion matrices, TopKPooling.  Weighted sampling without
    replacement of `fanout` neighbours is Gumbel top-k:
        g = -torch.log(-torch.log(torch.rand_like(w)))
        rp_s, ci_s, eid = row_topk(row_ptr, col_idx, torch.log(w) + g, fanout)
    The order is that of the bit pattern: -0 < +0, a NaN with the sign clear ranks above +inf
    (where torch.topk puts it), equal values go to the lower position: every output is a function
    of the input bits, and the CPU and the GPU give the same arrays.  `values` is 1-D [nnz] in
    float32, float64, float16 or bfloat16; row_ptr and col_idx share one index dtype (int32 or
    int64); all three share one device, which chooses the kernel.  k >= 1, without an upper bound;
    a row with deg <= k is copied whole.  M and nnz are below 2^31.  A row whose degree is outside
    [0, 2^31) or whose entries are outside [0, nnz) raises RuntimeError ("outside"); it is never
    used as an address.  num_threads is the kCPU kernel's (0: OpenMP's own count) and does not
    change the result."""
    for name, t in (("row_ptr", row_ptr), ("col_idx", col_idx), ("values", values)):
        if not isinstance(t, torch.Tensor) or t.dim() != 1:
            raise RuntimeError(f"row_topk: {name} must be a 1-D tensor")
    if row_ptr.numel() < 1:
        raise RuntimeError("row_topk: row_ptr must hold at least one entry")
    if row_ptr.dtype != col_idx.dtype:
        raise TypeError("row_topk: row_ptr and col_idx must have the same index dtype")
    if not (row_ptr.device == col_idx.device == values.device):
        raise RuntimeError("row_topk: row_ptr, col_idx and values must be on one device")
    if values.numel() != col_idx.numel():
        raise RuntimeError(f"row_topk: {values.numel()} values for {col_idx.numel()} entries")
    k = int(k)
    if k < 1:
        raise RuntimeError(f"row_topk: k {k} is not >= 1")
    row_ptr, col_idx, values = row_ptr.contiguous(), col_idx.contiguous(), values.detach().contiguous()
    it, dev = row_ptr.dtype, row_ptr.device
    idt, vdt = dtype_code(it), dtype_code(values.dtype)
    m, nnz = row_ptr.numel() - 1, col_idx.numel()
    ws_bytes = ctypes.c_size_t(0)
    if dev.type != "cpu":  # refuses bad sizes before anything is allocated
        check(LIB.ofx_row_topk_workspace_size(idt, m, nnz, ctypes.byref(ws_bytes)), "row_topk")
    bound = min(nnz, m * k)
    out_rp = torch.empty(m + 1, dtype=it, device=dev)
    out_ci = torch.empty(bound, dtype=it, device=dev)
    out_eid = torch.empty(bound, dtype=it, device=dev)
    ptr = lambda t: t.data_ptr() if t.numel() else None  # noqa: E731
    if dev.type == "cpu":
        cnt = ctypes.c_int64(0)
        check(LIB.ofx_row_topk_cpu(int(num_threads), idt, vdt, m, nnz, ptr(row_ptr), ptr(col_idx),
                                   ptr(values), k, int(bool(largest)), ptr(out_rp), ptr(out_ci),
                                   ptr(out_eid), ctypes.byref(cnt)), "row_topk")
        n_out = cnt.value
    else:
        ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8, device=dev)
        scalars = torch.zeros(2, dtype=torch.int64, device=dev)  # [nnz_s, bad flag]
        check(LIB.ofx_row_topk(current_stream_handle(row_ptr), idt, vdt, m, nnz, ptr(row_ptr),
                               ptr(col_idx), ptr(values), k, int(bool(largest)), ptr(out_rp),
                               ptr(out_ci), ptr(out_eid), scalars.data_ptr(),
                               scalars.data_ptr() + 8, ws.data_ptr(), ws_bytes.value), "row_topk")
        n_out, bad = (int(x) for x in scalars.tolist())  # the one read-back
        if bad:
            raise RuntimeError("row_topk: a row whose degree is outside [0, 2^31) or whose "
                               f"entries are outside [0, {nnz})")
    return out_rp, out_ci[:n_out], out_eid[:n_out]


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
    seeds, which are the next block's src).  `sample_neighbors`, then `compact_block` over the
    graph's rows.  A non-square CSR whose columns reach past its row count has ids that
    `compact_block` refuses: such a layer takes the torch route (`unique` and `searchsorted`), which
    gives the same arrays without a bound on the ids."""
    blocks = []
    cur = seeds
    fanouts = list(fanouts)
    for layer in reversed(range(len(fanouts))):  # from the output layer outwards
        rp_s, ci_s, eid = sample_neighbors(row_ptr, col_idx, cur, fanouts[layer], seed=seed + layer)
        try:
            src, col_local, seed_pos = compact_block(cur, ci_s, row_ptr.numel() - 1)
        except RuntimeError as err:
            if "outside" not in str(err):
                raise
            src = torch.unique(torch.cat((cur, ci_s)))
            col_local = torch.searchsorted(src, ci_s).to(ci_s.dtype)
            seed_pos = torch.searchsorted(src, cur)
        blocks.append((rp_s, col_local, eid, src, seed_pos))
        cur = src
    return blocks[::-1]

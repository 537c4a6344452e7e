"""oneflow_spmm._C — the functional binding `spmm_csr`, mirroring `oneflow._C.spmm_csr`.

Signature (functional YAML entry, pattern oneflow/core/functional/functional_api.yaml:1062-1065):
    "Tensor (Tensor a_csr_row_ptr, Tensor a_csr_col_idx, Tensor a_csr_values,
             Int64 a_num_rows, Int64 a_num_cols, Tensor b) => SpmmCsr"
Tensors are torch tensors (PyTorch-ROCm supplies device memory and streams); the call goes
through the C-ABI into the C++ op registry (oneflow/user/ops/spmm_op.cpp inference, kernel
choice, Compute) and launches the HIP kernel on torch's current stream.  CPU tensors run the
op's DeviceType::kCPU kernel (the reference registers CPU kernels the same way); GPU tensors run
only the HIP kernel — there is no fallback between them.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import LIB, TensorDesc, check

_TORCH_TO_DT = {
    torch.float32: _lib.DT_FLOAT,
    torch.float64: _lib.DT_DOUBLE,
    torch.float16: _lib.DT_FLOAT16,
    torch.bfloat16: _lib.DT_BFLOAT16,
    torch.int32: _lib.DT_INT32,
    torch.int64: _lib.DT_INT64,
}
_DT_TO_TORCH = {v: k for k, v in _TORCH_TO_DT.items()}


def dtype_code(dt: torch.dtype) -> int:
    try:
        return _TORCH_TO_DT[dt]
    except KeyError:
        raise TypeError(f"spmm_csr: unsupported dtype {dt}") from None


def _device_index(t: torch.Tensor) -> int:
    if t.device.type == "cpu":
        return -1
    if t.device.type != "cuda":  # PyTorch-ROCm names HIP devices "cuda"
        raise RuntimeError(f"spmm_csr: unsupported device {t.device}")
    return t.device.index if t.device.index is not None else torch.cuda.current_device()


def _prep(t: torch.Tensor, name: str, matrix: bool = False) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"spmm_csr: {name} must be a tensor, got {type(t).__name__}")
    if matrix and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]:
        return t  # row-strided views are consumed in place (ldb)
    return t.contiguous()


def _csr_pair(row_ptr: torch.Tensor, col_idx: torch.Tensor):
    """The two index tensors of a CSR, prepared."""
    return _prep(row_ptr, "a_csr_row_ptr"), _prep(col_idx, "a_csr_col_idx")


def desc(t: torch.Tensor) -> TensorDesc:
    d = TensorDesc()
    d.dtype = dtype_code(t.dtype)
    d.device = _device_index(t)
    d.ndim = t.dim()
    if d.ndim > 2:
        raise RuntimeError(f"spmm_csr: tensors must be 1-D or 2-D, got {t.dim()}-D")
    for i in range(t.dim()):
        d.shape[i] = t.shape[i]
        d.stride[i] = t.stride(i)
    d.data = t.data_ptr() if t.numel() > 0 else None
    return d


def current_stream_handle(t: torch.Tensor):
    if t.device.type == "cpu":
        return None
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _refs(*tensors):
    """Pointers to the descriptors of `tensors`, as the functional entries take them."""
    return tuple([ctypes.byref(desc(t)) for t in tensors])


def _two_phase(fn, stream_of, before, outs, after=(), attrs=(), *, what=None, query_fn=None,
               size=None, host_tmp=True):
    """The two-phase call of a functional entry
        fn(stream, *before, *outs, tmp, tmp_bytes, *after, size_out, *attrs):
    the tmp size query (no stream, NULL outputs, no tmp), then the run on `stream_of`'s current
    stream with the op's tmp_buffer on its device (host memory for kCPU kernels; none at all with
    host_tmp=False).  `attrs`: trailing arguments of an `_attrs` entry; `query_fn`: the entry
    without them that answers the size query instead; `size`: a size already known (no query is
    made).  `what` names the call in an error (default: the entry's name).  Returns the size."""
    what = what or fn.__name__
    if size is None:
        got = ctypes.c_size_t(0)
        null_outs = (None,) * len(outs)
        if query_fn is None:
            rc = fn(None, *before, *null_outs, None, 0, *after, ctypes.byref(got), *attrs)
        else:
            rc = query_fn(None, *before, *null_outs, None, 0, *after, ctypes.byref(got))
        check(rc, what)
        size = got.value
    tmp = None
    if size and (host_tmp or stream_of.device.type != "cpu"):
        tmp = torch.empty(size, dtype=torch.uint8, device=stream_of.device)
    check(fn(current_stream_handle(stream_of), *before, *outs,
             tmp.data_ptr() if tmp is not None else None, size if tmp is not None else 0,
             *after, None, *attrs), what)
    return size


def _placement(_parallel, _placement_nd):
    """(hierarchy dims, out split axis per hierarchy axis, parallel_id, logical N or -1)."""
    if _placement_nd is not None:
        pl = dict(_placement_nd)
        hier = tuple(int(x) for x in pl["hierarchy"])
        axes = tuple(-1 if a in (None, "B") else (int(a[2:-1]) if isinstance(a, str) else int(a))
                     for a in pl["nd_sbp"])
        return hier, axes, int(pl["parallel_id"]), int(pl.get("logical_n", -1))
    if _parallel is None:
        return (1,), (-1,), 0, -1
    pid, pnum, axis = _parallel[:3]
    logical_n = _parallel[3] if len(_parallel) > 3 else -1
    return (int(pnum),), (int(axis),), int(pid), int(logical_n)


def _attrs_arg(static_csr: int):
    """The `attrs` argument of an `_attrs` entry: None (the op's defaults), or a pointer to an
    ofx_spmm_attrs that carries the call's static_csr."""
    if not static_csr:
        return None
    attrs = _lib.SpmmAttrs()
    attrs.static_csr = int(static_csr)
    return ctypes.byref(attrs)


def spmm_csr(a_csr_row_ptr: torch.Tensor, a_csr_col_idx: torch.Tensor,
             a_csr_values: torch.Tensor, a_num_rows: int, a_num_cols: int, b: torch.Tensor, *,
             out: torch.Tensor | None = None, _parallel=None, _placement_nd=None,
             num_threads: int = 0, static_csr: int = 0) -> torch.Tensor:
    """out[M, N] = CSR(a_csr_row_ptr, a_csr_col_idx, a_csr_values; M x K) @ b[K, N].

    static_csr (op attr, include/ofx_spmm.h ofx_spmm_attrs): non-zero (True = 1) promises that
    the CSR at these addresses is not rewritten while the process calls the op with this value;
    the HIP kernel's state then plans its work list once and every later call launches planned
    (no planner kernel).  A caller that frees a static CSR and builds another one gives the new
    one another value.  No numeric effect.

    Global form (one rank of a placement; `b` and `out` are this rank's physical tensors):
      `_parallel=(parallel_id, parallel_num, out_split_axis[, logical_n])` for a 1-D placement
      (out_split_axis 0: this rank's BalancedSplitter rows; 1: a column slice of width b.shape[1]
      out of logical_n; -1: broadcast), or
      `_placement_nd=dict(hierarchy=(R, C), nd_sbp=("S(0)", "S(1)"), parallel_id=p, logical_n=N)`
      for an N-D one.  The op's physical inference shapes `out`; the kernel's cache takes the row
      range from out's NdSbp (GetTensorSliceView4ParallelId) and the hub schedule from logical N.
    """
    rp, ci = _csr_pair(a_csr_row_ptr, a_csr_col_idx)
    vals = _prep(a_csr_values, "a_csr_values")
    bb = _prep(b, "b", matrix=True)
    d_rp, d_ci, d_v, d_b = desc(rp), desc(ci), desc(vals), desc(bb)
    hier, axes, pid, logical_n = _placement(_parallel, _placement_nd)
    c_hier = (ctypes.c_int64 * len(hier))(*hier)
    c_axes = (ctypes.c_int32 * len(axes))(*axes)
    common = (ctypes.byref(d_rp), ctypes.byref(d_ci), ctypes.byref(d_v), int(a_num_rows),
              int(a_num_cols), ctypes.byref(d_b), logical_n)
    tail = (len(hier), c_hier, c_axes, pid, int(num_threads))
    # Out shape and tmp size depend only on the signature (shapes, dtypes, strides, device,
    # attrs, placement): memoised after the first successful call, as OneFlow's eager path keeps
    # its inferred descs per op signature.  The launch below still runs the full inference.
    key = (rp.shape, ci.shape, vals.shape, bb.shape, d_rp.dtype, d_ci.dtype, d_v.dtype, d_b.dtype,
           d_b.stride[0], d_b.device, int(a_num_rows), int(a_num_cols), hier, axes, pid, logical_n,
           int(num_threads))
    memo = _SIG_MEMO.get(key)
    if out is None and memo is not None:
        out = torch.empty(memo[0], dtype=memo[1], device=bb.device)
    if out is None:
        # the physical out of this rank: the op's physical inference, through a dry run on an
        # empty descriptor (tmp size query) would not return the shape, so ask the infer entry
        # for the logical shape and apply the placement like GetPhysicalShape
        od = TensorDesc()
        check(LIB.ofx_functional_spmm_csr_infer(*common[:6], ctypes.byref(od)), "spmm_csr")
        rows, n = od.shape[0], od.shape[1]
        for i, (h, a) in enumerate(zip(hier, axes)):
            if a == 0 and h > 1 and rows > 0:
                idx = pid
                for hh in hier[i + 1:]:
                    idx //= hh
                lo, hi = balanced_range(rows, h, idx % h)
                rows = hi - lo
        out = torch.empty((rows, n), dtype=_DT_TO_TORCH[od.dtype], device=bb.device)
    tmp_bytes = _two_phase(LIB.ofx_functional_spmm_csr_global_attrs, bb, common, _refs(out), tail,
                           (_attrs_arg(static_csr),), what="spmm_csr",
                           query_fn=LIB.ofx_functional_spmm_csr_global,
                           size=memo[2] if memo is not None else None)
    if memo is None and len(_SIG_MEMO) < 4096:
        _SIG_MEMO[key] = (tuple(out.shape), out.dtype, tmp_bytes)
    return out


_SIG_MEMO: dict = {}


def static_plans(release: bool = False) -> dict:
    """The static-CSR plans the eager op states hold (ofx_spmm_static_plans): live entries,
    planner launches and calls that reused a plan; release=True frees them first -- the plans
    graph captures used included, so destroy those graphs before releasing."""
    e, p, h = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    check(LIB.ofx_spmm_static_plans(ctypes.byref(e), ctypes.byref(p), ctypes.byref(h),
                                    1 if release else 0), "spmm_static_plans")
    return {"entries": e.value, "plans": p.value, "hits": h.value}


def fused_spmm_csr(a_csr_row_ptr: torch.Tensor, a_csr_col_idx: torch.Tensor,
                   a_csr_values: torch.Tensor, a_num_rows: int, a_num_cols: int, b: torch.Tensor,
                   bias: torch.Tensor | None = None, *, relu: bool = False,
                   out: torch.Tensor | None = None, static_csr: int = 0) -> torch.Tensor:
    """Op "fused_spmm_csr": relu?(A @ b + bias?) in one kernel, the same bits as
    spmm_csr -> bias_add -> relu run separately.  `static_csr` as for
    spmm_csr: the plan of an unchanged CSR is kept in the op's kernel state."""
    rp, ci = _csr_pair(a_csr_row_ptr, a_csr_col_idx)
    vals = _prep(a_csr_values, "a_csr_values")
    bb = _prep(b, "b", matrix=True)
    bs = _prep(bias, "bias") if bias is not None else None
    m, k = int(a_num_rows), int(a_num_cols)
    r_rp, r_ci, r_v, r_b = _refs(rp, ci, vals, bb)
    r_bias = _refs(bs)[0] if bs is not None else None
    od = TensorDesc()
    check(LIB.ofx_functional_spmm_csr_infer(r_rp, r_ci, r_v, m, k, r_b, ctypes.byref(od)),
          "fused_spmm_csr")
    if out is None:
        out = torch.empty((od.shape[0], od.shape[1]), dtype=_DT_TO_TORCH[od.dtype], device=bb.device)
    _two_phase(LIB.ofx_functional_fused_spmm_csr_attrs, bb,
               (r_rp, r_ci, r_v, r_b, r_bias, m, k, 1 if relu else 0), _refs(out),
               attrs=(_attrs_arg(static_csr),), what="fused_spmm_csr",
               query_fn=LIB.ofx_functional_fused_spmm_csr, host_tmp=False)
    return out


def sddmm_csr(a_csr_row_ptr: torch.Tensor, a_csr_col_idx: torch.Tensor, a: torch.Tensor,
              b: torch.Tensor, a_num_rows: int, a_num_cols: int, *,
              static_csr: int = 0) -> torch.Tensor:
    """out[j] = <a[row(j), :], b[col(j), :]> (op "sddmm_csr": the values-gradient of spmm_csr).
    `static_csr` as for spmm_csr: the SDDMM's plan of an unchanged CSR is kept."""
    rp, ci = _csr_pair(a_csr_row_ptr, a_csr_col_idx)
    a, b = _prep(a, "a", matrix=True), _prep(b, "b", matrix=True)
    if b.dim() == 2 and b.shape[1] == 0:  # empty inner dimension: every dot product is 0
        out = torch.zeros(ci.numel(), dtype=b.dtype, device=b.device)
    else:
        out = torch.empty(ci.numel(), dtype=b.dtype, device=b.device)
    if b.dim() == 2 and b.shape[1] == 0 and a.dim() == 2 and a.shape[1] == 0:
        return out
    _two_phase(LIB.ofx_functional_sddmm_csr_attrs, b,
               _refs(rp, ci, a, b) + (int(a_num_rows), int(a_num_cols)), _refs(out),
               attrs=(_attrs_arg(static_csr),))
    return out


def spmm_csr_gathered(a_csr_row_ptr: torch.Tensor, a_csr_col_idx: torch.Tensor,
                      a_csr_values: torch.Tensor, values_perm: torch.Tensor, a_num_rows: int,
                      a_num_cols: int, b: torch.Tensor, *, out: torch.Tensor | None = None,
                      static_csr: int = 0):
    """Op "spmm_csr_gathered": A @ b with nonzero j's value a_csr_values[values_perm[j]] (the
    d(b) gradient of spmm_csr with learnable values: A^T's structure, A's values, A^T's perm).
    `static_csr` as for spmm_csr (the autograd's cached A^T passes its entry's value)."""
    rp, ci = _csr_pair(a_csr_row_ptr, a_csr_col_idx)
    vals, perm = _prep(a_csr_values, "a_csr_values"), _prep(values_perm, "values_perm")
    bb = _prep(b, "b", matrix=True)
    if out is None:
        out = torch.empty((int(a_num_rows), bb.shape[1] if bb.dim() == 2 else 0), dtype=bb.dtype,
                          device=bb.device)
    if out.numel() == 0:
        return out
    _two_phase(LIB.ofx_functional_spmm_csr_gathered_attrs, bb,
               _refs(rp, ci, vals, perm, bb) + (int(a_num_rows), int(a_num_cols)), _refs(out),
               attrs=(_attrs_arg(static_csr),))
    return out


REDUCE_CODES = {"sum": _lib.REDUCE_SUM, "mean": _lib.REDUCE_MEAN, "max": _lib.REDUCE_MAX,
                "min": _lib.REDUCE_MIN}


def reduce_code(reduce: str) -> int:
    try:
        return REDUCE_CODES[reduce]
    except (KeyError, TypeError):
        raise ValueError(f"spmm: reduce must be one of {sorted(REDUCE_CODES)}, got {reduce!r}") \
            from None


def spmm_csr_reduce(a_csr_row_ptr: torch.Tensor, a_csr_col_idx: torch.Tensor,
                    a_csr_values: torch.Tensor, a_num_rows: int, a_num_cols: int, b: torch.Tensor,
                    reduce: str = "sum", *, out: torch.Tensor | None = None, _parallel=None,
                    num_threads: int = 0):
    """Op "spmm_csr_reduce": (out, arg) with out[r, :] = reduce_j values[j] * b[col_idx[j], :],
    reduce in {"sum", "mean", "max", "min"} (contract in include/ofx_spmm.h).  arg[r, c] is the
    winning GLOBAL nonzero index of max / min in the index dtype (-1 for an empty row, whose out
    is +0); for sum / mean it is an empty [0, N] tensor.  `_parallel=(parallel_id, parallel_num,
    out_split_axis[, logical_n])` as for spmm_csr: this rank's rows (axis 0) or columns (axis 1)
    of out and arg; arg keeps global nonzero indices under a row split."""
    code = reduce_code(reduce)
    rp, ci = _csr_pair(a_csr_row_ptr, a_csr_col_idx)
    vals = _prep(a_csr_values, "a_csr_values")
    bb = _prep(b, "b", matrix=True)
    pid, pnum, axis, logical_n = 0, 1, -1, -1
    if _parallel is not None:
        pid, pnum, axis = (int(x) for x in _parallel[:3])
        logical_n = int(_parallel[3]) if len(_parallel) > 3 else -1
    rows = int(a_num_rows)
    if axis == 0 and pnum > 1 and rows > 0:
        lo, hi = balanced_range(rows, pnum, pid)
        rows = hi - lo
    n = bb.shape[1] if bb.dim() == 2 else 0
    if out is None:
        out = torch.empty((rows, n), dtype=bb.dtype, device=bb.device)
    has_arg = code in (_lib.REDUCE_MAX, _lib.REDUCE_MIN)
    arg = torch.empty((rows if has_arg else 0, n), dtype=rp.dtype, device=bb.device)
    head = (*_refs(rp, ci, vals), int(a_num_rows), int(a_num_cols), *_refs(bb), code)
    _two_phase(LIB.ofx_functional_spmm_csr_reduce, bb, head, _refs(out, arg),
               (pid, pnum, axis, logical_n, int(num_threads)), what="spmm_csr_reduce")
    return out, arg


def spmm_csr_reduce_grad_b(at_row_ptr: torch.Tensor, at_col_idx: torch.Tensor,
                           at_perm: torch.Tensor, a_csr_values: torch.Tensor, arg: torch.Tensor,
                           dy: torch.Tensor, a_num_rows: int, a_num_cols: int) -> torch.Tensor:
    """Op "spmm_csr_reduce_grad_b": d(b) [K, N] of reduce = max / min from A^T's structure
    (csr_transpose), A's values, the forward's arg and the upstream gradient dy; deterministic,
    in the sum op's order on A^T (include/ofx_spmm.h ofx_spmm_csr_select)."""
    rp, ci, perm = (_prep(t, n) for t, n in ((at_row_ptr, "at_row_ptr"), (at_col_idx, "at_col_idx"),
                                             (at_perm, "at_perm")))
    vals = _prep(a_csr_values, "a_csr_values")
    arg, dy = _prep(arg, "arg", matrix=True), _prep(dy, "dy", matrix=True)
    out = torch.empty((int(a_num_cols), dy.shape[1]), dtype=dy.dtype, device=dy.device)
    _two_phase(LIB.ofx_functional_spmm_csr_reduce_grad_b, dy,
               _refs(rp, ci, perm, vals, arg, dy) + (int(a_num_rows), int(a_num_cols)), _refs(out))
    return out


def spmm_csr_reduce_grad_values(a_csr_row_ptr: torch.Tensor, a_csr_col_idx: torch.Tensor,
                                arg: torch.Tensor, dy: torch.Tensor, b: torch.Tensor,
                                a_num_rows: int, a_num_cols: int) -> torch.Tensor:
    """Op "spmm_csr_reduce_grad_values": d(values) [nnz] of reduce = max / min, the SDDMM of dy
    and b restricted to the columns each nonzero won (ofx_sddmm_csr_select)."""
    rp, ci = _csr_pair(a_csr_row_ptr, a_csr_col_idx)
    arg, dy = _prep(arg, "arg", matrix=True), _prep(dy, "dy", matrix=True)
    bb = _prep(b, "b", matrix=True)
    if bb.dim() == 2 and bb.shape[1] == 0:  # empty inner dimension: every dot product is +0
        return torch.zeros(ci.numel(), dtype=bb.dtype, device=bb.device)
    out = torch.empty(ci.numel(), dtype=bb.dtype, device=bb.device)
    _two_phase(LIB.ofx_functional_spmm_csr_reduce_grad_values, bb,
               _refs(rp, ci, arg, dy, bb) + (int(a_num_rows), int(a_num_cols)), _refs(out))
    return out


def _check_inputs(op, rp, ci, named, rank, ref, per_nonzero, gat=False):
    """The shape and dtype checks the edge-softmax, multi-head and GAT ops share, ahead of the op
    layer's own (its messages name the C-ABI).  `named`: [(name, tensor)], each of `rank`
    dimensions; `ref`: the name of the one whose dtype the others must have; per_nonzero: True
    (every tensor), False (none) or the names of those that have nnz elements (rank 1) or nnz
    rows (rank 2) of `ref`'s number of heads.  gat: the GAT ops' form, every tensor [rows, heads]
    with `ref`'s heads on `ref`'s device, `ref` with a_num_rows rows."""
    ref_t = dict(named)[ref]
    for name, t in named:
        nnz_rows = per_nonzero if isinstance(per_nonzero, bool) else name in per_nonzero
        layout = " [rows, heads]" if gat else " [nnz, heads]" if nnz_rows and rank == 2 else ""
        if name == ref and not per_nonzero and not gat:
            layout = " [K, heads * D]"
        if t.dim() != rank:
            raise RuntimeError(f"{op}: {name} should be {rank}-D{layout}, got shape "
                               f"{tuple(t.shape)}")
        if nnz_rows and t.shape[0] != ci.numel():
            raise RuntimeError(f"{op}: {name} should have nnz = {ci.numel()} "
                               f"{'elements' if rank == 1 else 'rows'} (as a_csr_col_idx), got "
                               f"{t.shape[0]}")
        if (nnz_rows or gat) and rank == 2 and t.shape[1] != ref_t.shape[1]:
            raise RuntimeError(f"{op}: {name} should have the number of heads of {ref} "
                               f"({t.shape[1]} vs {ref_t.shape[1]})")
        if gat and t.device != ref_t.device:
            raise RuntimeError(f"{op}: expected all tensors on the same device, got {name} on "
                               f"{t.device} and {ref} on {ref_t.device}")
    if gat and ref_t.shape[0] != rp.numel() - 1:
        raise RuntimeError(f"{op}: {ref} should have a_num_rows = {rp.numel() - 1} rows, got "
                           f"{ref_t.shape[0]}")
    if rp.dtype != ci.dtype:
        raise TypeError(f"{op}: a_csr_col_idx should have the dtype of a_csr_row_ptr "
                        f"({ci.dtype} vs {rp.dtype})")
    dtype_code(rp.dtype)
    if ref_t.dtype not in (torch.float32, torch.float64, torch.float16, torch.bfloat16):
        raise TypeError(f"{op} supports float, double, float16, bfloat16; got {ref_t.dtype}")
    for name, t in named:
        if t.dtype != ref_t.dtype:
            detail = f" ({t.dtype} vs {ref_t.dtype})" if gat or not per_nonzero else ""
            raise TypeError(f"{op}: {name} datatype should be equal to {ref}{detail}")


def edge_softmax_csr(a_csr_row_ptr: torch.Tensor, a_csr_col_idx: torch.Tensor, e: torch.Tensor, *,
                     out: torch.Tensor | None = None) -> torch.Tensor:
    """Op "edge_softmax_csr": out[j] = softmax of the scores e over the nonzeros of j's row (DGL's
    edge_softmax, PyG's softmax(src, ptr=row_ptr)); contract in include/ofx_spmm.h.  One HIP
    launch on GPU tensors, the kCPU kernel on CPU tensors: the same bits."""
    rp, ci = _csr_pair(a_csr_row_ptr, a_csr_col_idx)
    e = _prep(e, "e")
    _check_inputs("edge_softmax_csr", rp, ci, [("e", e)], 1, "e", True)
    if out is None:
        out = torch.empty_like(e)
    _two_phase(LIB.ofx_functional_edge_softmax_csr, e, _refs(rp, ci, e), _refs(out))
    return out


def edge_softmax_csr_grad(a_csr_row_ptr: torch.Tensor, a_csr_col_idx: torch.Tensor,
                          y: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """Op "edge_softmax_csr_grad": dx[j] = y[j] * (dy[j] - sum over j's row of y * dy), from the
    forward's stored y."""
    rp, ci = _csr_pair(a_csr_row_ptr, a_csr_col_idx)
    y, dy = _prep(y, "y"), _prep(dy, "dy")
    _check_inputs("edge_softmax_csr_grad", rp, ci, [("y", y), ("dy", dy)], 1, "y", True)
    dx = torch.empty_like(y)
    _two_phase(LIB.ofx_functional_edge_softmax_csr_grad, y, _refs(rp, ci, y, dy), _refs(dx))
    return dx


def _check_out(op, out, shape, like, contiguous=False):
    """The op's output: a new `shape` tensor of `like`'s dtype and device, or the caller's `out`
    once it is found to be one."""
    if out is None:
        return torch.empty(tuple(shape), dtype=like.dtype, device=like.device)
    if contiguous and not out.is_contiguous():
        raise RuntimeError(f"{op}: out must be contiguous")
    if tuple(out.shape) != tuple(shape) or out.dtype != like.dtype or out.device != like.device:
        raise RuntimeError(f"{op}: out must be a {tuple(shape)} tensor of dtype {like.dtype} on "
                           f"{like.device}, got {tuple(out.shape)} {out.dtype} on {out.device}")
    return out


def spmm_csr_heads(a_csr_row_ptr: torch.Tensor, a_csr_col_idx: torch.Tensor,
                   a_csr_values: torch.Tensor, a_num_rows: int, a_num_cols: int, b: torch.Tensor,
                   *, out: torch.Tensor | None = None) -> torch.Tensor:
    """Op "spmm_csr_heads": out[M, H*D] with out[r, h*D + c] = sum over the row's nonzeros j of
    a_csr_values[j, h] * b[a_csr_col_idx[j], h*D + c]; a_csr_values is [nnz, H], b is [K, H*D] with
    head h in columns [h*D, (h+1)*D).  One launch for all heads; every head's slice has the bits
    of spmm_csr on that slice (contract in include/ofx_spmm.h)."""
    rp, ci = _csr_pair(a_csr_row_ptr, a_csr_col_idx)
    vals = _prep(a_csr_values, "a_csr_values")
    bb = _prep(b, "b", matrix=True)
    _check_inputs("spmm_csr_heads", rp, ci, [("a_csr_values", vals), ("b", bb)], 2, "b", False)
    if vals.shape[0] != ci.numel():
        raise RuntimeError(f"spmm_csr_heads: a_csr_values should have nnz = {ci.numel()} rows (as "
                           f"a_csr_col_idx), got {vals.shape[0]}")
    if vals.shape[1] < 1 or bb.shape[1] % vals.shape[1] != 0:
        raise RuntimeError(f"spmm_csr_heads: b's columns ({bb.shape[1]}) should be a multiple of "
                           f"the number of heads ({vals.shape[1]})")
    out = _check_out("spmm_csr_heads", out, (int(a_num_rows), bb.shape[1]), bb)
    if out.numel() == 0:
        return out
    _two_phase(LIB.ofx_functional_spmm_csr_heads, bb,
               _refs(rp, ci, vals, bb) + (int(a_num_rows), int(a_num_cols)), _refs(out))
    return out


FP8_FORMATS = {torch.float8_e4m3fn: _lib.FP8_E4M3, torch.float8_e5m2: _lib.FP8_E5M2}


def _codes_desc(b_q: torch.Tensor) -> TensorDesc:
    """The descriptor of an FP8 tensor as the op takes it: its codes as kUInt8 (DataType has no
    8-bit float; the format travels in attr b_format)."""
    d = TensorDesc()
    d.dtype = _lib.DT_UINT8
    d.device = _device_index(b_q)
    d.ndim = b_q.dim()
    for i in range(b_q.dim()):
        d.shape[i] = b_q.shape[i]
        d.stride[i] = b_q.stride(i)
    d.data = b_q.data_ptr() if b_q.numel() > 0 else None
    return d


def spmm_csr_heads_fp8(a_csr_row_ptr: torch.Tensor, a_csr_col_idx: torch.Tensor,
                       a_csr_values: torch.Tensor, a_num_rows: int, a_num_cols: int,
                       b: torch.Tensor, b_scale: torch.Tensor | None = None, *,
                       out: torch.Tensor | None = None) -> torch.Tensor:
    """Op "spmm_csr_heads_fp8": spmm_csr_heads over a feature table stored in FP8.  b is [K, H*D] of
    dtype torch.float8_e4m3fn or torch.float8_e5m2 (a row-strided view is read in place), b_scale
    an optional float32 [K] scale per row of b, a_csr_values [nnz, H] of dtype float32, float16 or
    bfloat16, which is out's.  out has exactly the bits of spmm_csr_heads on the values times
    b_scale[col] rounded to the dtype and on b converted to the dtype (contract in
    include/ofx_spmm.h)."""
    op = "spmm_csr_heads_fp8"
    rp, ci = _csr_pair(a_csr_row_ptr, a_csr_col_idx)
    vals = _prep(a_csr_values, "a_csr_values")
    if not isinstance(b, torch.Tensor) or b.dtype not in FP8_FORMATS:
        raise TypeError(f"{op}: b should be float8_e4m3fn or float8_e5m2, got "
                        f"{getattr(b, 'dtype', type(b).__name__)}")
    bb = _prep(b, "b", matrix=True)
    _check_inputs(op, rp, ci, [("a_csr_values", vals)], 2, "a_csr_values", True)
    if vals.dtype == torch.float64:
        raise TypeError(f"{op} supports float, float16, bfloat16; got {vals.dtype}")
    if bb.dim() != 2:
        raise RuntimeError(f"{op}: b should be 2-D [K, heads * D], got shape {tuple(bb.shape)}")
    if vals.shape[1] < 1 or bb.shape[1] % vals.shape[1] != 0:
        raise RuntimeError(f"{op}: b's columns ({bb.shape[1]}) should be a multiple of the number "
                           f"of heads ({vals.shape[1]})")
    if bb.device != vals.device:
        raise RuntimeError(f"{op}: expected all tensors on the same device, got b on {bb.device} "
                           f"and a_csr_values on {vals.device}")
    r_scale = None
    if b_scale is not None:
        b_scale = _prep(b_scale, "b_scale")
        if b_scale.dtype != torch.float32 or tuple(b_scale.shape) != (bb.shape[0],):
            raise RuntimeError(f"{op}: b_scale should be float32 [K] = ({bb.shape[0]},), got "
                               f"{b_scale.dtype} {tuple(b_scale.shape)}")
        if b_scale.device != vals.device:
            raise RuntimeError(f"{op}: expected all tensors on the same device, got b_scale on "
                               f"{b_scale.device}")
        r_scale = ctypes.byref(desc(b_scale))
    out = _check_out(op, out, (int(a_num_rows), bb.shape[1]), vals)
    if out.numel() == 0:
        return out
    _two_phase(LIB.ofx_functional_spmm_csr_heads_fp8, vals,
               _refs(rp, ci, vals) + (ctypes.byref(_codes_desc(bb)), r_scale, int(a_num_rows),
                                      int(a_num_cols), FP8_FORMATS[bb.dtype]), _refs(out))
    return out


def sddmm_csr_heads(a_csr_row_ptr: torch.Tensor, a_csr_col_idx: torch.Tensor, a: torch.Tensor,
                    b: torch.Tensor, num_heads: int, *,
                    out: torch.Tensor | None = None) -> torch.Tensor:
    """Op "sddmm_csr_heads": out[nnz, H] with out[j, h] = <a[row(j), h*D:(h+1)*D],
    b[col(j), h*D:(h+1)*D]> for a [M, H*D], b [K, H*D], H = num_heads: the scores of multi-head
    graph attention and the values-gradient of spmm_csr_heads; every head has the bits of
    sddmm_csr on its slice."""
    rp, ci = _csr_pair(a_csr_row_ptr, a_csr_col_idx)
    a, bb = _prep(a, "a", matrix=True), _prep(b, "b", matrix=True)
    _check_inputs("sddmm_csr_heads", rp, ci, [("a", a), ("b", bb)], 2, "b", False)
    heads = int(num_heads)
    if heads < 1 or bb.shape[1] % heads != 0:
        raise RuntimeError(f"sddmm_csr_heads: b's columns ({bb.shape[1]}) should be a multiple of "
                           f"num_heads ({heads})")
    if a.shape[1] != bb.shape[1]:
        raise RuntimeError("sddmm_csr_heads: a and b should have the same number of columns "
                           f"({a.shape[1]} vs {bb.shape[1]})")
    out = _check_out("sddmm_csr_heads", out, (ci.numel(), heads), bb, contiguous=True)
    if out.numel() == 0:
        return out
    if bb.shape[1] == 0:  # empty inner dimension: every dot product is +0
        return out.zero_()
    _two_phase(LIB.ofx_functional_sddmm_csr_heads, bb, _refs(rp, ci, a, bb) + (heads,), _refs(out))
    return out


def graph_attention_csr_heads(a_csr_row_ptr: torch.Tensor, a_csr_col_idx: torch.Tensor,
                              q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, num_heads: int, *,
                              out: torch.Tensor | None = None,
                              attn_out: torch.Tensor | None = None):
    """Op "graph_attention_csr_heads": dot-product graph attention through one fused kernel for
    the rows below the SpMM's hub threshold, with the hub rows in follow-up launches.  For
    q [M, H*D], k and v [K, H*D] with H = num_heads, returns (out [M, H*D], attn [nnz, H]) with
    attn = edge_softmax_csr_heads(sddmm_csr_heads(q, k)) and out = spmm_csr_heads(attn, v), both
    with exactly the bits of that composition (contract in include/ofx_spmm.h).  `out`: a [M, H*D]
    tensor; `attn_out`: a contiguous [nnz, H] tensor; both written directly."""
    op = "graph_attention_csr_heads"
    rp, ci = _csr_pair(a_csr_row_ptr, a_csr_col_idx)
    q = _prep(q, "q", matrix=True)
    kk, vv = _prep(k, "k", matrix=True), _prep(v, "v", matrix=True)
    _check_inputs(op, rp, ci, [("q", q), ("v", vv), ("k", kk)], 2, "k", False)
    heads = int(num_heads)
    if heads < 1 or kk.shape[1] % heads != 0:
        raise RuntimeError(f"{op}: k's columns ({kk.shape[1]}) should be a multiple of "
                           f"num_heads ({heads})")
    if q.shape[1] != kk.shape[1] or vv.shape[1] != kk.shape[1]:
        raise RuntimeError(f"{op}: q, k and v should have the same number of columns "
                           f"({q.shape[1]}, {kk.shape[1]}, {vv.shape[1]})")
    if vv.shape[0] != kk.shape[0]:
        raise RuntimeError(f"{op}: k and v should have the same number of rows "
                           f"({kk.shape[0]} vs {vv.shape[0]})")
    m = rp.numel() - 1
    if q.shape[0] != m:
        raise RuntimeError(f"{op}: q should have a_num_rows = {m} rows, got {q.shape[0]}")
    out = _check_out(op, out, (m, kk.shape[1]), kk)
    attn_out = _check_out(op, attn_out, (ci.numel(), heads), kk, contiguous=True)
    if out.numel() == 0:
        return out, attn_out
    _two_phase(LIB.ofx_functional_graph_attention_csr_heads, kk,
               _refs(rp, ci, q, kk, vv) + (heads,), _refs(out, attn_out))
    return out, attn_out


def edge_softmax_csr_heads(a_csr_row_ptr: torch.Tensor, a_csr_col_idx: torch.Tensor,
                           e: torch.Tensor, *, out: torch.Tensor | None = None) -> torch.Tensor:
    """Op "edge_softmax_csr_heads": out[j, h] = softmax of the scores e[:, h] over the nonzeros of
    j's row, for e [nnz, H] (sddmm_csr_heads's output; a non-contiguous e is copied first).  One
    launch for all heads; every head has the bits of edge_softmax_csr on its column (contract in
    include/ofx_spmm.h).  `out`: a contiguous [nnz, H] tensor, written directly."""
    rp, ci = _csr_pair(a_csr_row_ptr, a_csr_col_idx)
    e = _prep(e, "e")
    _check_inputs("edge_softmax_csr_heads", rp, ci, [("e", e)], 2, "e", True)
    out = _check_out("edge_softmax_csr_heads", out, e.shape, e, contiguous=True)
    if out.numel() == 0:
        return out
    _two_phase(LIB.ofx_functional_edge_softmax_csr_heads, e, _refs(rp, ci, e), _refs(out))
    return out


def edge_softmax_csr_heads_grad(a_csr_row_ptr: torch.Tensor, a_csr_col_idx: torch.Tensor,
                                y: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """Op "edge_softmax_csr_heads_grad": dx[j, h] = y[j, h] * (dy[j, h] - sum over j's row of
    y[:, h] * dy[:, h]) for y, dy [nnz, H], from the forward's stored y; one launch."""
    rp, ci = _csr_pair(a_csr_row_ptr, a_csr_col_idx)
    y, dy = _prep(y, "y"), _prep(dy, "dy")
    _check_inputs("edge_softmax_csr_heads_grad", rp, ci, [("y", y), ("dy", dy)], 2, "y", True)
    dx = torch.empty_like(y)
    if dx.numel() == 0:
        return dx
    _two_phase(LIB.ofx_functional_edge_softmax_csr_heads_grad, y, _refs(rp, ci, y, dy), _refs(dx))
    return dx


def gat_softmax_csr_heads(a_csr_row_ptr: torch.Tensor, a_csr_col_idx: torch.Tensor,
                          s_row: torch.Tensor, s_col: torch.Tensor, negative_slope: float = 0.2, *,
                          out: torch.Tensor | None = None) -> torch.Tensor:
    """Op "gat_softmax_csr_heads": out[j, h] = softmax over j's row of
    LeakyReLU(s_row[row(j), h] + s_col[a_csr_col_idx[j], h]) for s_row [M, H] and s_col [K, H], in
    one launch: exactly the bits of edge_softmax_csr_heads on the scores rounded to the dtype
    (contract in include/ofx_spmm.h).  Non-contiguous inputs are copied first.  `out`: a contiguous
    [nnz, H] tensor, written directly.  negative_slope must be finite and > 0."""
    op = "gat_softmax_csr_heads"
    rp, ci = _csr_pair(a_csr_row_ptr, a_csr_col_idx)
    s_row, s_col = _prep(s_row, "s_row"), _prep(s_col, "s_col")
    _check_inputs(op, rp, ci, [("s_row", s_row), ("s_col", s_col)], 2, "s_row", (), gat=True)
    out = _check_out(op, out, (ci.numel(), s_row.shape[1]), s_row, contiguous=True)
    if out.numel() == 0:
        return out
    _two_phase(LIB.ofx_functional_gat_softmax_csr_heads, s_row,
               _refs(rp, ci, s_row, s_col) + (float(negative_slope),), _refs(out))
    return out


def gat_softmax_csr_heads_grad(a_csr_row_ptr: torch.Tensor, a_csr_col_idx: torch.Tensor,
                               s_row: torch.Tensor, s_col: torch.Tensor, y: torch.Tensor,
                               dy: torch.Tensor, negative_slope: float = 0.2):
    """Op "gat_softmax_csr_heads_grad": (ds [nnz, H], d_row [M, H]) from the forward's stored y and
    the upstream dy, one launch: ds = edge_softmax_csr_heads_grad(y, dy) times LeakyReLU's
    derivative at the recomputed sum, d_row[r] = the sum of ds over r's nonzeros in the softmax's
    order (+0 for an empty row)."""
    op = "gat_softmax_csr_heads_grad"
    rp, ci = _csr_pair(a_csr_row_ptr, a_csr_col_idx)
    s_row, s_col = _prep(s_row, "s_row"), _prep(s_col, "s_col")
    y, dy = _prep(y, "y"), _prep(dy, "dy")
    _check_inputs(op, rp, ci, [("s_row", s_row), ("s_col", s_col), ("y", y), ("dy", dy)], 2,
                  "s_row", ("y", "dy"), gat=True)
    ds = torch.empty_like(y)
    if ds.numel() == 0:  # nothing is written for nnz == 0 or H == 0: every row is empty
        return ds, torch.zeros_like(s_row)
    d_row = torch.empty_like(s_row)
    _two_phase(LIB.ofx_functional_gat_softmax_csr_heads_grad, s_row,
               _refs(rp, ci, s_row, s_col, y, dy) + (float(negative_slope),), _refs(ds, d_row))
    return ds, d_row


def _gatv2_inputs(op, rp, ci, x_row, x_col, att, num_heads):
    """The prepared inputs of the GATv2 ops after the shape checks they share: x_row [M, H*D],
    x_col [K, H*D] (row-strided views in place), att [H*D]."""
    x_row, x_col = _prep(x_row, "x_row", matrix=True), _prep(x_col, "x_col", matrix=True)
    att = _prep(att, "att")
    _check_inputs(op, rp, ci, [("x_row", x_row), ("x_col", x_col)], 2, "x_col", False)
    heads = int(num_heads)
    if att.dim() != 1:
        raise RuntimeError(f"{op}: att should be 1-D [heads * D], got shape {tuple(att.shape)}")
    if att.dtype != x_col.dtype:
        raise TypeError(f"{op}: att datatype should be equal to x_col ({att.dtype} vs "
                        f"{x_col.dtype})")
    if x_row.device != x_col.device or att.device != x_col.device:
        raise RuntimeError(f"{op}: expected all tensors on the same device, got x_row on "
                           f"{x_row.device}, x_col on {x_col.device} and att on {att.device}")
    if heads < 1 or x_col.shape[1] % heads != 0:
        raise RuntimeError(f"{op}: x_col's columns ({x_col.shape[1]}) should be a multiple of "
                           f"num_heads ({heads})")
    if x_row.shape[1] != x_col.shape[1] or att.shape[0] != x_col.shape[1]:
        raise RuntimeError(f"{op}: x_row, x_col and att should have the same number of columns "
                           f"({x_row.shape[1]}, {x_col.shape[1]}, {att.shape[0]})")
    if x_row.shape[0] != rp.numel() - 1:
        raise RuntimeError(f"{op}: x_row should have a_num_rows = {rp.numel() - 1} rows, got "
                           f"{x_row.shape[0]}")
    return x_row, x_col, att, heads


def gatv2_scores_csr_heads(a_csr_row_ptr: torch.Tensor, a_csr_col_idx: torch.Tensor,
                           x_row: torch.Tensor, x_col: torch.Tensor, att: torch.Tensor,
                           num_heads: int, negative_slope: float = 0.2, *,
                           out: torch.Tensor | None = None) -> torch.Tensor:
    """Op "gatv2_scores_csr_heads": out[j, h] = sum over c of att[h*D + c] *
    LeakyReLU(x_row[row(j), h*D + c] + x_col[a_csr_col_idx[j], h*D + c]) for x_row [M, H*D],
    x_col [K, H*D], att [H*D], H = num_heads, in one launch: exactly the bits of sddmm_csr_heads
    on the activated sum rounded to the dtype, which is never written (contract in
    include/ofx_spmm.h).  `out`: a contiguous [nnz, H] tensor, written directly.  negative_slope
    must be finite and > 0."""
    op = "gatv2_scores_csr_heads"
    rp, ci = _csr_pair(a_csr_row_ptr, a_csr_col_idx)
    x_row, x_col, att, heads = _gatv2_inputs(op, rp, ci, x_row, x_col, att, num_heads)
    out = _check_out(op, out, (ci.numel(), heads), x_col, contiguous=True)
    if out.numel() == 0:
        return out
    if x_col.shape[1] == 0:  # empty inner dimension: every dot product is +0
        return out.zero_()
    _two_phase(LIB.ofx_functional_gatv2_scores_csr_heads, x_row,
               _refs(rp, ci, x_row, x_col, att) + (heads, float(negative_slope)), _refs(out))
    return out


def gatv2_scores_csr_heads_grad(a_csr_row_ptr: torch.Tensor, a_csr_col_idx: torch.Tensor,
                                x_row: torch.Tensor, x_col: torch.Tensor, att: torch.Tensor,
                                dy: torch.Tensor, num_heads: int, negative_slope: float = 0.2,
                                with_att: bool = True):
    """Op "gatv2_scores_csr_heads_grad": (d_x [M, H*D], p) from the upstream dy [nnz, H], one
    launch: d_x is the gradient in x_row; p [M, H*D] (with_att; None otherwise) holds the per-row
    terms whose column sum is the gradient in att.  Both are sums over the row's nonzeros in
    spmm_csr_heads's order (+0 for an empty row)."""
    op = "gatv2_scores_csr_heads_grad"
    rp, ci = _csr_pair(a_csr_row_ptr, a_csr_col_idx)
    x_row, x_col, att, heads = _gatv2_inputs(op, rp, ci, x_row, x_col, att, num_heads)
    dy = _prep(dy, "dy")
    if dy.dim() != 2 or tuple(dy.shape) != (ci.numel(), heads):
        raise RuntimeError(f"{op}: dy should be [nnz, heads] = ({ci.numel()}, {heads}), got shape "
                           f"{tuple(dy.shape)}")
    if dy.dtype != x_col.dtype or dy.device != x_col.device:
        raise TypeError(f"{op}: dy datatype and device should be equal to x_col's ({dy.dtype} on "
                        f"{dy.device} vs {x_col.dtype} on {x_col.device})")
    m, n = x_row.shape
    d_x = torch.empty((m, n), dtype=x_col.dtype, device=x_col.device)
    p = torch.empty((m if with_att else 0, n), dtype=x_col.dtype, device=x_col.device)
    if d_x.numel():
        _two_phase(LIB.ofx_functional_gatv2_scores_csr_heads_grad, x_row,
                   _refs(rp, ci, x_row, x_col, att, dy) +
                   (heads, float(negative_slope), 1 if with_att else 0), _refs(d_x, p))
    return d_x, (p if with_att else None)


def row_scale_by_degree(a_csr_row_ptr: torch.Tensor, x: torch.Tensor, *,
                        out: torch.Tensor | None = None) -> torch.Tensor:
    """out[r, :] = x[r, :] / deg_r in x's accumulation type, rounded once (deg_r = 0: +0): the
    mean's divide, forward (on the sum) and backward (on the upstream gradient)."""
    rp = _prep(a_csr_row_ptr, "a_csr_row_ptr")
    x = _prep(x, "x", matrix=True)
    if out is None:
        out = torch.empty(tuple(x.shape), dtype=x.dtype, device=x.device)
    m, n = x.shape
    common = (dtype_code(rp.dtype), dtype_code(x.dtype), m, n, rp.data_ptr(),
              x.data_ptr() if x.numel() else None, x.stride(0) if m else n,
              out.data_ptr() if out.numel() else None, out.stride(0) if m else n, 0, m)
    if x.device.type == "cpu":
        check(LIB.ofx_row_scale_by_degree_cpu(0, *common), "row_scale_by_degree")
    else:
        check(LIB.ofx_row_scale_by_degree(current_stream_handle(x), *common),
              "row_scale_by_degree")
    return out


def csr_transpose(a_csr_row_ptr: torch.Tensor, a_csr_col_idx: torch.Tensor, a_num_rows: int,
                  a_num_cols: int):
    """Structure of A^T (op "csr_transpose"): (row_ptr [K+1], col_idx [nnz], perm [nnz])."""
    rp, ci = _csr_pair(a_csr_row_ptr, a_csr_col_idx)
    it, dev = rp.dtype, rp.device
    rp_t = torch.empty(int(a_num_cols) + 1, dtype=it, device=dev)
    ci_t = torch.empty(ci.numel(), dtype=it, device=dev)
    perm = torch.empty(ci.numel(), dtype=it, device=dev)
    _two_phase(LIB.ofx_functional_csr_transpose, rp,
               _refs(rp, ci) + (int(a_num_rows), int(a_num_cols)), _refs(rp_t, ci_t, perm))
    return rp_t, ci_t, perm


def balanced_range(total: int, parts: int, idx: int) -> tuple[int, int]:
    lo, hi = ctypes.c_int64(), ctypes.c_int64()
    check(LIB.ofx_balanced_range(total, parts, idx, ctypes.byref(lo), ctypes.byref(hi)),
          "balanced_range")
    return lo.value, hi.value


def sbp_signatures(op: str = "spmm_csr", optional_inputs: str = "") -> str:
    buf = ctypes.create_string_buffer(4096)
    check(LIB.ofx_op_sbp_signatures(op.encode(), optional_inputs.encode(), buf, len(buf)), "sbp")
    return buf.value.decode()

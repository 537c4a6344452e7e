"""Helpers of the max / min / mean aggregation tests (test_reduce_cpu.py, test_reduce_gpu.py):
numpy references written from the contract in include/ofx_spmm.h, and callers of the C-ABI
entries on host or device memory with explicit leading dimensions, row ranges and options."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from helpers import dtype_name, from_f32, to_oracle
from oracle import oracle
from oneflow_spmm._C import REDUCE_CODES, current_stream_handle, dtype_code
from oneflow_spmm._lib import LIB, Options, check

PAD = 5  # extra elements of a padded leading dimension


# ---- numpy views ----------------------------------------------------------------------------------
def acc(t: torch.Tensor) -> np.ndarray:
    """A value tensor in its accumulation type (f64 for f64, else f32)."""
    a = to_oracle(t)
    if t.dtype == torch.bfloat16:
        return oracle.bf16_bits_to_f32(a)
    return a.astype(np.float64 if t.dtype == torch.float64 else np.float32)


def store(x: np.ndarray, dtype: torch.dtype) -> np.ndarray:
    """Accumulation-type values rounded to the storage type, in the oracle's representation
    (bf16 as uint16 bits); a NaN becomes the canonical quiet NaN."""
    x = np.array(x, copy=True)
    x[np.isnan(x)] = np.nan
    if dtype == torch.bfloat16:
        return oracle.f32_to_bf16_bits(x.astype(np.float32))
    if dtype == torch.float16:
        return x.astype(np.float16)
    return x.astype(np.float64 if dtype == torch.float64 else np.float32)


def products(vals: torch.Tensor, b: torch.Tensor, ci: np.ndarray, k: int) -> np.ndarray:
    """p[j, :] = mul(val[j], b[col[j], :]) rounded to the storage type, in the accumulation type;
    a column outside [0, k) reads a zero row."""
    v, bb = acc(vals), acc(b)
    rows = np.zeros((len(ci), bb.shape[1]), dtype=bb.dtype)
    ok = (ci >= 0) & (ci < k)
    rows[ok] = bb[ci[ok]]
    with np.errstate(invalid="ignore", over="ignore"):
        p = v[:, None] * rows
    if b.dtype in (torch.bfloat16, torch.float16):
        p = oracle.round16(p, dtype_name(b.dtype)).reshape(p.shape)
    return p


def ref_extremum(rp, ci, vals, b, k, reduce, row_begin=0, row_end=None):
    """(out in the oracle's representation, arg int64) by the contract: ascending j, a candidate
    wins only if strictly better or if it is NaN and the best is not; empty row: +0 and -1."""
    rp = np.asarray(to_oracle(rp), dtype=np.int64)
    ci = np.asarray(to_oracle(ci), dtype=np.int64)
    row_end = len(rp) - 1 if row_end is None else row_end
    p = products(vals, b, ci, k)
    n = p.shape[1]
    best = np.zeros((row_end - row_begin, n), dtype=p.dtype)
    arg = np.full((row_end - row_begin, n), -1, dtype=np.int64)
    lens = np.diff(rp)[row_begin:row_end]
    for t in range(int(lens.max(initial=0))):  # the t-th nonzero of every row that has one
        rows = np.flatnonzero(lens > t)
        j = rp[row_begin + rows] + t
        c, bst, ba = p[j], best[rows], arg[rows]
        with np.errstate(invalid="ignore"):
            take = (ba < 0) | ((c > bst) if reduce == "max" else (c < bst)) | \
                (np.isnan(c) & ~np.isnan(bst))
        best[rows] = np.where(take, c, bst)
        arg[rows] = np.where(take, j[:, None], ba)
    return store(best, b.dtype), arg


def ref_mean(rp, ci, vals, b, split=0, chunk=0, row_begin=0, row_end=None):
    """oracle.spmm, then the division by the row degree in the accumulation type, rounded."""
    rp_np = np.asarray(to_oracle(rp), dtype=np.int64)
    row_end = len(rp_np) - 1 if row_end is None else row_end
    s = oracle.spmm(rp_np, to_oracle(ci), to_oracle(vals), to_oracle(b),
                    dtype=dtype_name(b.dtype), split=split, chunk=chunk, row_begin=row_begin,
                    row_end=row_end)
    if b.dtype == torch.bfloat16:
        s = oracle.bf16_bits_to_f32(s)
    s = s.astype(np.float64 if b.dtype == torch.float64 else np.float32)
    deg = np.diff(rp_np)[row_begin:row_end].astype(s.dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (s / deg[:, None]).astype(s.dtype)
    out[deg == 0] = 0
    return store(out, b.dtype)


def ref_grad_b(rp, ci, vals, arg, g, k, n_sched=None, split=0, chunk=0):
    """d(b) of max / min for finite inputs: column c is oracle.spmm on A^T at width 1 with values
    val[perm] * (arg[rows_T, c] == perm) and the dense g[:, c], under the schedule of the full
    width (a zero product adds +-0 to an accumulator that started at +0: the same as skipping)."""
    rp_np = np.asarray(to_oracle(rp), dtype=np.int64)
    ci_np = np.asarray(to_oracle(ci), dtype=np.int64)
    rp_t, rows_t, perm = oracle.transpose(rp_np, ci_np, k)
    # entries of columns outside [0, k) sort past row_ptr_T[k]: in no row of A^T
    live = int(rp_t[-1])
    rows_t, perm = rows_t[:live], perm[:live]
    arg_np = np.asarray(to_oracle(arg), dtype=np.int64)
    v = acc(vals)[perm]
    n = g.shape[1]
    n_sched = n if n_sched is None else n_sched
    s = split if split > 0 else oracle.default_split(n_sched)
    c_ = chunk if chunk > 0 else s
    name = dtype_name(g.dtype)
    cols = []
    for c in range(n):
        mask = (arg_np[rows_t, c] == perm).astype(v.dtype)
        vc = to_oracle(from_f32(v * mask, g.dtype)) if g.dtype != torch.float64 else v * mask
        gc = to_oracle(g[:, c:c + 1].contiguous())
        cols.append(oracle.spmm(rp_t, rows_t, vc, gc, dtype=name, split=s, chunk=c_))
    if not cols:
        return store(np.zeros((k, 0)), g.dtype)
    return np.concatenate(cols, axis=1)


def ref_grad_values(rp, ci, arg, g, b):
    """d(values) of max / min for finite inputs: oracle.sddmm on the expanded problem with one
    row per nonzero, a'[j, :] = where(arg[row(j), :] == j, g[row(j), :], 0)."""
    rp_np = np.asarray(to_oracle(rp), dtype=np.int64)
    ci_np = np.asarray(to_oracle(ci), dtype=np.int64)
    nnz = len(ci_np)
    rows = np.repeat(np.arange(len(rp_np) - 1), np.diff(rp_np))
    arg_np = np.asarray(to_oracle(arg), dtype=np.int64)
    g_np = to_oracle(g)
    a2 = np.where(arg_np[rows] == np.arange(nnz)[:, None], g_np[rows], np.zeros_like(g_np[rows]))
    return oracle.sddmm(np.arange(nnz + 1, dtype=np.int64), ci_np, a2, to_oracle(b),
                        dtype=dtype_name(b.dtype))


# ---- C-ABI callers --------------------------------------------------------------------------------
def options(split=0, chunk=0, ordered=False):
    o = Options()
    o.split_threshold, o.chunk, o.ordered = split, chunk, 1 if ordered else 0
    return o


def padded(t: torch.Tensor, pad: int) -> torch.Tensor:
    """A copy of the 2-D tensor t as a view of a buffer with `pad` more elements per row."""
    if pad == 0:
        return t.contiguous()
    buf = torch.empty((t.shape[0], t.shape[1] + pad), dtype=t.dtype, device=t.device)
    if t.dtype.is_floating_point:
        buf.fill_(float("nan"))
    else:
        buf.fill_(-7)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _workspace(query, dev):
    size = ctypes.c_size_t(0)
    query(ctypes.byref(size))
    return torch.empty(max(size.value, 1), dtype=torch.uint8, device=dev), size.value


def run_reduce(rp, ci, vals, b, m, k, reduce, *, pad=0, row_begin=0, row_end=None, opts=None,
               want_arg=True):
    """ofx_spmm_csr_reduce(_cpu) on the tensors' device: (out, arg) for rows [row_begin, row_end),
    with leading dimensions n + pad."""
    row_end = m if row_end is None else row_end
    code = REDUCE_CODES[reduce]
    dev, n = b.device, b.shape[1]
    bb = padded(b, pad)
    rows = row_end - row_begin
    out = padded(torch.empty((rows, n), dtype=b.dtype, device=dev), pad)
    arg = padded(torch.full((rows, n), -9, dtype=rp.dtype, device=dev), pad) if want_arg else None
    it, vt, nnz = dtype_code(rp.dtype), dtype_code(b.dtype), ci.numel()
    o = ctypes.byref(opts) if opts is not None else None
    tail = (_ptr(rp), _ptr(ci), _ptr(vals), _ptr(bb), n + pad, _ptr(out), n + pad, _ptr(arg),
            n + pad, row_begin, row_end, code)
    if dev.type == "cpu":
        check(LIB.ofx_spmm_csr_reduce_cpu(0, it, vt, m, k, n, nnz, *tail, o), "reduce_cpu")
    else:
        ws, size = _workspace(lambda s: check(LIB.ofx_spmm_csr_reduce_workspace_size(
            it, vt, m, k, n, nnz, code, o, s)), dev)
        check(LIB.ofx_spmm_csr_reduce(current_stream_handle(b), it, vt, m, k, n, nnz, *tail,
                                      ws.data_ptr(), size, o), "reduce")
    return out, arg


def run_grad_b(rp_t, ci_t, perm, vals, arg, g, m, k, *, pad=0, opts=None):
    """ofx_spmm_csr_select(_cpu): d(b) [k, n] with leading dimensions n + pad."""
    dev, n = g.device, g.shape[1]
    aa, gg = padded(arg, pad), padded(g, pad)
    db = padded(torch.empty((k, n), dtype=g.dtype, device=dev), pad)
    it, vt, nnz = dtype_code(rp_t.dtype), dtype_code(g.dtype), perm.numel()
    o = ctypes.byref(opts) if opts is not None else None
    tail = (_ptr(rp_t), _ptr(ci_t), _ptr(perm), _ptr(vals), _ptr(aa), n + pad, _ptr(gg), n + pad,
            _ptr(db), n + pad, 0, k)
    if dev.type == "cpu":
        check(LIB.ofx_spmm_csr_select_cpu(0, it, vt, m, k, n, nnz, *tail, o), "select_cpu")
    else:
        ws, size = _workspace(lambda s: check(LIB.ofx_spmm_csr_select_workspace_size(
            it, vt, m, k, n, nnz, o, s)), dev)
        check(LIB.ofx_spmm_csr_select(current_stream_handle(g), it, vt, m, k, n, nnz, *tail,
                                      ws.data_ptr(), size, o), "select")
    return db


def run_grad_values(rp, ci, arg, g, b, m, k, *, pad=0):
    """ofx_sddmm_csr_select(_cpu): d(values) [nnz] with leading dimensions n + pad."""
    dev, n = b.device, b.shape[1]
    aa, gg, bb = padded(arg, pad), padded(g, pad), padded(b, pad)
    out = torch.empty(ci.numel(), dtype=b.dtype, device=dev)
    it, vt, nnz = dtype_code(rp.dtype), dtype_code(b.dtype), ci.numel()
    tail = (_ptr(rp), _ptr(ci), _ptr(aa), n + pad, _ptr(gg), n + pad, _ptr(bb), n + pad, _ptr(out),
            0, m)
    if dev.type == "cpu":
        check(LIB.ofx_sddmm_csr_select_cpu(0, it, vt, m, k, n, nnz, *tail), "sddmm_select_cpu")
    else:
        ws, size = _workspace(lambda s: check(LIB.ofx_sddmm_csr_workspace_size(
            it, vt, m, n, nnz, s)), dev)
        check(LIB.ofx_sddmm_csr_select(current_stream_handle(b), it, vt, m, k, n, nnz, *tail,
                                       ws.data_ptr(), size), "sddmm_select")
    return out


def transpose_t(rp, ci, k):
    """A^T of the CSR as tensors on rp's device, from the oracle's transpose (all nnz entries;
    those of columns outside [0, k) lie past row_ptr_T[k])."""
    rp_t, rows_t, perm = oracle.transpose(to_oracle(rp), to_oracle(ci), k)
    np_idx = np.int32 if rp.dtype == torch.int32 else np.int64
    return tuple(torch.from_numpy(np.ascontiguousarray(x.astype(np_idx))).to(rp.device)
                 for x in (rp_t, rows_t, perm))


def assert_same(a: torch.Tensor, b: torch.Tensor, what=""):
    """Identical bytes (NaNs and signed zeros included)."""
    x, y = to_oracle(a), to_oracle(b)
    assert x.shape == y.shape, (what, x.shape, y.shape)
    xb, yb = np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)
    assert np.array_equal(xb, yb), f"{what}: {int((xb != yb).sum())} bytes differ"


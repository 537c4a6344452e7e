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
    return ref_row_scale(s, np.diff(rp_np)[row_begin:row_end], b.dtype)


def ref_row_scale(s: np.ndarray, deg: np.ndarray, dtype: torch.dtype) -> np.ndarray:
    """store(s / deg) per row: s in the accumulation type, one IEEE division there, one rounding to
    the storage type; a row of degree 0 gives +0."""
    deg = np.asarray(deg).astype(s.dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (s / deg[:, None]).astype(s.dtype)
    out[deg == 0] = 0
    return store(out, dtype)


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
def options(split=0, chunk=0, ordered=False, planned=False, range_nnz=0):
    o = Options()
    o.split_threshold, o.chunk, o.ordered = split, chunk, 1 if ordered else 0
    o.planned, o.range_nnz = 1 if planned else 0, range_nnz
    return o


def _fill(buf: torch.Tensor) -> torch.Tensor:
    """NaN (with sentinel()'s payload, so that is_sentinel tells it from a kernel's NaN) or -7."""
    if not buf.dtype.is_floating_point:
        return buf.fill_(-7)
    it, bits = SENTINEL[buf.dtype]
    buf.view(it).fill_(bits)
    return buf


def padded(t: torch.Tensor, pad: int, shift: int = 0) -> torch.Tensor:
    """A copy of the 2-D tensor t as a view of a buffer with `pad` more elements per row (filled
    with NaN / -7); the view starts `shift` elements into its buffer (a base pointer that is not
    aligned to a lane's load)."""
    if pad == 0 and shift == 0:
        return t.contiguous()
    rows, n = t.shape
    flat = _fill(torch.empty(rows * (n + pad) + shift, dtype=t.dtype, device=t.device))
    view = flat[shift:].view(rows, n + pad)[:, :n]
    view.copy_(t)
    return view


def padding_of(view: torch.Tensor, pad: int) -> torch.Tensor:
    """The `pad` extra elements per row of the buffer behind padded(t, pad)."""
    rows, n = view.shape
    return view._base.view(rows, n + pad)[:, n:]


def rebased(t: torch.Tensor, row_begin: int, row_end: int, pad: int) -> torch.Tensor:
    """Rows [row_begin, row_end) of t at the start of a buffer of t's own row count (and `pad`
    more elements per row); the other rows hold padded()'s fill.  A kernel that indexed such a
    buffer by the global row would read the fill, inside the buffer."""
    if row_begin == 0 and row_end == t.shape[0]:
        return padded(t, pad)
    buf = _fill(torch.empty((t.shape[0], t.shape[1] + pad), dtype=t.dtype, device=t.device))
    buf[:row_end - row_begin, :t.shape[1]] = t[row_begin:row_end]
    return buf[:, :t.shape[1]]


# A NaN payload no kernel writes (the canonical quiet NaN of a loud failure has none).
SENTINEL = {torch.float32: (torch.int32, 0x7FC0DEAD),
            torch.float64: (torch.int64, 0x7FF80000DEADBEEF),
            torch.bfloat16: (torch.int16, 0x7FCD), torch.float16: (torch.int16, 0x7EAD)}
POISON = {torch.float32: (torch.int32, 0x7FC00000),
          torch.float64: (torch.int64, 0x7FF8000000000000),
          torch.bfloat16: (torch.int16, 0x7FC0), torch.float16: (torch.int16, 0x7E00)}


def sentinel(shape, dtype, dev) -> torch.Tensor:
    it, bits = SENTINEL[dtype]
    return torch.full(shape, bits, dtype=it, device=dev).view(dtype)


def is_sentinel(t: torch.Tensor) -> torch.Tensor:
    """Elementwise: the element still holds sentinel()'s bits."""
    it, bits = SENTINEL[t.dtype]
    return t.contiguous().view(it) == bits


def poisoned(t: torch.Tensor) -> bool:
    """Every element is the canonical quiet NaN of its dtype (a loud failure's fill)."""
    it, bits = POISON[t.dtype]
    return bool((t.contiguous().view(it) == bits).all().item())


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _workspace(query, dev):
    size = ctypes.c_size_t(0)
    query(ctypes.byref(size))
    return torch.empty(max(size.value, 1), dtype=torch.uint8, device=dev), size.value


def _device_workspace(query, dev, ws):
    """The caller's workspace `ws` (a planned launch's), or a fresh one of the queried size."""
    if ws is not None:
        return ws, ws.numel()
    return _workspace(query, dev)


def run_reduce(rp, ci, vals, b, m, k, reduce, *, pad=0, row_begin=0, row_end=None, opts=None,
               want_arg=True, shift=0, ws=None):
    """ofx_spmm_csr_reduce(_cpu) on the tensors' device: (out, arg) for rows [row_begin, row_end),
    with leading dimensions n + pad; b, out and arg start `shift` elements into their buffers.
    ws: the device workspace to launch on (else one of the queried size)."""
    row_end = m if row_end is None else row_end
    code = REDUCE_CODES[reduce]
    dev, n = b.device, b.shape[1]
    bb = padded(b, pad, shift)
    rows = row_end - row_begin
    out = padded(torch.empty((rows, n), dtype=b.dtype, device=dev), pad, shift)
    arg = padded(torch.full((rows, n), -9, dtype=rp.dtype, device=dev), pad, shift) \
        if want_arg else None
    it, vt, nnz = dtype_code(rp.dtype), dtype_code(b.dtype), ci.numel()
    o = ctypes.byref(opts) if opts is not None else None
    tail = (_ptr(rp), _ptr(ci), _ptr(vals), _ptr(bb), n + pad, _ptr(out), n + pad, _ptr(arg),
            n + pad, row_begin, row_end, code)
    if dev.type == "cpu":
        check(LIB.ofx_spmm_csr_reduce_cpu(0, it, vt, m, k, n, nnz, *tail, o), "reduce_cpu")
    else:
        ws, size = _device_workspace(lambda s: check(LIB.ofx_spmm_csr_reduce_workspace_size(
            it, vt, m, k, n, nnz, code, o, s)), dev, ws)
        check(LIB.ofx_spmm_csr_reduce(current_stream_handle(b), it, vt, m, k, n, nnz, *tail,
                                      ws.data_ptr(), size, o), "reduce")
    return out, arg


def run_grad_b(rp_t, ci_t, perm, vals, arg, g, m, k, *, pad=0, opts=None, row_begin=0,
               row_end=None, ws=None):
    """ofx_spmm_csr_select(_cpu): d(b) of A^T's rows [row_begin, row_end) (all k by default),
    row_end - row_begin rows with leading dimensions n + pad; arg and g over all m rows."""
    row_end = k if row_end is None else row_end
    dev, n = g.device, g.shape[1]
    aa, gg = padded(arg, pad), padded(g, pad)
    db = padded(torch.empty((row_end - row_begin, n), dtype=g.dtype, device=dev), pad)
    it, vt, nnz = dtype_code(rp_t.dtype), dtype_code(g.dtype), perm.numel()
    o = ctypes.byref(opts) if opts is not None else None
    tail = (_ptr(rp_t), _ptr(ci_t), _ptr(perm), _ptr(vals), _ptr(aa), n + pad, _ptr(gg), n + pad,
            _ptr(db), n + pad, row_begin, row_end)
    if dev.type == "cpu":
        check(LIB.ofx_spmm_csr_select_cpu(0, it, vt, m, k, n, nnz, *tail, o), "select_cpu")
    else:
        ws, size = _device_workspace(lambda s: check(LIB.ofx_spmm_csr_select_workspace_size(
            it, vt, m, k, n, nnz, o, s)), dev, ws)
        check(LIB.ofx_spmm_csr_select(current_stream_handle(g), it, vt, m, k, n, nnz, *tail,
                                      ws.data_ptr(), size, o), "select")
    return db


def run_grad_values(rp, ci, arg, g, b, m, k, *, pad=0, row_begin=0, row_end=None, out=None):
    """ofx_sddmm_csr_select(_cpu) over A's rows [row_begin, row_end) (all m by default), with
    leading dimensions n + pad: all nnz entries of d(values), those outside the range still
    holding sentinel()'s bits (is_sentinel).  arg and g are given over all m rows; the entry gets
    them rebased to the range, in buffers of m rows (rebased()).  out: the buffer to write to."""
    row_end = m if row_end is None else row_end
    dev, n = b.device, b.shape[1]
    aa, gg = rebased(arg, row_begin, row_end, pad), rebased(g, row_begin, row_end, pad)
    bb = padded(b, pad)
    out = sentinel((ci.numel(),), b.dtype, dev) if out is None else out
    it, vt, nnz = dtype_code(rp.dtype), dtype_code(b.dtype), ci.numel()
    tail = (_ptr(rp), _ptr(ci), _ptr(aa), n + pad, _ptr(gg), n + pad, _ptr(bb), n + pad, _ptr(out),
            row_begin, row_end)
    if dev.type == "cpu":
        check(LIB.ofx_sddmm_csr_select_cpu(0, it, vt, m, k, n, nnz, *tail), "sddmm_select_cpu")
    else:
        ws, size = _workspace(lambda s: check(LIB.ofx_sddmm_csr_workspace_size(
            it, vt, m, n, nnz, s)), dev)
        check(LIB.ofx_sddmm_csr_select(current_stream_handle(b), it, vt, m, k, n, nnz, *tail,
                                       ws.data_ptr(), size), "sddmm_select")
    return out


def run_row_scale(rp, src, m, *, row_begin=0, row_end=None, pad_src=0, pad_dst=0):
    """ofx_row_scale_by_degree(_cpu) out of place on src's device: src holds the rows
    [row_begin, row_end) (leading dimension n + pad_src); returns dst (n + pad_dst), a view of a
    NaN-filled buffer (dst._base)."""
    row_end = m if row_end is None else row_end
    dev, n = src.device, src.shape[1]
    ss = padded(src, pad_src)
    dst = padded(torch.empty_like(src), pad_dst)
    it, vt = dtype_code(rp.dtype), dtype_code(src.dtype)
    tail = (it, vt, m, n, _ptr(rp), _ptr(ss), n + pad_src, _ptr(dst), n + pad_dst, row_begin,
            row_end)
    if dev.type == "cpu":
        check(LIB.ofx_row_scale_by_degree_cpu(0, *tail), "row_scale_cpu")
    else:
        check(LIB.ofx_row_scale_by_degree(current_stream_handle(src), *tail), "row_scale")
    return dst


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


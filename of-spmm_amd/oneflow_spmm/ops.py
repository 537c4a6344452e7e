"""Direct C-ABI entry points (below the op layer): the device kernel with explicit schedule
options and workspace, the CPU kernel, CSR validation and row slicing.  Used by the row-split
wrapper, the benchmark and the parity tests; `oneflow_spmm.spmm` is the op-level API.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._C import FP8_FORMATS, current_stream_handle, dtype_code
from ._lib import LIB, Options, check

INT64_MAX = (1 << 63) - 1


def make_options(split: int = 0, chunk: int = 0, ordered: bool = False, variant: int = 0,
                 heavy: int = 0, planned: bool = False, range_nnz: int = 0) -> Options:
    """heavy: rows longer than this (not split) are scheduled first; 0 = default, <0 = off.
    planned: the workspace holds ofx_spmm_csr_plan's work list (see SpmmCsrKernel.plan).
    range_nnz: the launch's row range holds this many nonzeros (0 = estimated as its share of
    nnz); picks the kernel form only."""
    return Options(int(split), int(chunk), 1 if ordered else 0, int(variant), int(heavy),
                   1 if planned else 0, 0, int(range_nnz))


def _with(o: Options | None, **fields) -> Options:
    """A copy of options `o` (None: the defaults) with `fields` replaced."""
    c = Options()
    if o is not None:
        ctypes.memmove(ctypes.addressof(c), ctypes.addressof(o), ctypes.sizeof(Options))
    for key, val in fields.items():
        setattr(c, key, val)
    return c


def _nz(t):
    """The data pointer of a tensor, NULL for None or an empty one."""
    return t.data_ptr() if t is not None and t.numel() else None


def _workspace(device, what, query, *args, workspace_bytes: int | None = None):
    """(buffer, bytes) of one device launch: the size `query(*args, &size)` answers, or
    workspace_bytes if given (the query is still made), in a buffer of max(bytes, 1) bytes."""
    size = ctypes.c_size_t(0)
    check(query(*args, ctypes.byref(size)), what)
    ws = size.value if workspace_bytes is None else int(workspace_bytes)
    return torch.empty(max(ws, 1), dtype=torch.uint8, device=device), ws


def default_split(n: int) -> int:
    return int(LIB.ofx_spmm_default_split(int(n)))


def workspace_size(idx_dtype: torch.dtype, val_dtype: torch.dtype, m: int, k: int, n: int, nnz: int,
                   options: Options | None = None) -> int:
    out = ctypes.c_size_t(0)
    check(LIB.ofx_spmm_csr_workspace_size(dtype_code(idx_dtype), dtype_code(val_dtype), m, k, n, nnz,
                                          ctypes.byref(options) if options else None,
                                          ctypes.byref(out)), "workspace_size")
    return out.value


class SpmmCsrKernel:
    """Holds the workspace for repeated launches of one problem shape (the OneFlow tmp buffer).

    plan(row_ptr, row_begin, row_end) builds the work list once (ofx_spmm_csr_plan) for a static
    graph; launches with planned=True on that same row_ptr tensor and row range then skip the
    planning kernel.  The caller promises row_ptr's contents have not changed (a bound
    CSR); the tensor identity and range are checked here."""

    def __init__(self, m: int, k: int, n: int, nnz: int, idx_dtype: torch.dtype,
                 val_dtype: torch.dtype, device, options: Options | None = None):
        self.m, self.k, self.n, self.nnz = m, k, n, nnz
        self.idx_dt, self.val_dt = dtype_code(idx_dtype), dtype_code(val_dtype)
        self.options = options
        ws = workspace_size(idx_dtype, val_dtype, m, k, n, nnz, options)
        self.workspace = torch.empty(max(ws, 1), dtype=torch.uint8, device=device)
        self.ws_bytes = ws
        self._planned_for = None
        self._planned_opts = None

    def plan(self, row_ptr, row_begin=0, row_end=None, stream=None, range_nnz: int = 0):
        row_end = self.m if row_end is None else row_end
        s = stream if stream is not None else current_stream_handle(row_ptr)
        o = _with(self.options, range_nnz=int(range_nnz)) if range_nnz else self.options
        check(LIB.ofx_spmm_csr_plan(s, self.idx_dt, self.val_dt, self.m, self.k, self.n, self.nnz,
                                    row_ptr.data_ptr(), row_begin, row_end,
                                    self.workspace.data_ptr(), self.ws_bytes,
                                    ctypes.byref(o) if o else None),
              "spmm_csr_plan")
        self._planned_opts = _with(o, planned=1)
        self._planned_for = (row_ptr.data_ptr(), row_ptr.numel(), row_begin, row_end, int(range_nnz))
        return self

    def launch_options(self, row_ptr, row_begin, row_end, planned: bool, range_nnz: int = 0):
        """The options struct of one launch (the planned form after a matching plan())."""
        if not planned:
            return _with(self.options, range_nnz=int(range_nnz)) if range_nnz else self.options
        if self._planned_for != (row_ptr.data_ptr(), row_ptr.numel(), row_begin, row_end,
                                 int(range_nnz)):
            raise RuntimeError("SpmmCsrKernel: planned launch without a plan() of this row_ptr, "
                               "row range and range_nnz")
        return self._planned_opts

    def __call__(self, row_ptr, col_idx, values, b, out, row_begin=0, row_end=None, stream=None,
                 bias=None, relu=False, planned: bool = False, range_nnz: int = 0):
        """bias / relu: the fused epilogue (ofx_spmm_csr_fused); none = the plain op.
        range_nnz: nonzeros of [row_begin, row_end) if known (the form choice; 0 = estimated)."""
        row_end = self.m if row_end is None else row_end
        s = stream if stream is not None else current_stream_handle(b)
        opts = self.launch_options(row_ptr, row_begin, row_end, planned, range_nnz)
        check(LIB.ofx_spmm_csr_fused(s, self.idx_dt, self.val_dt, self.m, self.k, self.n, self.nnz,
                                     row_ptr.data_ptr(), col_idx.data_ptr() if col_idx.numel() else None,
                                     values.data_ptr() if values.numel() else None,
                                     b.data_ptr() if b.numel() else None, b.stride(0), out.data_ptr(),
                                     out.stride(0), row_begin, row_end,
                                     bias.data_ptr() if bias is not None else None, 1 if relu else 0,
                                     self.workspace.data_ptr(), self.ws_bytes,
                                     ctypes.byref(opts) if opts else None),
              "spmm_csr")
        return out


def spmm_csr_device(row_ptr, col_idx, values, b, m, k, *, out=None, row_begin=0, row_end=None,
                    options: Options | None = None):
    """One launch of the HIP kernel (C-ABI ofx_spmm_csr) on torch's current stream."""
    if b.device.type != "cuda":
        raise RuntimeError("spmm_csr_device: HIP kernel needs device tensors")
    row_end = m if row_end is None else row_end
    if out is None:
        out = torch.empty((row_end - row_begin, b.shape[1]), dtype=b.dtype, device=b.device)
    kern = SpmmCsrKernel(m, k, b.shape[1], col_idx.numel(), row_ptr.dtype, b.dtype, b.device, options)
    return kern(row_ptr, col_idx, values, b, out, row_begin, row_end)


def describe(m: int, k: int, n: int, nnz: int, val_dtype: torch.dtype,
             idx_dtype: torch.dtype = torch.int32, *, row_begin: int = 0, row_end: int | None = None,
             ldb: int | None = None, ldc: int | None = None, b_addr: int = 256, c_addr: int = 256,
             options: Options | None = None) -> dict:
    """The configuration an ofx_spmm_csr launch with these arguments takes (ofx_spmm_csr_describe):
    {"form": "small"|"mid"|"narrow"|"prefetch"|"bandwidth", "kernel": ..., "VEC": .., "LPR": ..,
    "U": .., flags ...}.  Nothing is launched; b_addr / c_addr only set the pointer alignment the
    width dispatch sees (256: aligned)."""
    row_end = m if row_end is None else row_end
    buf = ctypes.create_string_buffer(512)
    check(LIB.ofx_spmm_csr_describe(dtype_code(idx_dtype), dtype_code(val_dtype), m, k, n, nnz,
                                    b_addr, ldb or n, c_addr, ldc or n, row_begin, row_end,
                                    ctypes.byref(options) if options else None, buf, len(buf)),
          "spmm_csr_describe")
    out = {}
    for kv in buf.value.decode().split():
        key, val = kv.split("=")
        out[key] = int(val) if val.lstrip("-").isdigit() else val
    return out


def spmm_csr_gathered(row_ptr, col_idx, values, values_perm, b, m, k, *, out=None,
                      options: Options | None = None):
    """out = A @ b where nonzero j's value is values[values_perm[j]] (ofx_spmm_csr_gathered):
    the backward's A^T @ d(out) on A's values without writing values[perm].  Same bits as
    spmm_csr on the gathered values."""
    if b.device.type != "cuda":
        return spmm_csr_cpu(row_ptr, col_idx, values[values_perm.long()], b, m, k, out=out,
                            options=options)
    if values_perm.dtype != row_ptr.dtype or values_perm.numel() != col_idx.numel():
        raise RuntimeError("spmm_csr_gathered: values_perm must be [nnz] in the index dtype")
    if out is None:
        out = torch.empty((m, b.shape[1]), dtype=b.dtype, device=b.device)
    n, nnz = b.shape[1], col_idx.numel()
    idt, vdt = dtype_code(row_ptr.dtype), dtype_code(b.dtype)
    popt = ctypes.byref(options) if options else None
    wbuf, ws = _workspace(b.device, "workspace_size", LIB.ofx_spmm_csr_workspace_size, idt, vdt,
                          m, k, n, nnz, popt)
    check(LIB.ofx_spmm_csr_gathered(current_stream_handle(b), idt, vdt, m, k, n, nnz,
                                    row_ptr.data_ptr(), _nz(col_idx), _nz(values),
                                    _nz(values_perm), _nz(b), b.stride(0), out.data_ptr(),
                                    out.stride(0), 0, m, wbuf.data_ptr(), ws, popt),
          "spmm_csr_gathered")
    return out


def relu_bias_grad(y, dy, *, relu: bool, bias_grad: bool, num_threads: int = 0):
    """Backward of the fused epilogue (ofx_relu_bias_grad[_cpu]): returns (dx, d_bias).
    dx = relu ? where(y > 0, dy, 0) : dy (dy itself when relu is off); d_bias = column sum of dx
    in the contract's fixed order, or None."""
    m, n = dy.shape
    dt = dtype_code(dy.dtype)
    dx = torch.empty_like(dy) if relu else dy
    db = torch.empty(n, dtype=dy.dtype, device=dy.device) if bias_grad else None
    if not relu and not bias_grad:
        return dx, db
    yy = y if relu else None
    args = (m, n, _nz(yy), yy.stride(0) if yy is not None else n, _nz(dy), dy.stride(0),
            _nz(dx) if relu else None, dx.stride(0) if relu else n, _nz(db), 1 if relu else 0)
    if dy.device.type == "cpu":
        check(LIB.ofx_relu_bias_grad_cpu(int(num_threads), dt, *args), "relu_bias_grad")
        return dx, db
    wbuf, ws = _workspace(dy.device, "relu_bias_grad", LIB.ofx_relu_bias_grad_workspace_size, dt,
                          m, n)
    check(LIB.ofx_relu_bias_grad(current_stream_handle(dy), dt, *args, wbuf.data_ptr(), ws),
          "relu_bias_grad")
    return dx, db


def spmm_csr_cpu(row_ptr, col_idx, values, b, m, k, *, out=None, row_begin=0, row_end=None,
                 options: Options | None = None, num_threads: int = 0, bias=None, relu=False):
    """The DeviceType::kCPU kernel (C-ABI ofx_spmm_csr_fused_cpu), host tensors."""
    row_end = m if row_end is None else row_end
    if out is None:
        out = torch.empty((row_end - row_begin, b.shape[1]), dtype=b.dtype)
    check(LIB.ofx_spmm_csr_fused_cpu(int(num_threads), dtype_code(row_ptr.dtype), dtype_code(b.dtype),
                                     m, k, b.shape[1], col_idx.numel(), row_ptr.data_ptr(),
                                     col_idx.data_ptr() if col_idx.numel() else None,
                                     values.data_ptr() if values.numel() else None,
                                     b.data_ptr() if b.numel() else None, b.stride(0), out.data_ptr(),
                                     out.stride(0), row_begin, row_end,
                                     bias.data_ptr() if bias is not None else None, 1 if relu else 0,
                                     ctypes.byref(options) if options else None), "spmm_csr_cpu")
    return out


def spmm_csr_heads(row_ptr, col_idx, values, b, m, k, heads, *, out=None, row_begin=0,
                   row_end=None, options: Options | None = None, num_threads: int = 0,
                   workspace_bytes: int | None = None):
    """The multi-head SpMM at the C-ABI (ofx_spmm_csr_heads on device tensors, the kCPU kernel
    ofx_spmm_csr_heads_cpu on host tensors): values [nnz, heads] contiguous, b [K, heads * D] with
    unit column stride -> out [row_end - row_begin, heads * D].  workspace_bytes: the device
    workspace to pass instead of the query's size (tests)."""
    row_end = m if row_end is None else row_end
    n, nnz = b.shape[1], col_idx.numel()
    d = n // heads if heads else 0
    if out is None:
        out = torch.empty((row_end - row_begin, n), dtype=b.dtype, device=b.device)
    idt, vdt = dtype_code(row_ptr.dtype), dtype_code(b.dtype)
    popt = ctypes.byref(options) if options else None
    body = (idt, vdt, m, k, heads, d, nnz, row_ptr.data_ptr(), _nz(col_idx), _nz(values), _nz(b),
            b.stride(0), out.data_ptr(), out.stride(0), row_begin, row_end)
    if b.device.type == "cpu":
        check(LIB.ofx_spmm_csr_heads_cpu(int(num_threads), *body, popt), "spmm_csr_heads_cpu")
        return out
    wbuf, ws = _workspace(b.device, "spmm_csr_heads", LIB.ofx_spmm_csr_heads_workspace_size, idt,
                          vdt, m, k, heads, d, nnz, popt, workspace_bytes=workspace_bytes)
    check(LIB.ofx_spmm_csr_heads(current_stream_handle(b), *body, wbuf.data_ptr(), ws, popt),
          "spmm_csr_heads")
    return out


def spmm_csr_heads_fp8(row_ptr, col_idx, values, b_q, b_scale, m, k, heads, *, b_format=None,
                       val_dtype=None, out=None, row_begin=0, row_end=None,
                       options: Options | None = None, num_threads: int = 0,
                       workspace_bytes: int | None = None):
    """The multi-head SpMM over an FP8 table at the C-ABI (ofx_spmm_csr_heads_fp8 on device
    tensors, the kCPU kernel ofx_spmm_csr_heads_fp8_cpu on host tensors): values [nnz, heads]
    contiguous, b_q [K, heads * D] of a torch FP8 dtype (or uint8 codes with b_format given) with
    unit column stride, b_scale float32 [K] or None -> out [row_end - row_begin, heads * D] of
    values' dtype.  b_format / val_dtype: the codes to pass instead of the tensors' own;
    workspace_bytes: the device workspace to pass instead of the query's size (tests)."""
    row_end = m if row_end is None else row_end
    n, nnz = b_q.shape[1], col_idx.numel()
    d = n // heads if heads else 0
    if out is None:
        out = torch.empty((row_end - row_begin, n), dtype=values.dtype, device=values.device)
    fmt = FP8_FORMATS[b_q.dtype] if b_format is None else int(b_format)
    idt = dtype_code(row_ptr.dtype)
    vdt = dtype_code(values.dtype) if val_dtype is None else int(val_dtype)
    popt = ctypes.byref(options) if options else None
    body = (idt, vdt, fmt, m, k, heads, d, nnz, row_ptr.data_ptr(), _nz(col_idx), _nz(values),
            _nz(b_q), b_q.stride(0), _nz(b_scale), _nz(out), out.stride(0), row_begin, row_end)
    if values.device.type == "cpu":
        check(LIB.ofx_spmm_csr_heads_fp8_cpu(int(num_threads), *body, popt),
              "spmm_csr_heads_fp8_cpu")
        return out
    wbuf, ws = _workspace(values.device, "spmm_csr_heads_fp8",
                          LIB.ofx_spmm_csr_heads_fp8_workspace_size, idt, vdt, fmt, m, k, heads, d,
                          nnz, popt, workspace_bytes=workspace_bytes)
    check(LIB.ofx_spmm_csr_heads_fp8(current_stream_handle(values), *body, wbuf.data_ptr(), ws,
                                     popt), "spmm_csr_heads_fp8")
    return out


def sddmm_csr_heads(row_ptr, col_idx, a, b, m, k, heads, *, out=None, row_begin=0, row_end=None,
                    num_threads: int = 0, workspace_bytes: int | None = None):
    """The multi-head SDDMM at the C-ABI (ofx_sddmm_csr_heads / ofx_sddmm_csr_heads_cpu by device):
    a holds rows [row_begin, row_end) of the left operand, out is [nnz, heads] and a row range
    writes its own nonzeros' rows of it."""
    row_end = m if row_end is None else row_end
    n, nnz = b.shape[1], col_idx.numel()
    d = n // heads if heads else 0
    if out is None:
        out = torch.empty((nnz, heads), dtype=b.dtype, device=b.device)
    idt, vdt = dtype_code(row_ptr.dtype), dtype_code(b.dtype)
    body = (idt, vdt, m, k, heads, d, nnz, row_ptr.data_ptr(), _nz(col_idx), _nz(a), a.stride(0),
            _nz(b), b.stride(0), _nz(out), row_begin, row_end)
    if b.device.type == "cpu":
        check(LIB.ofx_sddmm_csr_heads_cpu(int(num_threads), *body), "sddmm_csr_heads_cpu")
        return out
    wbuf, ws = _workspace(b.device, "sddmm_csr_heads", LIB.ofx_sddmm_csr_heads_workspace_size,
                          idt, vdt, m, heads, d, nnz, workspace_bytes=workspace_bytes)
    check(LIB.ofx_sddmm_csr_heads(current_stream_handle(b), *body, wbuf.data_ptr(), ws),
          "sddmm_csr_heads")
    return out


def graph_attention_csr_heads(row_ptr, col_idx, q, k_mat, v, m, k, heads, *, out=None, attn=None,
                              row_begin=0, row_end=None, options: Options | None = None,
                              num_threads: int = 0, workspace_bytes: int | None = None):
    """The fused multi-head graph attention at the C-ABI (ofx_graph_attention_csr_heads on device
    tensors, the kCPU kernel ofx_graph_attention_csr_heads_cpu on host tensors): q holds rows
    [row_begin, row_end) of the queries, k_mat and v are [K, heads * D], all with unit column
    stride -> (out [row_end - row_begin, heads * D], attn [nnz, heads]); a row range writes its own
    nonzeros' rows of attn.  workspace_bytes: the device workspace to pass instead of the query's
    size (tests)."""
    row_end = m if row_end is None else row_end
    n, nnz = k_mat.shape[1], col_idx.numel()
    d = n // heads if heads else 0
    if out is None:
        out = torch.empty((row_end - row_begin, n), dtype=k_mat.dtype, device=k_mat.device)
    if attn is None:
        attn = torch.empty((nnz, heads), dtype=k_mat.dtype, device=k_mat.device)
    idt, vdt = dtype_code(row_ptr.dtype), dtype_code(k_mat.dtype)
    popt = ctypes.byref(options) if options else None
    body = (idt, vdt, m, k, heads, d, nnz, row_ptr.data_ptr(), _nz(col_idx), _nz(q), q.stride(0),
            _nz(k_mat), k_mat.stride(0), _nz(v), v.stride(0), _nz(out), out.stride(0), _nz(attn),
            row_begin, row_end)
    if k_mat.device.type == "cpu":
        check(LIB.ofx_graph_attention_csr_heads_cpu(int(num_threads), *body, popt),
              "graph_attention_csr_heads_cpu")
        return out, attn
    wbuf, ws = _workspace(k_mat.device, "graph_attention_csr_heads",
                          LIB.ofx_graph_attention_csr_heads_workspace_size, idt, vdt, m, k, heads,
                          d, nnz, popt, workspace_bytes=workspace_bytes)
    check(LIB.ofx_graph_attention_csr_heads(current_stream_handle(k_mat), *body, wbuf.data_ptr(),
                                            ws, popt), "graph_attention_csr_heads")
    return out, attn


def gatv2_scores_csr_heads(row_ptr, col_idx, x_row, x_col, att, m, k, heads, negative_slope=0.2, *,
                           out=None, row_begin=0, row_end=None, num_threads: int = 0,
                           workspace_bytes: int | None = None):
    """The GATv2 scores at the C-ABI (ofx_gatv2_scores_csr_heads on device tensors, the kCPU kernel
    ofx_gatv2_scores_csr_heads_cpu on host tensors): x_row holds rows [row_begin, row_end) of the
    destination features, x_col is [K, heads * D] (unit column stride both), att [heads * D] ->
    out [nnz, heads]; a row range writes its own nonzeros' rows of it."""
    row_end = m if row_end is None else row_end
    n, nnz = x_col.shape[1], col_idx.numel()
    d = n // heads if heads else 0
    if out is None:
        out = torch.empty((nnz, heads), dtype=x_col.dtype, device=x_col.device)
    idt, vdt = dtype_code(row_ptr.dtype), dtype_code(x_col.dtype)
    body = (idt, vdt, m, k, heads, d, nnz, row_ptr.data_ptr(), _nz(col_idx), _nz(x_row),
            x_row.stride(0), _nz(x_col), x_col.stride(0), _nz(att), float(negative_slope), _nz(out),
            row_begin, row_end)
    if x_col.device.type == "cpu":
        check(LIB.ofx_gatv2_scores_csr_heads_cpu(int(num_threads), *body),
              "gatv2_scores_csr_heads_cpu")
        return out
    wbuf, ws = _workspace(x_col.device, "gatv2_scores_csr_heads",
                          LIB.ofx_gatv2_scores_csr_heads_workspace_size, idt, vdt, m, heads, d,
                          nnz, workspace_bytes=workspace_bytes)
    check(LIB.ofx_gatv2_scores_csr_heads(current_stream_handle(x_col), *body, wbuf.data_ptr(), ws),
          "gatv2_scores_csr_heads")
    return out


def gatv2_scores_csr_heads_grad(row_ptr, col_idx, x_row, x_col, att, de, m, k, heads,
                                negative_slope=0.2, *, with_att=True, d_x=None, p=None,
                                row_begin=0, row_end=None, options: Options | None = None,
                                num_threads: int = 0, workspace_bytes: int | None = None):
    """The gradient of the GATv2 scores at the C-ABI (ofx_gatv2_scores_csr_heads_grad /
    ofx_gatv2_scores_csr_heads_grad_cpu by device): de [nnz, heads] -> (d_x, p), both
    [row_end - row_begin, heads * D]; p is None unless with_att (or a p is passed)."""
    row_end = m if row_end is None else row_end
    n, nnz = x_col.shape[1], col_idx.numel()
    d = n // heads if heads else 0
    if d_x is None:
        d_x = torch.empty((row_end - row_begin, n), dtype=x_col.dtype, device=x_col.device)
    if p is None and with_att:
        p = torch.empty((row_end - row_begin, n), dtype=x_col.dtype, device=x_col.device)
    idt, vdt = dtype_code(row_ptr.dtype), dtype_code(x_col.dtype)
    popt = ctypes.byref(options) if options else None
    body = (idt, vdt, m, k, heads, d, nnz, row_ptr.data_ptr(), _nz(col_idx), _nz(x_row),
            x_row.stride(0), _nz(x_col), x_col.stride(0), _nz(att), float(negative_slope), _nz(de),
            _nz(d_x), d_x.stride(0), _nz(p), p.stride(0) if p is not None else n, row_begin,
            row_end)
    if x_col.device.type == "cpu":
        check(LIB.ofx_gatv2_scores_csr_heads_grad_cpu(int(num_threads), *body, popt),
              "gatv2_scores_csr_heads_grad_cpu")
        return d_x, p
    wbuf, ws = _workspace(x_col.device, "gatv2_scores_csr_heads_grad",
                          LIB.ofx_gatv2_scores_csr_heads_grad_workspace_size, idt, vdt, m, k, heads,
                          d, nnz, 1 if p is not None else 0, popt, workspace_bytes=workspace_bytes)
    check(LIB.ofx_gatv2_scores_csr_heads_grad(current_stream_handle(x_col), *body, wbuf.data_ptr(),
                                              ws, popt), "gatv2_scores_csr_heads_grad")
    return d_x, p


def validate_csr(row_ptr, col_idx, m, k) -> int:
    """Device-side CSR check; returns 0 ok, 1 bad row_ptr, 2 column out of range (syncs)."""
    flag = torch.zeros(1, dtype=torch.int32, device=row_ptr.device)
    check(LIB.ofx_csr_validate(current_stream_handle(row_ptr), dtype_code(row_ptr.dtype), m, k,
                               col_idx.numel(), row_ptr.data_ptr(),
                               col_idx.data_ptr() if col_idx.numel() else None, flag.data_ptr()),
          "csr_validate")
    return int(flag.item())


def csr_row_slice(row_ptr, row_begin: int, row_end: int):
    """Rebased row_ptr of rows [row_begin, row_end) (+ the nnz range it covers)."""
    out = torch.empty(row_end - row_begin + 1, dtype=row_ptr.dtype, device=row_ptr.device)
    if row_ptr.device.type == "cpu":
        lo, hi = ctypes.c_int64(), ctypes.c_int64()
        check(LIB.ofx_csr_row_slice_host(dtype_code(row_ptr.dtype), row_ptr.data_ptr(), row_begin,
                                         row_end, out.data_ptr(), ctypes.byref(lo), ctypes.byref(hi)),
              "csr_row_slice")
        return out, lo.value, hi.value
    check(LIB.ofx_csr_row_slice(current_stream_handle(row_ptr), dtype_code(row_ptr.dtype),
                                row_ptr.data_ptr(), row_begin, row_end, out.data_ptr()),
          "csr_row_slice")
    return out, None, None


__all__ = ["make_options", "default_split", "workspace_size", "SpmmCsrKernel", "spmm_csr_device",
           "describe",
           "spmm_csr_gathered", "spmm_csr_heads", "spmm_csr_heads_fp8", "sddmm_csr_heads", "gatv2_scores_csr_heads",
           "gatv2_scores_csr_heads_grad",
           "spmm_csr_cpu", "validate_csr", "csr_row_slice", "INT64_MAX", "_lib"]

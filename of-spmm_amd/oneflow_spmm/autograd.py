"""Gradients of `spmm_csr`: d(values) by SDDMM, d(b) by SpMM with A^T.

Mirrors what a OneFlow gradient function for the op would do (pattern
oneflow/core/autograd/gradient_funcs/matrix_vector_product.cpp:26-91: capture what the backward
needs, then call the grad functors): for out = A @ b,
    d(values)[j] = <d(out)[row(j), :], b[col(j), :]>      ofx_sddmm_csr
    d(b)         = A^T @ d(out)                            ofx_csr_transpose (cached per graph)
                                                           + ofx_spmm_csr_gathered (values read
                                                           through perm), or ofx_gather_values
                                                           once + ofx_spmm_csr for constant values
The index inputs never get gradients (spmm_op.cpp ModifyInputArg).  All device work runs in the
HIP kernels; CPU tensors run the kCPU kernels.  Both give the same bits (contracts in
include/ofx_spmm.h).
"""
from __future__ import annotations

from collections import OrderedDict

import torch

from . import _C, ops
from ._C import current_stream_handle, dtype_code, spmm_csr
from ._lib import LIB, check


# ---- building blocks ----------------------------------------------------------------------------
def csr_transpose(row_ptr: torch.Tensor, col_idx: torch.Tensor, k: int):
    """Structure of A^T: (row_ptr_T [k+1], col_idx_T [nnz] = rows of A, perm [nnz]).
    Op "csr_transpose" through the op layer (CPU or HIP kernel by device)."""
    return _C.csr_transpose(row_ptr, col_idx, row_ptr.numel() - 1, k)


def gather_values(perm: torch.Tensor, values: torch.Tensor) -> torch.Tensor:
    """values[perm] (device kernel on GPU)."""
    if values.device.type == "cpu":
        return values[perm.long()]
    out = torch.empty_like(values)
    check(LIB.ofx_gather_values(current_stream_handle(values), dtype_code(perm.dtype),
                                dtype_code(values.dtype), values.numel(),
                                perm.data_ptr() if perm.numel() else None,
                                values.data_ptr() if values.numel() else None,
                                out.data_ptr() if out.numel() else None), "gather_values")
    return out


def _gather_rows(perm: torch.Tensor, values: torch.Tensor) -> torch.Tensor:
    """The rows values[perm] of a contiguous [nnz, H] tensor (ofx_gather_rows on the device, a
    torch index on the host: plumbing, not hot path)."""
    if values.device.type == "cpu" or values.numel() == 0:
        return values.index_select(0, perm.long())
    out = torch.empty_like(values)
    row_bytes = values.shape[1] * values.element_size()
    check(LIB.ofx_gather_rows(current_stream_handle(values), dtype_code(perm.dtype),
                              values.shape[0], row_bytes, perm.data_ptr(), values.data_ptr(),
                              row_bytes, out.data_ptr(), row_bytes), "gather_rows")
    return out


def _recording(op: str, out, *tensors) -> bool:
    """Whether gradients are being recorded for any of `tensors` (None: an absent input), the
    dispatch decision of every public op; `out=` is refused then."""
    if not torch.is_grad_enabled():
        return False
    for t in tensors:
        if t is not None and t.requires_grad:
            if out is not None:
                raise RuntimeError(f"{op}: out= is not supported when gradients are required")
            return True
    return False


def _heads_2d(t: torch.Tensor, name: str) -> torch.Tensor:
    """A [rows, H, D] tensor made contiguous and viewed as [rows, H*D]."""
    if t.dim() != 3:
        raise RuntimeError(f"{name} should be 3-D [rows, heads, D], got shape {tuple(t.shape)}")
    return t.contiguous().view(t.shape[0], t.shape[1] * t.shape[2])


def sddmm(row_ptr: torch.Tensor, col_idx: torch.Tensor, a: torch.Tensor, b: torch.Tensor,
          static_csr: int = 0) -> torch.Tensor:
    """out[j] = <a[row(j), :], b[col_idx[j], :]>: op "sddmm_csr" through the op layer
    (`static_csr`: the forward's promise that the CSR is unchanged; its SDDMM plan is kept).
    Differentiable in a and b when one of them requires a gradient (the scores of a dot-product
    attention layer: SddmmCsrFunction).

    Multi-head: a [M, H, D] and b [K, H, D] give out [nnz, H] with out[j, h] = <a[row(j), h, :],
    b[col_idx[j], h, :]> in one launch (op "sddmm_csr_heads"), every head with the bits of the
    2-D call on its slice; `static_csr` is accepted and has no effect there."""
    if a.dim() == 3:
        if b.dim() != 3 or a.shape[1:] != b.shape[1:]:
            raise RuntimeError("sddmm: a [M, H, D] needs b [K, H, D] with the same heads and D, "
                               f"got {tuple(a.shape)} and {tuple(b.shape)}")
        heads = a.shape[1]
        if _recording("sddmm", None, a, b):
            return SddmmCsrHeadsFunction.apply(row_ptr, col_idx, a, b)
        return _C.sddmm_csr_heads(row_ptr, col_idx, _heads_2d(a, "a"), _heads_2d(b, "b"), heads)
    if _recording("sddmm", None, a, b):
        return SddmmCsrFunction.apply(row_ptr, col_idx, a, b, int(static_csr))
    return _C.sddmm_csr(row_ptr, col_idx, a, b, row_ptr.numel() - 1, b.shape[0],
                        static_csr=static_csr)


# ---- transpose cache (the sparsity pattern of a GNN graph is static across layers/steps) -------
class _TransposeCache:
    def __init__(self, capacity: int = 4):
        self.capacity = capacity
        self.static_ids: dict = {}  # id(row_ptr_T) -> its static_csr value (while cached)
        self._next_id = 1 << 40  # clear of the small values callers pass
        self.entries: OrderedDict = OrderedDict()
        self.value_entries: OrderedDict = OrderedDict()
        self.seen: OrderedDict = OrderedDict()  # value keys met once (not yet worth a copy)

    def _insert(self, d: OrderedDict, key, item) -> list:
        """d[key] = item, bounded: the oldest entries beyond `capacity` leave and are returned."""
        d[key] = item
        return [d.popitem(last=False)[1] for _ in range(len(d) - self.capacity)]

    def get(self, row_ptr, col_idx, k):
        key = (row_ptr.data_ptr(), col_idx.data_ptr(), row_ptr._version, col_idx._version,
               row_ptr.numel(), col_idx.numel(), k, str(row_ptr.device))
        hit = self.entries.get(key)
        if hit is not None:
            self.entries.move_to_end(key)
            return hit[2]
        t = csr_transpose(row_ptr, col_idx, k)
        # keep the source tensors alive so their storage (and so the key) cannot be reused; the
        # entry's A^T is static while it lives, so its SpMMs run with static_csr = a value no
        # other entry ever had (a later transpose at recycled addresses gets a new one)
        self._next_id += 1
        self.static_ids[id(t[0])] = self._next_id
        for _, _, old in self._insert(self.entries, key, (row_ptr, col_idx, t)):
            self.static_ids.pop(id(old[0]), None)
        return t

    def static_id(self, rp_t) -> int:
        """The static_csr value of a cached A^T (0 if it is not cached any more)."""
        return self.static_ids.get(id(rp_t), 0)

    @staticmethod
    def _values_key(row_ptr, col_idx, k, values):
        return (row_ptr.data_ptr(), col_idx.data_ptr(), row_ptr._version, col_idx._version, k,
                values.data_ptr(), values._version, values.dtype, tuple(values.shape),
                str(values.device))

    def transposed_values(self, row_ptr, col_idx, values, k, first_sight):
        """(row_ptr_T, col_idx_T, perm, A^T's values = values[perm]) for values [nnz] or a
        contiguous [nnz, H].  Edge weights of a GNN (GCN normalisation, constant attention
        weights) are usually constant across steps, so values met again unchanged keep their
        gathered copy, keyed on the values tensor's storage and version (an in-place update
        invalidates it); values new every step (learnable weights, upstream gradients) are not
        worth one.  `first_sight` is what values met for the first time get:
          "fused":  no copy at all, None is returned (the caller reads them through perm);
          "gather": a copy that is not kept;
          "cache":  a copy kept at once.
        A copy gathered while the current stream is capturing is used but never stored, nor is
        its sighting: it lives in the graph's pool."""
        rp_t, ci_t, perm = self.get(row_ptr, col_idx, k)
        key = self._values_key(row_ptr, col_idx, k, values)
        hit = self.value_entries.get(key)
        if hit is not None:
            self.value_entries.move_to_end(key)
            return rp_t, ci_t, perm, hit[1]
        again = first_sight == "cache" or key in self.seen
        if first_sight == "fused" and not again:
            self._insert(self.seen, key, values)  # holds values: its storage cannot be reused
            return rp_t, ci_t, perm, None
        vals_t = gather_values(perm, values) if values.dim() == 1 else _gather_rows(perm, values)
        if not (values.device.type == "cuda" and torch.cuda.is_current_stream_capturing()):
            if again:
                self._insert(self.value_entries, key, (values, vals_t))  # holds values, as seen
            else:
                self._insert(self.seen, key, values)
        return rp_t, ci_t, perm, vals_t

    def grad_b(self, row_ptr, col_idx, values, m, k, d_out):
        """d(b) = A^T @ d(out) for values [nnz].  On the GPU, values met for the first time are
        read through the transpose's perm inside the SpMM (ofx_spmm_csr_gathered: no
        values[perm] copy written); values met again are gathered once and cached, then the
        plain SpMM runs on them.  On the CPU the copy is cached at once.  Every route gives the
        same bits.  The cached A^T's structure is static while its entry lives: its plan is kept
        across steps (static_csr, a value unique to the entry)."""
        rp_t, ci_t, perm, vals_t = self.transposed_values(
            row_ptr, col_idx, values, k, "fused" if values.device.type == "cuda" else "cache")
        if vals_t is None:
            return _C.spmm_csr_gathered(rp_t, ci_t, values, perm, k, m, d_out,
                                        static_csr=self.static_id(rp_t))
        return spmm_csr(rp_t, ci_t, vals_t, k, m, d_out, static_csr=self.static_id(rp_t))

    def grad_b_heads(self, row_ptr, col_idx, values, m, k, x):
        """A(values)^T @ x per head for values [nnz, H]: op "spmm_csr_heads" on the cached
        transpose with the rows values[perm], gathered every time until the values are met again
        unchanged."""
        rp_t, ci_t, _, vals_t = self.transposed_values(row_ptr, col_idx, values.contiguous(), k,
                                                       "gather")
        return _C.spmm_csr_heads(rp_t, ci_t, vals_t, k, m, x)


TRANSPOSE_CACHE = _TransposeCache()
_heads_grad_b = TRANSPOSE_CACHE.grad_b_heads  # the former name, for callers that still use it


class SpmmCsrFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, row_ptr, col_idx, values, m, k, b, static_csr=0):
        out = spmm_csr(row_ptr, col_idx, values, m, k, b, static_csr=static_csr)
        ctx.save_for_backward(row_ptr, col_idx, values, b)
        ctx.m, ctx.k, ctx.static_csr = m, k, static_csr
        return out

    @staticmethod
    def backward(ctx, d_out):
        row_ptr, col_idx, values, b = ctx.saved_tensors
        d_out = d_out.contiguous()
        d_values = d_b = None
        if ctx.needs_input_grad[2]:
            d_values = sddmm(row_ptr, col_idx, d_out, b, ctx.static_csr)
        if ctx.needs_input_grad[5]:
            d_b = TRANSPOSE_CACHE.grad_b(row_ptr, col_idx, values.detach(), ctx.m, ctx.k, d_out)
        return None, None, d_values, None, None, d_b, None


class SddmmCsrFunction(torch.autograd.Function):
    """out[j] = <a[row(j), :], b[col(j), :]>, differentiable in a and b.  With g = d(out) as the
    values of A's pattern: d(a) = A(g) @ b and d(b) = A(g)^T @ a, both the SpMM kernels (the latter
    on the cached transpose)."""

    @staticmethod
    def forward(ctx, row_ptr, col_idx, a, b, static_csr=0):
        ctx.save_for_backward(row_ptr, col_idx, a, b)
        ctx.static_csr = static_csr
        return _C.sddmm_csr(row_ptr, col_idx, a, b, row_ptr.numel() - 1, b.shape[0],
                            static_csr=static_csr)

    @staticmethod
    def backward(ctx, d_out):
        row_ptr, col_idx, a, b = ctx.saved_tensors
        g = d_out.contiguous()
        m, k = row_ptr.numel() - 1, b.shape[0]
        d_a = d_b = None
        if ctx.needs_input_grad[2]:
            d_a = spmm_csr(row_ptr, col_idx, g, m, k, b.detach())
        if ctx.needs_input_grad[3]:
            d_b = TRANSPOSE_CACHE.grad_b(row_ptr, col_idx, g, m, k, a.detach())
        return None, None, d_a, d_b, None


class SpmmCsrHeadsFunction(torch.autograd.Function):
    """out [M, H, D] = per head h, A(values[:, h]) @ b[:, h, :], differentiable in values [nnz, H]
    and b [K, H, D]: d(values) is the multi-head SDDMM of d(out) and b, d(b) the multi-head SpMM
    on the cached transpose.  No sum crosses heads, so both have the bits of the per-head
    gradients."""

    @staticmethod
    def forward(ctx, row_ptr, col_idx, values, m, k, b):
        heads, d = b.shape[1], b.shape[2]
        b2 = _heads_2d(b, "b")
        out = _C.spmm_csr_heads(row_ptr, col_idx, values, m, k, b2)
        ctx.save_for_backward(row_ptr, col_idx, values, b2)
        ctx.m, ctx.k, ctx.heads, ctx.d = m, k, heads, d
        return out.view(m, heads, d)

    @staticmethod
    def backward(ctx, d_out):
        row_ptr, col_idx, values, b2 = ctx.saved_tensors
        g = d_out.contiguous().view(ctx.m, ctx.heads * ctx.d)
        d_values = d_b = None
        if ctx.needs_input_grad[2]:
            d_values = _C.sddmm_csr_heads(row_ptr, col_idx, g, b2, ctx.heads)
        if ctx.needs_input_grad[5]:
            d_b = TRANSPOSE_CACHE.grad_b_heads(row_ptr, col_idx, values.detach(), ctx.m, ctx.k, g)
            d_b = d_b.view(ctx.k, ctx.heads, ctx.d)
        return None, None, d_values, None, None, d_b


class SddmmCsrHeadsFunction(torch.autograd.Function):
    """out [nnz, H] = per head the SDDMM of a [M, H, D] and b [K, H, D], differentiable in a and b.
    With g = d(out) as the per-head values of A's pattern: d(a) = spmm_heads(g, b) and d(b) =
    spmm_heads on A^T with g[perm]."""

    @staticmethod
    def forward(ctx, row_ptr, col_idx, a, b):
        heads, d = b.shape[1], b.shape[2]
        a2, b2 = _heads_2d(a, "a"), _heads_2d(b, "b")
        ctx.save_for_backward(row_ptr, col_idx, a2, b2)
        ctx.heads, ctx.d = heads, d
        return _C.sddmm_csr_heads(row_ptr, col_idx, a2, b2, heads)

    @staticmethod
    def backward(ctx, d_out):
        row_ptr, col_idx, a2, b2 = ctx.saved_tensors
        g = d_out.contiguous()
        m, k = row_ptr.numel() - 1, b2.shape[0]
        d_a = d_b = None
        if ctx.needs_input_grad[2]:
            d_a = _C.spmm_csr_heads(row_ptr, col_idx, g, m, k, b2).view(m, ctx.heads, ctx.d)
        if ctx.needs_input_grad[3]:
            d_b = TRANSPOSE_CACHE.grad_b_heads(row_ptr, col_idx, g, m, k, a2)
            d_b = d_b.view(k, ctx.heads, ctx.d)
        return None, None, d_a, d_b


def _spmm_heads(row_ptr, col_idx, values, m, k, b, out, reduce):
    """`spmm` with b [K, H, D]: values [nnz, H] -> [M, H, D]."""
    if reduce != "sum":
        raise ValueError(f"spmm: a multi-head b [K, H, D] supports reduce='sum' only, got {reduce!r}")
    if values.dim() != 2 or values.shape[1] != b.shape[1]:
        raise RuntimeError("spmm: a multi-head b [K, H, D] needs a_csr_values [nnz, H], got "
                           f"{tuple(values.shape)} for b {tuple(b.shape)}")
    m, k = int(m), int(k)
    heads, d = b.shape[1], b.shape[2]
    if _recording("spmm", out, values, b):
        return SpmmCsrHeadsFunction.apply(row_ptr, col_idx, values, m, k, b)
    out2 = None
    if out is not None:
        if tuple(out.shape) != (m, heads, d) or not out.is_contiguous():
            raise RuntimeError(f"spmm: out must be a contiguous {(m, heads, d)} tensor, got "
                               f"{tuple(out.shape)}")
        out2 = out.view(m, heads * d)
    res = _C.spmm_csr_heads(row_ptr, col_idx, values, m, k, _heads_2d(b, "b"), out=out2)
    return out if out is not None else res.view(m, heads, d)


FP8_MAX = {torch.float8_e4m3fn: 448.0, torch.float8_e5m2: 57344.0}


def quantize_rows_fp8(b: torch.Tensor, dtype: torch.dtype = torch.float8_e4m3fn):
    """(b_q, b_scale) for `spmm_fp8`: every row of b (the last dimension of a [K, N] or [K, H, D]
    tensor) scaled into the range of `dtype` (torch.float8_e4m3fn, max 448, or torch.float8_e5m2,
    max 57344) and rounded to it.  scale = amax / max per row in float32, 1 for an all-zero row;
    b_q = (b / scale).to(dtype), so b is b_q * scale[:, None] up to the format's rounding.  One-off
    preprocessing of a feature table: a torch composition, no kernel of its own."""
    if dtype not in FP8_MAX:
        raise TypeError(f"quantize_rows_fp8: dtype should be float8_e4m3fn or float8_e5m2, got "
                        f"{dtype}")
    if b.dim() not in (2, 3):
        raise RuntimeError("quantize_rows_fp8: b should be [K, N] or [K, H, D], got shape "
                           f"{tuple(b.shape)}")
    bf = b.detach().to(torch.float32)
    amax = bf.flatten(1).abs().amax(dim=1) if bf.numel() else bf.new_zeros(bf.shape[0])
    scale = torch.where(amax > 0, amax / FP8_MAX[dtype], torch.ones_like(amax))
    b_q = (bf / scale.view(-1, *([1] * (bf.dim() - 1)))).to(dtype)
    return b_q, scale


class SpmmFp8Function(torch.autograd.Function):
    """out = spmm_fp8(values, b_q, b_scale), differentiable in values [nnz, H] alone:
    d(values)[j, h] = <d(out)[row(j), h, :], Bd[col[j], h, :]> * b_scale[col[j]], the multi-head
    SDDMM over Bd = b_q converted to the values' dtype, which only the backward materialises."""

    @staticmethod
    def forward(ctx, row_ptr, col_idx, values, m, k, b_q2, b_scale, heads):
        out = _C.spmm_csr_heads_fp8(row_ptr, col_idx, values, m, k, b_q2, b_scale)
        ctx.save_for_backward(row_ptr, col_idx, b_q2, b_scale)
        ctx.heads = heads
        return out

    @staticmethod
    def backward(ctx, d_out):
        row_ptr, col_idx, b_q2, b_scale = ctx.saved_tensors
        d_values = None
        if ctx.needs_input_grad[2]:
            g = d_out.contiguous()
            d_values = _C.sddmm_csr_heads(row_ptr, col_idx, g, b_q2.to(g.dtype), ctx.heads)
            if b_scale is not None:
                ci = col_idx.long()
                inside = (ci >= 0) & (ci < b_scale.numel())
                s = torch.where(inside, b_scale[ci.clamp(0, max(b_scale.numel() - 1, 0))],
                                torch.zeros((), dtype=b_scale.dtype, device=b_scale.device))
                d_values = (d_values.to(torch.float32) * s.unsqueeze(1)).to(g.dtype)
        return None, None, d_values, None, None, None, None, None


def spmm_fp8(row_ptr, col_idx, values, m, k, b_q, b_scale=None, *, out=None):
    """`spmm` over a feature table stored in FP8: b_q is torch.float8_e4m3fn or torch.float8_e5m2,
    [K, N] with values [nnz] (or [nnz, 1]) or [K, H, D] with values [nnz, H]; b_scale an optional
    float32 [K] scale per row of b_q (`quantize_rows_fp8` makes the pair).  values is float32,
    float16 or bfloat16 and so is the result, [M, N] or [M, H, D]:
        out[r, h, :] = sum_j (values[j, h] * b_scale[col[j]]) * b_q[col[j], h, :]
    in one launch for all heads (op "spmm_csr_heads_fp8"), accumulated in float32, with exactly the
    bits of `spmm` on the scaled values rounded to the dtype and on b_q.to(dtype); without b_scale,
    those of `spmm(values, b_q.to(dtype))`.  The gathered rows are one byte per element.

    Differentiable in values only (b_q and b_scale get no gradient): the gradient is
    sddmm(d(out), b_q.to(dtype)) * b_scale[col].  That backward dequantises the whole of b_q to the
    values' dtype, K * N elements each time it runs; an FP8 SDDMM does not exist yet.  `out=` is
    only accepted when no gradient is being recorded."""
    if not isinstance(b_q, torch.Tensor) or b_q.dtype not in FP8_MAX:
        raise TypeError("spmm_fp8: b_q should be float8_e4m3fn or float8_e5m2, got "
                        f"{getattr(b_q, 'dtype', type(b_q).__name__)}")
    m, k = int(m), int(k)
    if b_q.dim() == 3:
        heads, d = b_q.shape[1], b_q.shape[2]
        if values.dim() != 2 or values.shape[1] != heads:
            raise RuntimeError("spmm_fp8: a multi-head b_q [K, H, D] needs values [nnz, H], got "
                               f"{tuple(values.shape)} for b_q {tuple(b_q.shape)}")
        b2, vals, shape = _heads_2d(b_q, "b_q"), values, (m, heads, d)
    elif b_q.dim() == 2:
        if values.dim() == 2 and values.shape[1] != 1:
            raise RuntimeError("spmm_fp8: b_q [K, N] needs values [nnz] or [nnz, 1], got "
                               f"{tuple(values.shape)}")
        heads, b2, shape = 1, b_q, (m, b_q.shape[1])
        vals = values.reshape(-1, 1) if values.dim() == 1 else values
    else:
        raise RuntimeError(f"spmm_fp8: b_q should be [K, N] or [K, H, D], got {tuple(b_q.shape)}")
    if _recording("spmm_fp8", out, values):
        return SpmmFp8Function.apply(row_ptr, col_idx, vals, m, k, b2, b_scale, heads).view(shape)
    out2 = None
    if out is not None:
        if tuple(out.shape) != shape or (len(shape) == 3 and not out.is_contiguous()):
            raise RuntimeError(f"spmm_fp8: out must be a {shape} tensor"
                               f"{' (contiguous)' if len(shape) == 3 else ''}, got "
                               f"{tuple(out.shape)}")
        out2 = out.view(m, -1) if len(shape) == 3 else out
    res = _C.spmm_csr_heads_fp8(row_ptr, col_idx, vals, m, k, b2, b_scale, out=out2)
    return out if out is not None else res.view(shape)


class EdgeSoftmaxFunction(torch.autograd.Function):
    """y = edge_softmax(row_ptr, e) for e [nnz] or [nnz, H], differentiable in e.  The output is
    saved and the backward is one launch of op "edge_softmax_csr_grad" (for [nnz, H]:
    "edge_softmax_csr_heads_grad") on it (nothing is recomputed)."""

    @staticmethod
    def forward(ctx, row_ptr, col_idx, e):
        op = _C.edge_softmax_csr_heads if e.dim() == 2 else _C.edge_softmax_csr
        y = op(row_ptr, col_idx, e)
        ctx.save_for_backward(row_ptr, col_idx, y)
        return y

    @staticmethod
    def backward(ctx, d_y):
        row_ptr, col_idx, y = ctx.saved_tensors
        op = _C.edge_softmax_csr_heads_grad if y.dim() == 2 else _C.edge_softmax_csr_grad
        return None, None, op(row_ptr, col_idx, y, d_y.contiguous())


EdgeSoftmaxHeadsFunction = EdgeSoftmaxFunction  # one class serves both ranks


def _edge_softmax_heads_composed(a_csr_row_ptr, a_csr_col_idx, e):
    """The multi-head edge softmax as a per-head composition of the single-head op: one contiguous
    column per head through `edge_softmax`, the results stacked back (H launches and H column
    copies each way).  What the 2-D `edge_softmax` was before op "edge_softmax_csr_heads"; kept as
    the comparison object of the tests and of scripts/edge_softmax_heads_bench.py."""
    if e.shape[1] == 0:
        return torch.empty_like(e)
    return torch.stack([edge_softmax(a_csr_row_ptr, a_csr_col_idx, e[:, h].contiguous())
                        for h in range(e.shape[1])], dim=1)


def edge_softmax(a_csr_row_ptr, a_csr_col_idx, e, *, out=None):
    """The scores e [nnz] of a CSR's nonzeros normalised over each row:
    y[j] = exp(e[j] - max_row) / sum over j's row of exp(e - max_row) (DGL's edge_softmax, PyG's
    softmax(src, ptr=row_ptr)), the step between `sddmm` and `spmm` of dot-product graph
    attention.  One launch, deterministic, the same bits on CPU and GPU tensors; differentiable
    in e.  `a_csr_col_idx` is taken for its shape only.  `out=` only when no gradient is being
    recorded.

    Multi-head scores e [nnz, H] (the output of the 3-D `sddmm`) give y [nnz, H], each head
    normalised on its own, in one launch forward and one backward (op "edge_softmax_csr_heads");
    a non-contiguous e or upstream gradient is made contiguous first, `out=` (a contiguous
    [nnz, H] tensor) is written directly.  Every head has the bits of the 1-D call on its
    column."""
    if _recording("edge_softmax", out, e):
        return EdgeSoftmaxFunction.apply(a_csr_row_ptr, a_csr_col_idx, e)
    op = _C.edge_softmax_csr_heads if e.dim() == 2 else _C.edge_softmax_csr
    return op(a_csr_row_ptr, a_csr_col_idx, e, out=out)


class GraphAttentionFunction(torch.autograd.Function):
    """(out [M, H, D], attn [nnz, H]) = graph attention of q [M, H, D], k and v [K, H, D] through
    op "graph_attention_csr_heads", differentiable in q, k and v.  The weights are saved
    and the backward consists of the composed layer's own ops, so every gradient has the bits of
    the autograd of spmm(edge_softmax(sddmm(q, k)), v)."""

    @staticmethod
    def forward(ctx, row_ptr, col_idx, q, k, v):
        heads, d = k.shape[1], k.shape[2]
        q2, k2, v2 = _heads_2d(q, "q"), _heads_2d(k, "k"), _heads_2d(v, "v")
        out, attn = _C.graph_attention_csr_heads(row_ptr, col_idx, q2, k2, v2, heads)
        ctx.save_for_backward(row_ptr, col_idx, q2, k2, v2, attn)
        ctx.heads, ctx.d = heads, d
        # an output that did not enter the loss hands in None, not a tensor of zeros: no [nnz, H]
        # allocation and no add (which would also turn a -0 of d_attn into +0) for unused weights
        ctx.set_materialize_grads(False)
        return out.view(q2.shape[0], heads, d), attn

    @staticmethod
    def backward(ctx, d_out, d_attn_up):
        row_ptr, col_idx, q2, k2, v2, attn = ctx.saved_tensors
        heads, d = ctx.heads, ctx.d
        m, k = q2.shape[0], k2.shape[0]
        d_q = d_k = d_v = None
        g = None if d_out is None else d_out.contiguous().view(m, heads * d)
        if g is None and d_attn_up is None:
            return None, None, None, None, None
        if ctx.needs_input_grad[4] and g is not None:
            d_v = TRANSPOSE_CACHE.grad_b_heads(row_ptr, col_idx, attn, m, k, g).view(k, heads, d)
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            if g is None:  # only the returned weights entered the loss
                d_attn = d_attn_up
            else:
                d_attn = _C.sddmm_csr_heads(row_ptr, col_idx, g, v2, heads)
                if d_attn_up is not None:  # the returned weights entered the loss as well
                    d_attn = d_attn + d_attn_up
            d_e = _C.edge_softmax_csr_heads_grad(row_ptr, col_idx, attn, d_attn.contiguous())
            if ctx.needs_input_grad[2]:
                d_q = _C.spmm_csr_heads(row_ptr, col_idx, d_e, m, k, k2).view(m, heads, d)
            if ctx.needs_input_grad[3]:
                d_k = TRANSPOSE_CACHE.grad_b_heads(row_ptr, col_idx, d_e, m, k, q2)
                d_k = d_k.view(k, heads, d)
        return None, None, d_q, d_k, d_v


def graph_attention(a_csr_row_ptr, a_csr_col_idx, q, k, v, *, return_attention=False):
    """Dot-product graph attention over a CSR:
        attn[j, h] = softmax over j's row of <q[row(j), h, :], k[col[j], h, :]>
        out[r, h, :] = sum over r's nonzeros j of attn[j, h] * v[col[j], h, :]
    for q [M, H, D], k and v [K, H, D] (DGL's / PyG's fused dot-product attention).  Returns
    out [M, H, D], or (out, attn [nnz, H]) with return_attention=True.  The 2-D forms q [M, D],
    k and v [K, D] mean H = 1 and return out [M, D].  There is no scale factor: scale q.
    On the GPU a row of at most the SpMM's hub threshold (512 nonzeros at D <= 128) goes through
    scores, softmax and aggregation inside one kernel; longer rows take the planner's chunks and
    three small follow-up launches.

    out and attn have exactly the bits of `spmm(rp, ci, edge_softmax(rp, ci, sddmm(rp, ci, q, k)),
    M, K, v)`, on CPU and GPU tensors, and so have the gradients in q, k and v: the backward is
    that composition's.  Non-contiguous inputs are made contiguous first."""
    if q.dim() != k.dim() or q.dim() != v.dim() or q.dim() not in (2, 3):
        raise RuntimeError("graph_attention: q [M, H, D], k and v [K, H, D] (or q [M, D], k and v "
                           f"[K, D]) are expected, got {tuple(q.shape)}, {tuple(k.shape)}, "
                           f"{tuple(v.shape)}")
    flat = q.dim() == 2
    if flat:
        q, k, v = q.unsqueeze(1), k.unsqueeze(1), v.unsqueeze(1)
    if q.shape[1:] != k.shape[1:] or v.shape != k.shape:
        raise RuntimeError("graph_attention: q [M, H, D] needs k and v [K, H, D] with the same "
                           f"heads and D, got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    if q.dtype != k.dtype or v.dtype != k.dtype:
        raise TypeError("graph_attention: q, k and v should have one dtype, got "
                        f"{q.dtype}, {k.dtype}, {v.dtype}")
    if q.device != k.device or v.device != k.device:
        raise RuntimeError("graph_attention: expected all tensors on the same device, got "
                           f"{q.device}, {k.device}, {v.device}")
    heads, d = k.shape[1], k.shape[2]
    if _recording("graph_attention", None, q, k, v):
        out, attn = GraphAttentionFunction.apply(a_csr_row_ptr, a_csr_col_idx, q, k, v)
    else:
        out, attn = _C.graph_attention_csr_heads(a_csr_row_ptr, a_csr_col_idx, _heads_2d(q, "q"),
                                                 _heads_2d(k, "k"), _heads_2d(v, "v"), heads)
        out = out.view(q.shape[0], heads, d)
    if flat:
        out = out.view(q.shape[0], d)
    return (out, attn) if return_attention else out


class GatSoftmaxFunction(torch.autograd.Function):
    """attn [nnz, H] = gat_softmax of s_row [M, H] and s_col [K, H] through op
    "gat_softmax_csr_heads", differentiable in both.  The weights are saved; the backward is one
    launch of op "gat_softmax_csr_heads_grad" (ds per nonzero and d(s_row), its row sums) and, only
    when s_col needs a gradient, the multi-head SpMM of ds on the cached transpose with b = ones
    (deterministic, no atomics, the same bits on CPU and GPU)."""

    @staticmethod
    def forward(ctx, row_ptr, col_idx, s_row, s_col, negative_slope):
        s_row, s_col = s_row.contiguous(), s_col.contiguous()
        attn = _C.gat_softmax_csr_heads(row_ptr, col_idx, s_row, s_col, negative_slope)
        ctx.save_for_backward(row_ptr, col_idx, s_row, s_col, attn)
        ctx.negative_slope = negative_slope
        return attn

    @staticmethod
    def backward(ctx, d_attn):
        row_ptr, col_idx, s_row, s_col, attn = ctx.saved_tensors
        ds, d_row = _C.gat_softmax_csr_heads_grad(row_ptr, col_idx, s_row, s_col, attn,
                                                  d_attn.contiguous(), ctx.negative_slope)
        d_col = None
        if ctx.needs_input_grad[3]:
            d_col = TRANSPOSE_CACHE.grad_b_heads(row_ptr, col_idx, ds, s_row.shape[0],
                                                 s_col.shape[0], torch.ones_like(s_row))
        return None, None, d_row if ctx.needs_input_grad[2] else None, d_col, None


def gat_softmax(a_csr_row_ptr, a_csr_col_idx, s_row, s_col, negative_slope=0.2, *, out=None):
    """The attention weights of a GAT layer over a CSR, in one launch:
        attn[j, h] = softmax over j's row of LeakyReLU(s_row[row(j), h] + s_col[col[j], h])
    for s_row [M, H] (a_l . W h_i per destination) and s_col [K, H] (a_r . W h_j per source);
    1-D s_row [M] and s_col [K] mean H = 1 and return attn [nnz].  The scores are rounded to the
    dtype before the softmax and never written: attn has exactly the bits of
    `edge_softmax(rp, ci, e)` on them, on CPU and GPU tensors.  negative_slope must
    be finite and > 0 (0 would turn a -inf mask into NaN).  Differentiable in s_row and s_col; the
    gradient in s_col is built only when it is needed.  Non-contiguous inputs are made contiguous
    first; `out=` (a contiguous [nnz, H] tensor, [nnz] for 1-D inputs) only when no gradient is
    being recorded."""
    if s_row.dim() != s_col.dim() or s_row.dim() not in (1, 2):
        raise RuntimeError("gat_softmax: s_row [M, H] and s_col [K, H] (or s_row [M] and s_col "
                           f"[K]) are expected, got {tuple(s_row.shape)} and {tuple(s_col.shape)}")
    flat = s_row.dim() == 1
    if flat:
        s_row, s_col = s_row.unsqueeze(1), s_col.unsqueeze(1)
    negative_slope = float(negative_slope)
    if _recording("gat_softmax", out, s_row, s_col):
        attn = GatSoftmaxFunction.apply(a_csr_row_ptr, a_csr_col_idx, s_row, s_col, negative_slope)
        return attn.squeeze(1) if flat else attn
    if flat and out is not None:
        if out.dim() != 1 or not out.is_contiguous():
            raise RuntimeError("gat_softmax: out must be a contiguous [nnz] tensor for 1-D "
                               f"inputs, got {tuple(out.shape)}")
        _C.gat_softmax_csr_heads(a_csr_row_ptr, a_csr_col_idx, s_row, s_col, negative_slope,
                                 out=out.unsqueeze(1))
        return out
    attn = _C.gat_softmax_csr_heads(a_csr_row_ptr, a_csr_col_idx, s_row, s_col, negative_slope,
                                    out=out)
    return attn.squeeze(1) if flat else attn


def gat_attention(a_csr_row_ptr, a_csr_col_idx, s_row, s_col, v, negative_slope=0.2, *,
                  return_attention=False):
    """A GAT layer's aggregation: out = spmm(rp, ci, gat_softmax(rp, ci, s_row, s_col,
    negative_slope), M, K, v) for s_row [M, H], s_col [K, H] and v [K, H, D] (out [M, H, D]), or
    1-D s_row, s_col and v [K, D] (out [M, D]).  Plain composition of the two ops: their bits and
    their gradients.  Returns out, or (out, attn) with return_attention=True."""
    attn = gat_softmax(a_csr_row_ptr, a_csr_col_idx, s_row, s_col, negative_slope)
    out = spmm(a_csr_row_ptr, a_csr_col_idx, attn, s_row.shape[0], s_col.shape[0], v)
    return (out, attn) if return_attention else out


class Gatv2ScoresFunction(torch.autograd.Function):
    """e [nnz, H] = the GATv2 scores of x_row [M, H*D], x_col [K, H*D] and att [H*D] through op
    "gatv2_scores_csr_heads", differentiable in all three.  The inputs are saved (no per-nonzero
    tensor is); the backward is one launch of op "gatv2_scores_csr_heads_grad" on A (d(x_row), and
    p only when att needs a gradient: d(att) is its column sum in relu_bias_grad's fixed order) and,
    only when x_col needs a gradient, one on the cached transpose with x_row and x_col exchanged
    and the upstream gradient gathered by the transpose's perm (deterministic, no atomics, the
    same bits on CPU and GPU)."""

    @staticmethod
    def forward(ctx, row_ptr, col_idx, x_row, x_col, att, heads, negative_slope):
        x_row, x_col, att = x_row.contiguous(), x_col.contiguous(), att.contiguous()
        e = _C.gatv2_scores_csr_heads(row_ptr, col_idx, x_row, x_col, att, heads, negative_slope)
        ctx.save_for_backward(row_ptr, col_idx, x_row, x_col, att)
        ctx.heads, ctx.negative_slope = heads, negative_slope
        return e

    @staticmethod
    def backward(ctx, d_e):
        row_ptr, col_idx, x_row, x_col, att = ctx.saved_tensors
        d_e = d_e.contiguous()
        d_row = d_col = d_att = None
        need_row, need_col, need_att = ctx.needs_input_grad[2:5]
        if need_row or need_att:
            d_row, p = _C.gatv2_scores_csr_heads_grad(row_ptr, col_idx, x_row, x_col, att, d_e,
                                                      ctx.heads, ctx.negative_slope,
                                                      with_att=need_att)
            if need_att:
                d_att = ops.relu_bias_grad(None, p, relu=False, bias_grad=True)[1]
        if need_col:
            rp_t, ci_t, _, de_t = TRANSPOSE_CACHE.transposed_values(row_ptr, col_idx, d_e,
                                                                    x_col.shape[0], "gather")
            d_col, _ = _C.gatv2_scores_csr_heads_grad(rp_t, ci_t, x_col, x_row, att, de_t,
                                                      ctx.heads, ctx.negative_slope,
                                                      with_att=False)
        return None, None, d_row if need_row else None, d_col, d_att, None, None


def _gatv2_forms(op, x_row, x_col, att):
    """(x_row [M, H*D], x_col [K, H*D], att [H*D], H, D, flat) of the public GATv2 entries'
    3-D form (x [rows, H, D], att [H, D]) or 2-D form (x [rows, D], att [D]: H = 1, flat)."""
    flat = x_row.dim() == 2
    if x_row.dim() != x_col.dim() or x_row.dim() not in (2, 3) or att.dim() != x_row.dim() - 1:
        raise RuntimeError(f"{op}: x_row [M, H, D], x_col [K, H, D] and att [H, D] (or x_row "
                           f"[M, D], x_col [K, D] and att [D]) are expected, got "
                           f"{tuple(x_row.shape)}, {tuple(x_col.shape)} and {tuple(att.shape)}")
    if x_row.shape[1:] != x_col.shape[1:] or att.shape != x_col.shape[1:]:
        raise RuntimeError(f"{op}: x_row, x_col and att should agree in heads and D, got "
                           f"{tuple(x_row.shape)}, {tuple(x_col.shape)} and {tuple(att.shape)}")
    if x_row.dtype != x_col.dtype or att.dtype != x_col.dtype:
        raise TypeError(f"{op}: x_row, x_col and att should have one dtype, got "
                        f"{x_row.dtype}, {x_col.dtype}, {att.dtype}")
    if x_row.device != x_col.device or att.device != x_col.device:
        raise RuntimeError(f"{op}: expected all tensors on the same device, got "
                           f"{x_row.device}, {x_col.device}, {att.device}")
    heads = 1 if flat else x_col.shape[1]
    d = x_col.shape[-1]
    return (x_row.reshape(x_row.shape[0], heads * d), x_col.reshape(x_col.shape[0], heads * d),
            att.reshape(heads * d), heads, d, flat)


def gatv2_scores(a_csr_row_ptr, a_csr_col_idx, x_row, x_col, att, negative_slope=0.2, *, out=None):
    """The attention scores of a GATv2 layer over a CSR, in one launch:
        e[j, h] = sum over d of att[h, d] * LeakyReLU(x_row[row(j), h, d] + x_col[col[j], h, d])
    for x_row [M, H, D] (W_l h_i per destination), x_col [K, H, D] (W_r h_j per source) and
    att [H, D]; 2-D x_row [M, D], x_col [K, D] and 1-D att [D] mean H = 1 and return e [nnz].  The
    activated sum is rounded to the dtype and never written: e has exactly the bits of
    `sddmm(rp, arange(nnz), att repeated, U)` on it, on CPU and GPU tensors.
    negative_slope must be finite and > 0.  Differentiable in x_row, x_col and att; the gradient
    in x_col (one launch on the cached transpose) is built only when it is needed.  `out=` (a
    contiguous [nnz, H] tensor, [nnz] for the 2-D form) only when no gradient is being recorded.
    A column index outside [0, K) reads x_col as +0."""
    xr, xc, w, heads, _, flat = _gatv2_forms("gatv2_scores", x_row, x_col, att)
    negative_slope = float(negative_slope)
    if _recording("gatv2_scores", out, x_row, x_col, att):
        e = Gatv2ScoresFunction.apply(a_csr_row_ptr, a_csr_col_idx, xr, xc, w, heads,
                                      negative_slope)
        return e.squeeze(1) if flat else e
    if flat and out is not None:
        if out.dim() != 1 or not out.is_contiguous():
            raise RuntimeError("gatv2_scores: out must be a contiguous [nnz] tensor for the 2-D "
                               f"form, got {tuple(out.shape)}")
        _C.gatv2_scores_csr_heads(a_csr_row_ptr, a_csr_col_idx, xr, xc, w, heads, negative_slope,
                                  out=out.unsqueeze(1))
        return out
    e = _C.gatv2_scores_csr_heads(a_csr_row_ptr, a_csr_col_idx, xr, xc, w, heads, negative_slope,
                                  out=out)
    return e.squeeze(1) if flat else e


def gatv2_softmax(a_csr_row_ptr, a_csr_col_idx, x_row, x_col, att, negative_slope=0.2):
    """The attention weights of a GATv2 layer: edge_softmax(rp, ci, gatv2_scores(...)), [nnz, H]
    ([nnz] for the 2-D form).  Plain composition: the bits and gradients of the two ops."""
    return edge_softmax(a_csr_row_ptr, a_csr_col_idx,
                        gatv2_scores(a_csr_row_ptr, a_csr_col_idx, x_row, x_col, att,
                                     negative_slope))


def gatv2_attention(a_csr_row_ptr, a_csr_col_idx, x_row, x_col, att, negative_slope=0.2, *,
                    v=None, return_attention=False):
    """A GATv2 layer's aggregation: out = spmm(rp, ci, gatv2_softmax(rp, ci, x_row, x_col, att,
    negative_slope), M, K, v) with v = x_col unless given ([K, H, D'] or, for the 2-D form,
    [K, D']).  Plain composition of the three ops: their bits and their gradients.  Returns out,
    or (out, attn) with return_attention=True."""
    attn = gatv2_softmax(a_csr_row_ptr, a_csr_col_idx, x_row, x_col, att, negative_slope)
    out = spmm(a_csr_row_ptr, a_csr_col_idx, attn, x_row.shape[0], x_col.shape[0],
               x_col if v is None else v)
    return (out, attn) if return_attention else out


class SpmmCsrReduceFunction(torch.autograd.Function):
    """(out, arg) = spmm_csr_reduce(..., reduce) for reduce in {"mean", "max", "min"},
    differentiable in `a_csr_values` and `b`; `arg` is not differentiable.

    max / min: the forward's arg is saved; d(b) is the masked SpMM on the cached A^T
    (TRANSPOSE_CACHE, op "spmm_csr_reduce_grad_b": deterministic, no atomics) and d(values) the
    masked SDDMM (op "spmm_csr_reduce_grad_values").  mean: the upstream gradient is divided by
    the row degrees (the forward's row scale), then the sum op's gradients run on it."""

    @staticmethod
    def forward(ctx, row_ptr, col_idx, values, m, k, b, reduce):
        out, arg = _C.spmm_csr_reduce(row_ptr, col_idx, values, m, k, b, reduce)
        ctx.save_for_backward(row_ptr, col_idx, values, b, arg)
        ctx.m, ctx.k, ctx.reduce = m, k, reduce
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, d_out, _d_arg):
        row_ptr, col_idx, values, b, arg = ctx.saved_tensors
        d_out = d_out.contiguous()
        d_values = d_b = None
        if ctx.reduce == "mean":
            g = _C.row_scale_by_degree(row_ptr, d_out)
            if ctx.needs_input_grad[2]:
                d_values = sddmm(row_ptr, col_idx, g, b)
            if ctx.needs_input_grad[5]:
                d_b = TRANSPOSE_CACHE.grad_b(row_ptr, col_idx, values.detach(), ctx.m, ctx.k, g)
            return None, None, d_values, None, None, d_b, None
        if ctx.needs_input_grad[2]:
            d_values = _C.spmm_csr_reduce_grad_values(row_ptr, col_idx, arg, d_out, b, ctx.m, ctx.k)
        if ctx.needs_input_grad[5]:
            rp_t, ci_t, perm = TRANSPOSE_CACHE.get(row_ptr, col_idx, ctx.k)
            d_b = _C.spmm_csr_reduce_grad_b(rp_t, ci_t, perm, values.detach(), arg, d_out, ctx.m,
                                            ctx.k)
        return None, None, d_values, None, None, d_b, None


def spmm_reduce(a_csr_row_ptr, a_csr_col_idx, a_csr_values, a_num_rows, a_num_cols, b,
                reduce="sum", *, out=None):
    """(out, arg) of `spmm(..., reduce=reduce)`: arg[r, c] is the global nonzero index that won
    column c of row r for "max" / "min" (-1 for an empty row), an empty [0, N] tensor for "sum" /
    "mean".  With autograd, as `spmm`; `out=` only when no gradient is being recorded."""
    _C.reduce_code(reduce)  # ValueError for an unknown name, before anything runs
    if _recording("spmm_reduce", out, a_csr_values, b):
        if reduce == "sum":
            res = SpmmCsrFunction.apply(a_csr_row_ptr, a_csr_col_idx, a_csr_values,
                                        int(a_num_rows), int(a_num_cols), b, 0)
            return res, torch.empty((0, res.shape[1]), dtype=a_csr_row_ptr.dtype,
                                    device=res.device)
        return SpmmCsrReduceFunction.apply(a_csr_row_ptr, a_csr_col_idx, a_csr_values,
                                           int(a_num_rows), int(a_num_cols), b, reduce)
    return _C.spmm_csr_reduce(a_csr_row_ptr, a_csr_col_idx, a_csr_values, a_num_rows, a_num_cols,
                              b, reduce, out=out)


def spmm(a_csr_row_ptr, a_csr_col_idx, a_csr_values, a_num_rows, a_num_cols, b, *, out=None,
         static_csr=0, reduce="sum"):
    """`oneflow.spmm` with autograd: differentiable in `a_csr_values` and `b`.
    `out=` (a preallocated result) is only accepted when no gradient is being recorded.
    `static_csr` (op attr; True = 1): the CSR is not rewritten while calls carry this value, so
    the forward plans its work list once (_C.spmm_csr).
    `reduce`: "sum" (the default: the op as it always was), "mean", "max" or "min" (PyG's
    reduce=, DGL's u_mul_e_max / _min / copy-mean); `spmm_reduce` also returns max / min's arg.
    static_csr applies to "sum" only.

    Multi-head: b [K, H, D] with a_csr_values [nnz, H] gives out [M, H, D], out[r, h, :] =
    sum_j values[j, h] * b[col[j], h, :], in one launch (op "spmm_csr_heads"; reduce must be
    "sum", static_csr is accepted and has no effect), every head with the bits of the 2-D call on
    its slice."""
    if isinstance(b, torch.Tensor) and b.dim() == 3:
        return _spmm_heads(a_csr_row_ptr, a_csr_col_idx, a_csr_values, a_num_rows, a_num_cols, b,
                           out, reduce)
    if reduce != "sum":
        return spmm_reduce(a_csr_row_ptr, a_csr_col_idx, a_csr_values, a_num_rows, a_num_cols, b,
                           reduce, out=out)[0]
    if _recording("spmm", out, a_csr_values, b):
        return SpmmCsrFunction.apply(a_csr_row_ptr, a_csr_col_idx, a_csr_values, int(a_num_rows),
                                     int(a_num_cols), b, int(static_csr))
    return spmm_csr(a_csr_row_ptr, a_csr_col_idx, a_csr_values, a_num_rows, a_num_cols, b, out=out,
                    static_csr=int(static_csr))


class FusedSpmmCsrFunction(torch.autograd.Function):
    """relu?(A @ b + bias?).  Backward as the unfused graph's: relu_grad from the output
    (dy where y > 0, oneflow/core/autograd/gradient_funcs/activation.cpp:195-205), bias_add
    grad = column sum of the masked gradient (gradient_funcs/bias_add.cpp:62), then the
    spmm_csr gradients."""

    @staticmethod
    def forward(ctx, row_ptr, col_idx, values, m, k, b, bias, relu, static_csr=0):
        out = _C.fused_spmm_csr(row_ptr, col_idx, values, m, k, b, bias, relu=relu,
                                static_csr=static_csr)
        ctx.save_for_backward(row_ptr, col_idx, values, b, out if relu else None)
        ctx.m, ctx.k, ctx.relu, ctx.has_bias = m, k, relu, bias is not None
        ctx.static_csr = static_csr
        return out

    @staticmethod
    def backward(ctx, d_out):
        row_ptr, col_idx, values, b, out = ctx.saved_tensors
        # relu_grad and the bias column sum in one HIP pass (ofx_relu_bias_grad)
        g, d_bias = ops.relu_bias_grad(out, d_out.contiguous(), relu=ctx.relu,
                                       bias_grad=ctx.has_bias and ctx.needs_input_grad[6])
        d_values = d_b = None
        if ctx.needs_input_grad[2]:
            d_values = sddmm(row_ptr, col_idx, g, b, ctx.static_csr)
        if ctx.needs_input_grad[5]:
            d_b = TRANSPOSE_CACHE.grad_b(row_ptr, col_idx, values.detach(), ctx.m, ctx.k, g)
        return None, None, d_values, None, None, d_b, d_bias, None, None


def fused_spmm(a_csr_row_ptr, a_csr_col_idx, a_csr_values, a_num_rows, a_num_cols, b, bias=None,
               *, relu=False, out=None, static_csr=0):
    """A GCN layer's aggregation + bias + activation: relu?(A @ b + bias?) with autograd.
    `static_csr` as for `spmm`: the forward plans an unchanged CSR once."""
    if _recording("fused_spmm", out, a_csr_values, b, bias):
        return FusedSpmmCsrFunction.apply(a_csr_row_ptr, a_csr_col_idx, a_csr_values,
                                          int(a_num_rows), int(a_num_cols), b, bias, bool(relu),
                                          int(static_csr))
    return _C.fused_spmm_csr(a_csr_row_ptr, a_csr_col_idx, a_csr_values, a_num_rows, a_num_cols, b,
                             bias, relu=relu, out=out, static_csr=int(static_csr))


__all__ = ["csr_transpose", "gather_values", "sddmm", "SpmmCsrFunction", "spmm", "TRANSPOSE_CACHE", "ops",
           "FusedSpmmCsrFunction", "fused_spmm", "SpmmCsrReduceFunction", "spmm_reduce",
           "SddmmCsrFunction", "EdgeSoftmaxFunction", "edge_softmax", "SpmmCsrHeadsFunction",
           "SddmmCsrHeadsFunction", "EdgeSoftmaxHeadsFunction", "GatSoftmaxFunction", "gat_softmax",
           "gat_attention", "Gatv2ScoresFunction", "gatv2_scores", "gatv2_softmax",
           "gatv2_attention"]

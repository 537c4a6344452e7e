"""Helpers of the edge-softmax tests (test_edge_softmax_cpu.py, test_edge_softmax_gpu.py): the
numpy restatement of the contract in include/ofx_spmm.h (exp_acc, the leaf / tree sum, forward and
backward), and callers of the C-ABI entries on host or device memory with row ranges, options and
an unaligned base pointer."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from oneflow_spmm._C import current_stream_handle, dtype_code
from oneflow_spmm._lib import LIB, check
from reduce_helpers import acc, sentinel, store

LEAF = 8          # positions per leaf of the sum's order
G = 512           # the widest in-register capacity of the HIP kernels (a wave, one leaf per lane)
T = 512           # the long-row tile of the HIP kernels, in elements


# ---- the contract in numpy ------------------------------------------------------------------------
def exp_acc(t: np.ndarray) -> np.ndarray:
    """exp(t) for t <= 0 as csrc/edge_softmax.h computes it: every operation rounded to t's dtype
    (float32 or float64), no FMA; below the cut-off +0, NaN -> NaN."""
    t = np.asarray(t)
    f = t.dtype.type
    assert f in (np.float32, np.float64)
    nan = np.isnan(t)
    cut = f(-87.0) if f is np.float32 else f(-708.0)
    with np.errstate(invalid="ignore"):
        low = t < cut
    x = np.where(nan | low, f(0), t).astype(f)
    if f is np.float32:
        k = np.rint(x * f(1.44269504088896341))
        r = x - k * f(0.693359375)
        r = r - k * f(-2.12194440e-4)
        p = np.full_like(x, f(1.9875691500e-4))
        for c in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1,
                  5.0000001201e-1):
            p = p * r + f(c)
        z = r * r
        p = p * z
        p = p + r
        p = p + f(1.0)
        scale = ((k.astype(np.int32) + 127).astype(np.uint32) << np.uint32(23)).view(np.float32)
    else:
        k = np.rint(x * f(1.4426950408889634073599))
        r = x - k * f(6.93145751953125e-1)
        r = r - k * f(1.42860682030941723212e-6)
        z = r * r
        pp = np.full_like(x, f(1.26177193074810590878e-4))
        pp = pp * z + f(3.02994407707441961300e-2)
        pp = pp * z + f(9.99999999999999999910e-1)
        pp = pp * r
        qq = np.full_like(x, f(3.00198505138664455042e-6))
        qq = qq * z + f(2.52448340349684104192e-3)
        qq = qq * z + f(2.27265548208155028766e-1)
        qq = qq * z + f(2.00000000000000000009e0)
        p = pp / (qq - pp)
        p = p * f(2.0)
        p = p + f(1.0)
        scale = ((k.astype(np.int64) + 1023).astype(np.uint64) << np.uint64(52)).view(np.float64)
    out = (p * scale).astype(f)
    out = np.where(low, f(0), out)
    return np.where(nan, f(np.nan), out).astype(f)


def tree_sum(x: np.ndarray):
    """The contract's sum of one row: leaves of 8 positions summed sequentially from +0 (absent
    positions add nothing), zero-padded to a power of two, added pairwise level by level."""
    f = x.dtype.type
    leaves = (len(x) + LEAF - 1) // LEAF
    padded = 1
    while padded < leaves:
        padded *= 2
    buf = np.zeros(padded * LEAF, dtype=x.dtype)
    buf[:len(x)] = x
    buf = buf.reshape(padded, LEAF)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.zeros(padded, dtype=x.dtype)
        for c in range(LEAF):
            s = s + buf[:, c]
        while len(s) > 1:
            s = s[0::2] + s[1::2]
    return f(s[0])


def ref_forward(rp, e: torch.Tensor, row_begin=0, row_end=None):
    """y of rows [row_begin, row_end) in the oracle's representation (all nnz entries; those
    outside the range are zero and not to be compared)."""
    rpn = np.asarray(rp.cpu().numpy(), dtype=np.int64)
    row_end = len(rpn) - 1 if row_end is None else row_end
    ea = acc(e)
    y = np.zeros_like(ea)
    for r in range(row_begin, row_end):
        j0, j1 = rpn[r], rpn[r + 1]
        if j1 == j0:
            continue
        row = ea[j0:j1]
        m = row.dtype.type(np.nan) if np.isnan(row).any() else row.max()
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            x = exp_acc((row - m).astype(row.dtype))
            y[j0:j1] = x / tree_sum(x)
    return store(y, e.dtype)


def ref_backward(rp, y: torch.Tensor, g: torch.Tensor, row_begin=0, row_end=None):
    rpn = np.asarray(rp.cpu().numpy(), dtype=np.int64)
    row_end = len(rpn) - 1 if row_end is None else row_end
    ya, ga = acc(y), acc(g)
    de = np.zeros_like(ya)
    for r in range(row_begin, row_end):
        j0, j1 = rpn[r], rpn[r + 1]
        if j1 == j0:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            d = tree_sum((ya[j0:j1] * ga[j0:j1]).astype(ya.dtype))
            de[j0:j1] = ya[j0:j1] * (ga[j0:j1] - d).astype(ya.dtype)
    return store(de, y.dtype)


# ---- C-ABI callers --------------------------------------------------------------------------------
def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def shifted(t: torch.Tensor, shift: int) -> torch.Tensor:
    """A copy of the 1-D tensor t that starts `shift` elements into its buffer (a base pointer that
    is not aligned to a 16-byte load)."""
    if shift == 0:
        return t.contiguous()
    buf = torch.empty(t.numel() + shift, dtype=t.dtype, device=t.device)
    buf[shift:].copy_(t)
    return buf[shift:]


def _out(nnz, dtype, dev, shift):
    buf = sentinel((nnz + shift,), dtype, dev)
    return buf[shift:]


def _workspace(it, vt, m, nnz, o, dev):
    size = ctypes.c_size_t(0)
    check(LIB.ofx_edge_softmax_csr_workspace_size(it, vt, m, nnz, o, ctypes.byref(size)),
          "edge_softmax_workspace_size")
    return torch.empty(max(size.value, 1), dtype=torch.uint8, device=dev), size.value


def run_forward(rp, e, m, *, row_begin=0, row_end=None, opts=None, shift=0):
    """ofx_edge_softmax_csr(_cpu) on the tensors' device: all nnz entries of y, those outside the
    rows [row_begin, row_end) still holding sentinel()'s bits.  e and y start `shift` elements
    into their buffers."""
    row_end = m if row_end is None else row_end
    dev, nnz = e.device, e.numel()
    ee, y = shifted(e, shift), _out(nnz, e.dtype, dev, shift)
    it, vt = dtype_code(rp.dtype), dtype_code(e.dtype)
    o = ctypes.byref(opts) if opts is not None else None
    if dev.type == "cpu":
        check(LIB.ofx_edge_softmax_csr_cpu(0, it, vt, m, nnz, _ptr(rp), _ptr(ee), _ptr(y),
                                           row_begin, row_end, o), "edge_softmax_cpu")
    else:
        ws, size = _workspace(it, vt, m, nnz, o, dev)
        check(LIB.ofx_edge_softmax_csr(current_stream_handle(e), it, vt, m, nnz, _ptr(rp),
                                       _ptr(ee), _ptr(y), row_begin, row_end, ws.data_ptr(), size,
                                       o), "edge_softmax")
    return y


def run_backward(rp, y, g, m, *, row_begin=0, row_end=None, opts=None, shift=0):
    """ofx_edge_softmax_csr_grad(_cpu): all nnz entries of de, as run_forward."""
    row_end = m if row_end is None else row_end
    dev, nnz = y.device, y.numel()
    yy, gg, de = shifted(y, shift), shifted(g, shift), _out(nnz, y.dtype, dev, shift)
    it, vt = dtype_code(rp.dtype), dtype_code(y.dtype)
    o = ctypes.byref(opts) if opts is not None else None
    if dev.type == "cpu":
        check(LIB.ofx_edge_softmax_csr_grad_cpu(0, it, vt, m, nnz, _ptr(rp), _ptr(yy), _ptr(gg),
                                                _ptr(de), row_begin, row_end, o),
              "edge_softmax_grad_cpu")
    else:
        ws, size = _workspace(it, vt, m, nnz, o, dev)
        check(LIB.ofx_edge_softmax_csr_grad(current_stream_handle(y), it, vt, m, nnz, _ptr(rp),
                                            _ptr(yy), _ptr(gg), _ptr(de), row_begin, row_end,
                                            ws.data_ptr(), size, o), "edge_softmax_grad")
    return de


# ---- references for the accuracy checks -----------------------------------------------------------
def dense_softmax(rp, e64: torch.Tensor) -> torch.Tensor:
    """torch.softmax over each row's scores (float64), row by row."""
    rpn = rp.cpu().numpy()
    out = torch.empty_like(e64)
    for r in range(len(rpn) - 1):
        j0, j1 = int(rpn[r]), int(rpn[r + 1])
        if j1 > j0:
            out[j0:j1] = torch.softmax(e64[j0:j1], dim=0)
    return out


def dense_attention(rp, ci, q, k, v):
    """The composed layer spmm(edge_softmax(sddmm(q, k))) @ v on dense tensors: scores masked to
    the CSR's pattern, softmax over each row (an empty row gives a zero row)."""
    m = rp.numel() - 1
    rows = torch.repeat_interleave(torch.arange(m), torch.diff(rp.cpu().long())).to(q.device)
    cols = ci.long().to(q.device)
    mask = torch.zeros((m, k.shape[0]), dtype=torch.bool, device=q.device)
    mask[rows, cols] = True
    s = (q @ k.t()).masked_fill(~mask, float("-inf"))
    p = torch.softmax(s, dim=1)
    p = torch.where(mask, p, torch.zeros_like(p))  # an all -inf (empty) row: NaN -> 0
    return p @ v

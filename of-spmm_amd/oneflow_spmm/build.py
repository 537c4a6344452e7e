"""COO (edge_index) -> CSR construction: HIP kernels on GPU tensors
(csrc/csr_build.hip: stable radix sort + run merge + row_ptr by search), the C++ host version on
CPU tensors; both give the same arrays and the same summed values.  And the product of two CSR
matrices as a CSR (csrc/spgemm.hip: hash tables in LDS; csrc/spgemm_cpu.cpp), DESIGN.md §3p."""
from __future__ import annotations

import ctypes

import torch

from ._C import current_stream_handle, dtype_code
from ._lib import LIB, check


def coo_to_csr(row: torch.Tensor, col: torch.Tensor, values: torch.Tensor | None, m: int, k: int,
               merge_duplicates: bool = True):
    """Returns (row_ptr [m+1], col_idx [nnz'], values [nnz'] or None) in canonical CSR order.
    Duplicates (same row and col) are summed in input order when merge_duplicates."""
    if row.shape != col.shape or row.dim() != 1:
        raise RuntimeError("coo_to_csr: row and col must be 1-D tensors of equal length")
    if row.dtype != col.dtype:
        raise TypeError("coo_to_csr: row and col must have the same index dtype")
    row, col = row.contiguous(), col.contiguous()
    nnz = row.numel()
    it, dev = row.dtype, row.device
    idt = dtype_code(it)
    vdt = dtype_code(values.dtype) if values is not None else dtype_code(torch.float32)
    if values is not None:
        values = values.contiguous()
        if values.shape != row.shape:
            raise RuntimeError("coo_to_csr: values must match row/col")
    out_rp = torch.empty(m + 1, dtype=it, device=dev)
    out_ci = torch.empty(nnz, dtype=it, device=dev)
    out_v = torch.empty(nnz, dtype=values.dtype, device=dev) if values is not None else None
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
    if dev.type == "cpu":
        cnt = ctypes.c_int64(0)
        check(LIB.ofx_coo_to_csr_cpu(idt, vdt, m, k, nnz, ptr(row), ptr(col), ptr(values),
                                     int(merge_duplicates), out_rp.data_ptr(), ptr(out_ci),
                                     ptr(out_v), ctypes.byref(cnt)), "coo_to_csr")
        n_out = cnt.value
    else:
        ws_bytes = ctypes.c_size_t(0)
        check(LIB.ofx_coo_to_csr_workspace_size(idt, m, k, nnz, ctypes.byref(ws_bytes)), "coo_to_csr")
        ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8, device=dev)
        scalars = torch.zeros(2, dtype=torch.int64, device=dev)  # [nnz', bad flag]
        check(LIB.ofx_coo_to_csr(current_stream_handle(row), idt, vdt, m, k, nnz, ptr(row), ptr(col),
                                 ptr(values), int(merge_duplicates), out_rp.data_ptr(), ptr(out_ci),
                                 ptr(out_v), scalars.data_ptr(), scalars.data_ptr() + 8,
                                 ws.data_ptr(), ws_bytes.value), "coo_to_csr")
        n_out, bad = (int(x) for x in scalars.tolist())
        if bad:
            raise RuntimeError(f"coo_to_csr: entries outside the {m} x {k} matrix")
    return out_rp, out_ci[:n_out], (out_v[:n_out] if out_v is not None else None)


def spgemm(row_ptr_a: torch.Tensor, col_idx_a: torch.Tensor, values_a: torch.Tensor | None,
           row_ptr_b: torch.Tensor, col_idx_b: torch.Tensor, values_b: torch.Tensor | None, n: int,
           *, num_threads: int = 0):
    """C = A @ B for A [M, K] and B [K, n], both CSR: returns (row_ptr_c [M+1], col_idx_c [nnz_c],
    values_c [nnz_c]).  M = len(row_ptr_a) - 1 and K = len(row_ptr_b) - 1.  Row i of C holds the
    distinct columns some entry of A's row i reaches through a row of B, strictly ascending, so the
    result is a valid B of the next product (`row_topk(T @ A)` diffusion steps, two-hop and metapath
    graphs, `csr_transpose(S) @ A @ S` coarsening) and every op takes it.  An entry whose products
    cancel is kept with the value +0: the structure does not depend on the values.  A value is the
    sum over A's entries p in order, then B's entries q in order, of a_p * b_q rounded to the value
    dtype, accumulated from +0 in float32 (float64 for float64) and rounded once: the CPU and the
    GPU give the same bits.  values_a and values_b are both None (pattern only: values_c is None)
    or both tensors of one dtype out of float32, float64, float16, bfloat16; no autograd.  The six
    index tensors are 1-D and share one dtype (int32 or int64) and one device, which chooses the
    kernel.  A's rows may be in any order and may repeat a column; a column of A at or above K
    selects a zero row and adds nothing.  B's rows must be strictly ascending in [0, n) (what
    `coo_to_csr` emits with merge_duplicates=True, and what this op emits): anything else raises
    RuntimeError ("ascending" or "outside"), as do a negative column of A and a row whose entry
    range leaves its matrix; none is ever used as an address.  M, K, n and the three entry counts
    are below 2^31.  num_threads is the kCPU kernel's (0: OpenMP's own count) and does not change
    the result."""
    idx = (("row_ptr_a", row_ptr_a), ("col_idx_a", col_idx_a), ("row_ptr_b", row_ptr_b),
           ("col_idx_b", col_idx_b))
    for name, t in idx:
        if not isinstance(t, torch.Tensor) or t.dim() != 1:
            raise RuntimeError(f"spgemm: {name} must be a 1-D tensor")
    if row_ptr_a.numel() < 1 or row_ptr_b.numel() < 1:
        raise RuntimeError("spgemm: a row_ptr must hold at least one entry")
    if len({t.dtype for _, t in idx}) != 1:
        raise TypeError("spgemm: the index tensors must have the same index dtype")
    if (values_a is None) != (values_b is None):
        raise RuntimeError("spgemm: values_a and values_b must both be tensors or both be None")
    valued = values_a is not None
    if valued:
        if values_a.dtype != values_b.dtype:
            raise TypeError("spgemm: values_a and values_b must have the same dtype")
        if values_a.shape != col_idx_a.shape or values_b.shape != col_idx_b.shape:
            raise RuntimeError("spgemm: values must match their col_idx")
        values_a, values_b = values_a.detach().contiguous(), values_b.detach().contiguous()
    if len({t.device for t in (row_ptr_a, col_idx_a, row_ptr_b, col_idx_b)
            + ((values_a, values_b) if valued else ())}) != 1:
        raise RuntimeError("spgemm: every tensor must be on one device")
    rp_a, ci_a, rp_b, ci_b = (t.contiguous() for _, t in idx)
    it, dev = rp_a.dtype, rp_a.device
    vt = values_a.dtype if valued else torch.float32
    idt, vdt = dtype_code(it), dtype_code(vt)
    m, k, n = rp_a.numel() - 1, rp_b.numel() - 1, int(n)
    nnz_a, nnz_b = ci_a.numel(), ci_b.numel()
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
    out_rp = torch.empty(m + 1, dtype=it, device=dev)
    sizes = (m, k, n, nnz_a, nnz_b)
    csr = (ptr(rp_a), ptr(ci_a), ptr(values_a), ptr(rp_b), ptr(ci_b), ptr(values_b))

    def outputs(nnz_c):
        if nnz_c >= 2 ** 31:
            raise RuntimeError(f"spgemm: the product holds {nnz_c} entries, not below 2^31")
        return (torch.empty(nnz_c, dtype=it, device=dev),
                torch.empty(nnz_c, dtype=vt, device=dev) if valued else None)

    if dev.type == "cpu":
        cnt = ctypes.c_int64(0)
        check(LIB.ofx_spgemm_count_cpu(int(num_threads), idt, *sizes, csr[0], csr[1], csr[3], csr[4],
                                       out_rp.data_ptr(), ctypes.byref(cnt)), "spgemm")
        out_ci, out_v = outputs(cnt.value)
        check(LIB.ofx_spgemm_fill_cpu(int(num_threads), idt, vdt, *sizes, cnt.value, *csr,
                                      out_rp.data_ptr(), ptr(out_ci), ptr(out_v)), "spgemm")
        return out_rp, out_ci, out_v
    ws_bytes = ctypes.c_size_t(0)
    check(LIB.ofx_spgemm_workspace_size(idt, vdt, *sizes, ctypes.byref(ws_bytes)), "spgemm")
    stream = current_stream_handle(rp_a)
    ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8, device=dev)
    scalars = torch.zeros(2, dtype=torch.int64, device=dev)  # [nnz_c, bad flag]
    check(LIB.ofx_spgemm_count(stream, idt, *sizes, csr[0], csr[1], csr[3], csr[4], out_rp.data_ptr(),
                               scalars.data_ptr(), scalars.data_ptr() + 8, ws.data_ptr(),
                               ws_bytes.value), "spgemm")
    nnz_c, bad = (int(x) for x in scalars.tolist())  # the one read-back
    if bad & 1:
        raise RuntimeError("spgemm: a row whose degree is outside [0, 2^31) or whose entries are "
                           f"outside its matrix, a negative column of A, or a column of B outside "
                           f"[0, {n})")
    if bad:
        raise RuntimeError("spgemm: a row of B is not strictly ascending (pass B through "
                           "coo_to_csr with merge_duplicates=True)")
    out_ci, out_v = outputs(nnz_c)
    check(LIB.ofx_spgemm_fill(stream, idt, vdt, *sizes, nnz_c, *csr, out_rp.data_ptr(), ptr(out_ci),
                              ptr(out_v), ws.data_ptr(), ws_bytes.value), "spgemm")
    return out_rp, out_ci, out_v

"""The checks of the GAT attention weights (ops "gat_softmax_csr_heads" and its gradient), written
once for both devices (test_gat_softmax_cpu.py runs them on host tensors, test_gat_softmax_gpu.py on
the GPU, where every result is also compared with the kCPU entry's bits).  Every comparison is bit
for bit unless it says otherwise.

The reference is never the code under test.  The scores are restated in numpy (a float32 / float64
add, the z > 0 select and one multiply, helpers.from_f32 for the rounding to T), then fed to the
existing ofx_edge_softmax_csr_heads_cpu and, per column, to edge_softmax_helpers.ref_forward.
Backward: ref_backward gives de, the numpy mask multiply ds, edge_softmax_helpers.tree_sum d_row and
autograd.TRANSPOSE_CACHE.grad_b_heads (the multi-head SpMM on the transpose) d_col."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import edge_softmax_heads_cases as hc
import oneflow_spmm as flow_spmm
from edge_softmax_cases import scores
from edge_softmax_helpers import ref_backward, ref_forward, tree_sum
from helpers import assert_bitwise, from_f32
from oneflow_spmm import _C, _lib, autograd
from oneflow_spmm._C import current_stream_handle, dtype_code
from oneflow_spmm._lib import LIB, check
from reduce_helpers import acc, assert_same, is_sentinel, options, sentinel, store

K = 37  # columns: far fewer than the nonzeros of the long rows, so columns repeat within a row
SLOPES = [0.2, 1.0, 0.01]
to_dev = hc.to_dev


def problem(lengths, heads, dtype, idx_dtype=torch.int32, m=None, seed=0, exact=False, k=K,
            col_range=None):
    """(row_ptr, col_idx, s_row [M, H], s_col [K, H], g [nnz, H]); columns drawn with repetition
    from [0, k), or from col_range = (lo, hi) to reach outside of it."""
    rp, ci = hc.csr_of(lengths, idx_dtype, m, seed)
    rng = np.random.default_rng(seed + 1)
    m, nnz = rp.numel() - 1, ci.numel()
    lo, hi = col_range if col_range is not None else (0, k)
    ci = torch.from_numpy(rng.integers(lo, hi, size=nnz)).to(idx_dtype)
    s_row = scores(m * heads, dtype, rng, exact).view(m, heads)
    s_col = scores(k * heads, dtype, rng, exact).view(k, heads)
    g = scores(nnz * heads, dtype, rng, exact).view(nnz, heads)
    return rp, ci, s_row, s_col, g


def tensor_of(x: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
    """reduce_helpers.store()'s representation (bf16 as uint16 bits) as a torch tensor."""
    x = np.ascontiguousarray(x)
    if dtype == torch.bfloat16:
        return torch.from_numpy(x.view(np.int16)).view(torch.bfloat16)
    return torch.from_numpy(x)


# ---- the contract's new steps in numpy -------------------------------------------------------------
def ref_scores(rp, ci, s_row, s_col, slope, activate=True):
    """(e [nnz, H] rounded to T, z [nnz, H] in the accumulation type) for host tensors."""
    A = np.float64 if s_row.dtype == torch.float64 else np.float32
    rpn = rp.numpy().astype(np.int64)
    rows = np.repeat(np.arange(len(rpn) - 1), np.diff(rpn))
    c = ci.numpy().astype(np.int64)
    k, heads = s_col.shape
    ok = (c >= 0) & (c < k)
    sr, sc = acc(s_row).astype(A), acc(s_col).astype(A)
    gathered = np.zeros((len(c), heads), dtype=A)  # a column outside [0, K) reads +0
    gathered[ok] = sc[c[ok]]
    with np.errstate(invalid="ignore", over="ignore"):
        z = (sr[rows] + gathered).astype(A)
        u = np.where(z > 0, z, (z * A(slope)).astype(A)) if activate else z.copy()
    u[np.isnan(u)] = np.nan  # the canonical quiet NaN
    e = torch.from_numpy(u) if A is np.float64 else from_f32(u, s_row.dtype)
    return e, z


def ref_grad(rp, ci, y, g, z, slope):
    """(ds [nnz, H], d_row [M, H]) from the stored weights y, the upstream g and the sums z."""
    dtype, A = y.dtype, z.dtype.type
    rpn = rp.numpy().astype(np.int64)
    m, heads = len(rpn) - 1, y.shape[1]
    ds = torch.empty_like(y)
    d_row = np.zeros((m, heads), dtype=A)
    with np.errstate(invalid="ignore", over="ignore"):
        for h in range(heads):
            de = acc(tensor_of(ref_backward(rp, y[:, h].contiguous(), g[:, h].contiguous()), dtype))
            factor = np.where(z[:, h] > 0, A(1), A(slope))
            ds[:, h] = tensor_of(store((de.astype(A) * factor).astype(A), dtype), dtype)
            loaded = acc(ds[:, h].contiguous()).astype(A)
            for r in range(m):
                if rpn[r + 1] > rpn[r]:
                    d_row[r, h] = tree_sum(loaded[rpn[r]:rpn[r + 1]])
    return ds, tensor_of(store(d_row, dtype), dtype)


# ---- C-ABI callers ---------------------------------------------------------------------------------
_ptr = hc._ptr


def _workspace(it, vt, m, k, heads, nnz, o, dev):
    size = ctypes.c_size_t(7)
    check(LIB.ofx_gat_softmax_csr_heads_workspace_size(it, vt, m, k, heads, nnz, o,
                                                       ctypes.byref(size)), "gat workspace size")
    assert size.value == 0
    return torch.empty(1, dtype=torch.uint8, device=dev), size.value


def run_forward(rp, ci, s_row, s_col, slope, *, row_begin=0, row_end=None, opts=None, shift=0,
                threads=0):
    """ofx_gat_softmax_csr_heads(_cpu) on the tensors' device: all [nnz, H] entries of attn, those
    outside the rows [row_begin, row_end) still holding sentinel()'s bits.  s_row is passed from
    row_begin on; s_row, s_col and attn start `shift` elements into their buffers."""
    m, k = rp.numel() - 1, s_col.shape[0]
    row_end = m if row_end is None else row_end
    dev, heads, nnz = s_row.device, s_row.shape[1], ci.numel()
    sr, sc = hc.shifted(s_row[row_begin:], shift), hc.shifted(s_col, shift)
    attn = hc._out((nnz, heads), s_row.dtype, dev, shift)
    it, vt = dtype_code(rp.dtype), dtype_code(s_row.dtype)
    o = ctypes.byref(opts) if opts is not None else None
    args = (it, vt, m, k, heads, nnz, _ptr(rp), _ptr(ci), _ptr(sr), _ptr(sc), float(slope),
            _ptr(attn), row_begin, row_end)
    if dev.type == "cpu":
        check(LIB.ofx_gat_softmax_csr_heads_cpu(threads, *args, o), "gat cpu")
    else:
        ws, size = _workspace(it, vt, m, k, heads, nnz, o, dev)
        check(LIB.ofx_gat_softmax_csr_heads(current_stream_handle(s_row), *args, ws.data_ptr(),
                                            size, o), "gat")
    return attn


def run_backward(rp, ci, s_row, s_col, slope, y, g, *, row_begin=0, row_end=None, opts=None,
                 shift=0, threads=0):
    """ofx_gat_softmax_csr_heads_grad(_cpu): (ds [nnz, H], d_row [M - row_begin, H]) over
    sentinels, as run_forward."""
    m, k = rp.numel() - 1, s_col.shape[0]
    row_end = m if row_end is None else row_end
    dev, heads, nnz = s_row.device, s_row.shape[1], ci.numel()
    sr, sc = hc.shifted(s_row[row_begin:], shift), hc.shifted(s_col, shift)
    yy, gg = hc.shifted(y, shift), hc.shifted(g, shift)
    ds = hc._out((nnz, heads), s_row.dtype, dev, shift)
    d_row = hc._out((m - row_begin, heads), s_row.dtype, dev, shift)
    it, vt = dtype_code(rp.dtype), dtype_code(s_row.dtype)
    o = ctypes.byref(opts) if opts is not None else None
    args = (it, vt, m, k, heads, nnz, _ptr(rp), _ptr(ci), _ptr(sr), _ptr(sc), float(slope),
            _ptr(yy), _ptr(gg), _ptr(ds), _ptr(d_row), row_begin, row_end)
    if dev.type == "cpu":
        check(LIB.ofx_gat_softmax_csr_heads_grad_cpu(threads, *args, o), "gat grad cpu")
    else:
        ws, size = _workspace(it, vt, m, k, heads, nnz, o, dev)
        check(LIB.ofx_gat_softmax_csr_heads_grad(current_stream_handle(s_row), *args,
                                                 ws.data_ptr(), size, o), "gat grad")
    return ds, d_row


# ---- checks ----------------------------------------------------------------------------------------
def check_problem(dev, rp, ci, s_row, s_col, g, slope=0.2, *, shift=0, per_column=True, what=""):
    """Forward and gradient of one problem against the reference chain and, on the GPU, against the
    kCPU entry.  Returns (attn, ds, d_row) on `dev`."""
    heads = s_row.shape[1]
    e, z = ref_scores(rp, ci, s_row, s_col, slope)
    want = hc.run_forward(rp, e, rp.numel() - 1)  # the existing kCPU multi-head edge softmax
    d = to_dev(dev, rp, ci, s_row, s_col, g)
    attn = run_forward(*d[:4], slope, shift=shift)
    assert_same(attn, want, f"{what} forward vs edge_softmax_csr_heads_cpu on the numpy scores")
    if per_column:
        for h in range(heads):
            assert_bitwise(attn[:, h], ref_forward(rp, e[:, h].contiguous()),
                           f"{what} forward head {h} vs numpy")
    ds, d_row = run_backward(*d[:4], slope, attn, d[4], shift=shift)
    want_ds, want_d_row = ref_grad(rp, ci, want, g, z, slope)
    assert_same(ds, want_ds, f"{what} ds")
    assert_same(d_row, want_d_row, f"{what} d_row")
    if dev != "cpu":
        assert_same(attn, run_forward(rp, ci, s_row, s_col, slope), f"{what} forward vs kCPU")
        k_ds, k_d_row = run_backward(rp, ci, s_row, s_col, slope, want, g)
        assert_same(ds, k_ds, f"{what} ds vs kCPU")
        assert_same(d_row, k_d_row, f"{what} d_row vs kCPU")
    return attn, ds, d_row


def check_boundaries(dev, heads, dtype, idx_dtype):
    """One CSR with a row of every boundary length, every head count of both paths, K = 37."""
    p = problem(hc.BOUNDARY, heads, dtype, idx_dtype, seed=heads)
    check_problem(dev, *p, what=f"boundary H={heads} {dtype} {idx_dtype}")


def check_lane_groups(dev, mix, heads, dtype):
    """CSRs whose mean degree picks LG = 1, 4 and 16, with rows taken over by the wave."""
    p = problem(hc.LG_MIXES[mix], heads, dtype, m=40, seed=len(mix) + heads, exact=True)
    check_problem(dev, *p, slope=0.01, what=f"{mix} H={heads} {dtype}")


def check_many_rows(dev, heads, dtype):
    """2,500 rows with power-law degrees of mean 3 and two long rows: more than one block at
    LG = 1, with take-overs by the wave."""
    from helpers import power_law_degrees
    m = 2500
    deg = power_law_degrees(m, 3 * m, 4096, np.random.default_rng(5))
    deg[123], deg[2000] = 600, 1100
    assert 2 * (int(deg.sum()) // m) <= 8  # LG = 1
    p = problem([int(x) for x in deg], heads, dtype, seed=6)
    check_problem(dev, *p, per_column=False, what=f"many rows H={heads} {dtype}")


def check_unaligned_and_ranges(dev, heads, dtype):
    """Every base one element off the vector alignment (the general path) gives the aligned bits;
    a row range reads s_row and writes d_row from row_begin on and writes exactly
    [row_ptr[rb] * H, row_ptr[re] * H) of attn and ds; options change no bit."""
    slope = 0.2
    rp, ci, s_row, s_col, g = problem([0, 1, 7, 8, 9, 33, 64, 65, 129, 513, 1030, 3], heads, dtype,
                                      seed=17)
    m = rp.numel() - 1
    attn, ds, d_row = check_problem(dev, rp, ci, s_row, s_col, g, slope, per_column=False,
                                    what="aligned")
    d = to_dev(dev, rp, ci, s_row, s_col)
    d_g = g.to(dev)
    assert_same(run_forward(*d, slope, shift=1), attn, "forward, bases + 1 element")
    s_ds, s_d_row = run_backward(*d, slope, attn, d_g, shift=1)
    assert_same(s_ds, ds, "ds, bases + 1 element")
    assert_same(s_d_row, d_row, "d_row, bases + 1 element")
    for name, o in (("ordered", options(ordered=True)), ("split8", options(split=8, chunk=4)),
                    ("planned", options(planned=True))):
        assert_same(run_forward(*d, slope, opts=o), attn, f"forward {name}")
        o_ds, o_d_row = run_backward(*d, slope, attn, d_g, opts=o)
        assert_same(o_ds, ds, f"ds {name}")
        assert_same(o_d_row, d_row, f"d_row {name}")
    rpn = rp.numpy().astype(np.int64)
    for lo, hi in ((1, m - 1), (3, 4), (2, 9), (5, 5), (0, 0), (m, m), (0, m)):
        j0, j1 = int(rpn[lo]), int(rpn[hi])
        for shift in (0, 1):
            part = run_forward(*d, slope, row_begin=lo, row_end=hi, shift=shift)
            p_ds, p_d_row = run_backward(*d, slope, attn, d_g, row_begin=lo, row_end=hi,
                                         shift=shift)
            for name, got, full in (("attn", part, attn), ("ds", p_ds, ds)):
                assert_same(got[j0:j1], full[j0:j1], f"{name} rows [{lo}, {hi}) shift {shift}")
                kept = is_sentinel(got)
                assert bool(kept[:j0].all()) and bool(kept[j1:].all()), \
                    f"{name} rows [{lo}, {hi}) shift {shift}: wrote outside [{j0}, {j1}) * H"
            assert_same(p_d_row[:hi - lo], d_row[lo:hi], f"d_row rows [{lo}, {hi}) shift {shift}")
            assert bool(is_sentinel(p_d_row[hi - lo:]).all()), \
                f"d_row rows [{lo}, {hi}) shift {shift}: wrote past the range"


def check_columns_out_of_range(dev, dtype):
    """Columns outside [0, K) (negative ones included) read s_col = +0, on the packed path (8
    heads) and the general one (3); the transpose drops the columns >= K from d(s_col) (it refuses
    negative ones, as for every op whose gradient goes through it)."""
    for heads in (8, 3):
        p = problem([0, 1, 7, 9, 33, 65, 129, 600], heads, dtype, seed=3, col_range=(-5, 2 * K))
        assert int((p[1] >= K).sum()) > 0 and int((p[1] < 0).sum()) > 0
        check_problem(dev, *p, per_column=False, what=f"columns outside [0, K) H={heads} {dtype}")
    check_grads(dev, 3, dtype, col_range=(0, 2 * K))


def check_activation_edges(dev, dtype, slope):
    """Exact inputs at the activation's edges, one row each: z = +0, z = -0, s_row = -s_col, the
    smallest negative z, and sums that T cannot hold (257 in bf16, 2049 in f16: the score is
    rounded to T before the softmax, so it ties with its neighbour 256 / 2048 and both weights are
    exactly 1/2).  Slope 1 gives the bits of edge_softmax on the rounded z."""
    tiny = {torch.float32: 2.0 ** -149, torch.float64: 5e-324, torch.bfloat16: 2.0 ** -133,
            torch.float16: 2.0 ** -24}[dtype]
    big = {torch.bfloat16: 256.0, torch.float16: 2048.0}.get(dtype, 4.0)
    #        s_row   s_col by column
    rows = [(0.0, [0.0, 1.0, -2.0]),        # +0 among a positive and a negative z
            (-0.0, [-0.0, 1.0, -2.0]),      # -0: the multiply branch keeps the sign
            (3.0, [-3.0, -3.0, 1.0]),       # cancellation: +0 twice
            (-tiny, [0.0, tiny, -tiny]),    # the smallest negative z, an exact +0 and 2 * tiny
            (big, [1.0, 0.0]),              # big + 1 is not a T value in bf16 / f16
            (-big, [-1.0, 0.0, 1.0])]       # the same below zero
    heads = 2
    lens = [len(c) for _, c in rows]
    rp = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
    key = lambda v: (float(v), bool(np.signbit(v)))  # noqa: E731  (+0 and -0 are two columns)
    cols = sorted({key(v) for _, c in rows for v in c})
    col_of = {kv: i for i, kv in enumerate(cols)}
    cols = [-0.0 if neg and v == 0 else v for v, neg in cols]
    ci = torch.tensor([col_of[key(v)] for _, c in rows for v in c], dtype=torch.int32)
    f64 = np.float64 if dtype == torch.float64 else np.float32
    mk = lambda vals: torch.from_numpy(np.array(vals, dtype=f64)).to(dtype)  # noqa: E731
    s_row = mk([[r, r] for r, _ in rows])
    s_col = mk([[v, v] for v in cols])
    assert s_row[3, 0].item() == -tiny and bool(np.signbit(s_row[1, 0].item()))
    g = scores(ci.numel() * heads, dtype, np.random.default_rng(4), True).view(-1, heads)
    attn, _, _ = check_problem(dev, rp, ci, s_row, s_col, g, slope,
                               what=f"activation edges {dtype} slope {slope}")
    if dtype in (torch.bfloat16, torch.float16):
        j = int(rp[4])
        assert attn[j:j + 2].cpu().float().tolist() == [[0.5, 0.5], [0.5, 0.5]], \
            "the score is rounded to T before the softmax"
    if slope == 1.0:
        z_t, _ = ref_scores(rp, ci, s_row, s_col, slope, activate=False)
        d_rp, d_ci, d_z = to_dev(dev, rp, ci, z_t)
        assert_same(attn, _C.edge_softmax_csr_heads(d_rp, d_ci, d_z),
                    "slope 1 vs edge_softmax on the rounded z")


def check_special_confined(dev, dtype):
    """One row holds a NaN in head 0, +inf in head 1, -inf in head 2 (an all -inf row) of s_row and
    one nonzero masked with -inf in head 3 (through a column no other row reads); heads 4..7 and
    every other row stay finite."""
    heads, lens = 8, [3, 11, 0, 70, 5, 600]
    rp, ci, s_row, s_col, g = problem(lens, heads, dtype, seed=5, k=K - 1)
    s_col = torch.cat([s_col, s_col[:1]])  # column K - 1: read by the marked nonzero only
    rpn = rp.numpy()
    marked = {}
    for r in (1, 3, 5):
        j0, j1 = int(rpn[r]), int(rpn[r + 1])
        marked[r] = j0 + (j1 - j0) // 2
        ci[marked[r]] = K - 1
    s_col[K - 1, 3] = float("-inf")
    for r in marked:
        s_row[r, 0], s_row[r, 1], s_row[r, 2] = float("nan"), float("inf"), float("-inf")
    attn, ds, d_row = check_problem(dev, rp, ci, s_row, s_col, g, what=f"special {dtype}")
    a = attn.cpu().double()
    for r in range(len(lens)):
        j0, j1 = int(rpn[r]), int(rpn[r + 1])
        if r in marked:
            assert bool(torch.isnan(a[j0:j1, :3]).all()), f"row {r}: heads 0..2 are NaN"
            assert not bool(torch.isnan(a[j0:j1, 3:]).any()), f"row {r}: a NaN leaked into 3.."
            assert a[marked[r], 3] == 0 and abs(float(a[j0:j1, 3].sum()) - 1) < 2e-2
        else:
            assert not bool(torch.isnan(a[j0:j1]).any()), f"row {r}: a NaN leaked into the row"


def check_degenerate(dev, dtype):
    """H == 1 gives the bits of the single-head edge softmax on e; H == 0, nnz == 0 and an empty
    range write nothing."""
    rp, ci, s_row, s_col, g = problem(hc.BOUNDARY, 1, dtype, seed=23)
    d = to_dev(dev, rp, ci, s_row, s_col)
    attn = run_forward(*d, 0.2)
    e, _ = ref_scores(rp, ci, s_row, s_col, 0.2)
    assert_same(attn[:, 0], _C.edge_softmax_csr(d[0], d[1], e[:, 0].contiguous().to(dev)),
                "H == 1 vs edge_softmax_csr")
    check_problem(dev, rp, ci, s_row, s_col, g, per_column=False, what="H == 1")
    m, nnz = rp.numel() - 1, ci.numel()
    none_m, none_k = (torch.empty((r, 0), dtype=dtype, device=dev) for r in (m, K))
    none_e = torch.empty((nnz, 0), dtype=dtype, device=dev)
    assert run_forward(d[0], d[1], none_m, none_k, 0.2).shape == (nnz, 0)
    assert run_backward(d[0], d[1], none_m, none_k, 0.2, none_e, none_e)[1].shape == (m, 0)
    rp0 = torch.zeros(4, dtype=torch.int32, device=dev)
    s3 = s_row[:3].repeat(1, 4).to(dev)
    sk = s_col.repeat(1, 4).to(dev)
    no_e = torch.empty((0, 4), dtype=dtype, device=dev)
    assert run_forward(rp0, rp0[:0], s3, sk, 0.2).shape == (0, 4)
    _, d_row0 = run_backward(rp0, rp0[:0], s3, sk, 0.2, no_e, no_e)
    assert bool(is_sentinel(d_row0).all()), "nnz == 0 writes nothing"
    part = run_forward(*d, 0.2, row_begin=2, row_end=2)
    assert bool(is_sentinel(part).all()), "an empty range writes nothing"
    # the public entry on the same degenerate shapes
    assert tuple(flow_spmm.gat_softmax(rp0, rp0[:0], s3, sk).shape) == (0, 4)
    assert tuple(flow_spmm.gat_softmax(d[0], d[1], none_m, none_k).shape) == (nnz, 0)
    a = s3.clone().requires_grad_(True)
    flow_spmm.gat_softmax(rp0, rp0[:0], a, sk).sum().backward()
    assert a.grad is not None and not bool(a.grad.any()), "nnz == 0: d(s_row) is +0"


def check_argument_checks(dev):
    """NULLs, overlapping buffers, a bad slope, a bad range, a negative H and bad dtypes return the
    documented code and launch nothing: the outputs keep their sentinels."""
    rp = torch.tensor([0, 2, 3], dtype=torch.int32, device=dev)
    ci = torch.tensor([0, 1, 1], dtype=torch.int32, device=dev)
    s_row = torch.tensor([[1.0, 2.0], [2.0, 0.0]], device=dev)
    s_col = torch.tensor([[0.5, -2.0], [-3.0, 1.0]], device=dev)
    g = torch.tensor([[1.0, 2.0], [2.0, 0.0], [3.0, 1.0]], device=dev)
    attn = sentinel((3, 2), torch.float32, dev)
    ds = sentinel((3, 2), torch.float32, dev)
    d_row = sentinel((2, 2), torch.float32, dev)
    I, F, EINVAL = _lib.DT_INT32, _lib.DT_FLOAT, _lib.OFX_EINVAL
    if dev == "cpu":
        fwd = lambda *a: LIB.ofx_gat_softmax_csr_heads_cpu(0, *a, None)       # noqa: E731
        bwd = lambda *a: LIB.ofx_gat_softmax_csr_heads_grad_cpu(0, *a, None)  # noqa: E731
    else:
        s = current_stream_handle(g)
        fwd = lambda *a: LIB.ofx_gat_softmax_csr_heads(s, *a, None, 0, None)       # noqa: E731
        bwd = lambda *a: LIB.ofx_gat_softmax_csr_heads_grad(s, *a, None, 0, None)  # noqa: E731
    ins = (rp.data_ptr(), ci.data_ptr(), s_row.data_ptr(), s_col.data_ptr())
    for call, outs in ((fwd, (attn.data_ptr(),)),
                       (bwd, (g.data_ptr(), g.data_ptr(), ds.data_ptr(), d_row.data_ptr()))):
        ok = lambda slope=0.2, h=2, nnz=3, p=ins, o=outs, rb=0, re=2, it=I, vt=F, k=2: call(  # noqa: E731
            it, vt, 2, k, h, nnz, *p, slope, *o, rb, re)
        assert ok(h=-1) == EINVAL and ok(nnz=-3) == EINVAL and ok(k=-1) == EINVAL
        assert ok(rb=1, re=3) == EINVAL and ok(rb=2, re=1) == EINVAL          # row range
        for bad in (0.0, -0.2, float("nan"), float("inf"), 1e-60, 1e60):      # the slope, as f32
            assert ok(slope=bad) == EINVAL, bad
        for i in range(4):                                                    # a NULL input
            assert ok(p=ins[:i] + (None,) + ins[i + 1:]) == EINVAL, i
        for i in range(len(outs)):                                            # a NULL y / g / output
            assert ok(o=outs[:i] + (None,) + outs[i + 1:]) == EINVAL, i
        for i in range(4):                                                    # an output on an input
            assert ok(o=outs[:-1] + (ins[i],)) == EINVAL, i
        assert ok(vt=_lib.DT_INT64) == _lib.OFX_EUNSUPPORTED
        assert ok(it=F) == _lib.OFX_EUNSUPPORTED
        assert ok(nnz=1 << 31) == EINVAL                                      # int32 and nnz
        assert ok(h=0) == _lib.OFX_OK and ok(rb=1, re=1) == _lib.OFX_OK       # nothing to do
    # f64 keeps slopes that f32 cannot hold
    assert bwd(I, _lib.DT_DOUBLE, 2, 2, 0, 3, *ins, 1e-60, g.data_ptr(), g.data_ptr(),
               ds.data_ptr(), d_row.data_ptr(), 0, 2) == _lib.OFX_OK
    # ds on the upstream gradient, d_row on ds
    assert bwd(I, F, 2, 2, 2, 3, *ins, 0.2, attn.data_ptr(), g.data_ptr(), g.data_ptr(),
               d_row.data_ptr(), 0, 2) == EINVAL
    assert bwd(I, F, 2, 2, 2, 3, *ins, 0.2, attn.data_ptr(), g.data_ptr(), ds.data_ptr(),
               ds.data_ptr(), 0, 2) == EINVAL
    size = ctypes.c_size_t(7)
    query = LIB.ofx_gat_softmax_csr_heads_workspace_size
    assert query(I, F, 2, 2, 2, 3, None, ctypes.byref(size)) == _lib.OFX_OK and size.value == 0
    assert query(I, F, 2, 2, 2, 3, None, None) == EINVAL
    assert query(I, F, 2, 2, -2, 3, None, ctypes.byref(size)) == EINVAL
    bad = _lib.Options()
    bad.magic = 0
    if dev == "cpu":
        assert LIB.ofx_gat_softmax_csr_heads_cpu(0, I, F, 2, 2, 2, 3, *ins, 0.2, attn.data_ptr(),
                                                 0, 2, ctypes.byref(bad)) == EINVAL
    else:
        s = current_stream_handle(g)
        assert LIB.ofx_gat_softmax_csr_heads(s, I, F, 2, 2, 2, 3, *ins, 0.2, attn.data_ptr(), 0, 2,
                                             None, 0, ctypes.byref(bad)) == EINVAL
        # a NULL workspace with a non-zero size
        assert LIB.ofx_gat_softmax_csr_heads(s, I, F, 2, 2, 2, 3, *ins, 0.2, attn.data_ptr(), 0, 2,
                                             None, 16, None) == _lib.OFX_EWORKSPACE
        assert LIB.ofx_gat_softmax_csr_heads_grad(
            s, I, F, 2, 2, 2, 3, *ins, 0.2, g.data_ptr(), g.data_ptr(), ds.data_ptr(),
            d_row.data_ptr(), 0, 2, None, 16, None) == _lib.OFX_EWORKSPACE
        torch.cuda.synchronize()
    assert all(bool(is_sentinel(t).all()) for t in (attn, ds, d_row)), "an error launched"
    assert fwd(I, F, 2, 2, 2, 3, *ins, 0.2, attn.data_ptr(), 0, 2) == _lib.OFX_OK
    assert not bool(is_sentinel(attn).any())


def check_registrations():
    """Both ops for every dtype x index type x device, through the tmp-size query of the functional
    entries (inference and kernel choice; nothing is launched, the descriptors carry NULL): one
    kernel matches and its tmp size is the workspace query's."""
    m, k, nnz, heads = 2, 4, 601, 2
    for dev in (-1, 0):
        for vt in (_lib.DT_FLOAT, _lib.DT_DOUBLE, _lib.DT_FLOAT16, _lib.DT_BFLOAT16):
            for it in (_lib.DT_INT32, _lib.DT_INT64):
                def d(dtype, *shape):
                    t = _lib.TensorDesc()
                    t.dtype, t.device, t.ndim, t.data = dtype, dev, len(shape), None
                    for i, s in enumerate(shape):
                        t.shape[i] = s
                        t.stride[i] = shape[1] if i == 0 and len(shape) == 2 else 1
                    return ctypes.byref(t)
                rp, ci = d(it, m + 1), d(it, nnz)
                sr, sc, e = d(vt, m, heads), d(vt, k, heads), d(vt, nnz, heads)
                want = ctypes.c_size_t(5)
                check(LIB.ofx_gat_softmax_csr_heads_workspace_size(it, vt, m, k, heads, nnz, None,
                                                                   ctypes.byref(want)), "query")
                got = ctypes.c_size_t(1 << 40)
                check(LIB.ofx_functional_gat_softmax_csr_heads(None, rp, ci, sr, sc, 0.2, None,
                                                               None, 0, ctypes.byref(got)), "fwd")
                assert got.value == want.value == 0, (dev, vt, it)
                got = ctypes.c_size_t(1 << 40)
                check(LIB.ofx_functional_gat_softmax_csr_heads_grad(
                    None, rp, ci, sr, sc, e, e, 0.2, None, None, None, 0, ctypes.byref(got)), "bwd")
                assert got.value == want.value == 0, (dev, vt, it)


def check_sbp():
    """The SBP strings are those of edge_softmax_csr_heads: one all-broadcast signature."""
    for op, vals in (("gat_softmax_csr_heads", ("s_row", "s_col", "out")),
                     ("gat_softmax_csr_heads_grad", ("s_row", "s_col", "y", "dy", "ds", "d_row"))):
        s = _C.sbp_signatures(op)
        sigs, no_grad = s.split("|")
        assert len(sigs.split(";")) == 1, s  # all-broadcast only
        want = {"a_csr_row_ptr:B", "a_csr_col_idx:B"} | {f"{v}:B" for v in vals}
        assert set(sigs.split(",")) == want, s
        assert set(no_grad.split(":")[1].split(",")) == {"a_csr_row_ptr", "a_csr_col_idx"}, s
    ref = _C.sbp_signatures("edge_softmax_csr_heads")
    assert _C.sbp_signatures("gat_softmax_csr_heads").replace("s_row:B,s_col:B", "e:B") == ref


def check_op_layer(dev):
    """Both ops through the registry dispatch against the C-ABI, for every dtype and index type, and
    the refusals of the Python layer and of the op's own inference."""
    for dt, it, heads in ((torch.float32, torch.int32, 4), (torch.float64, torch.int64, 5),
                          (torch.bfloat16, torch.int32, 8), (torch.float16, torch.int64, 3)):
        p = problem([3, 0, 9, 40, 600], heads, dt, it, seed=8)
        d_rp, d_ci, d_sr, d_sc, d_g = to_dev(dev, *p)
        y = _C.gat_softmax_csr_heads(d_rp, d_ci, d_sr, d_sc, 0.01)
        assert y.shape == d_g.shape and y.dtype == dt
        assert_same(y, run_forward(d_rp, d_ci, d_sr, d_sc, 0.01), f"op vs C-ABI {dt} {it}")
        ds, d_row = _C.gat_softmax_csr_heads_grad(d_rp, d_ci, d_sr, d_sc, y, d_g, 0.01)
        w_ds, w_d_row = run_backward(d_rp, d_ci, d_sr, d_sc, 0.01, y, d_g)
        assert_same(ds, w_ds, f"grad op ds vs C-ABI {dt} {it}")
        assert_same(d_row, w_d_row, f"grad op d_row vs C-ABI {dt} {it}")
    with pytest.raises(RuntimeError, match="2-D"):
        _C.gat_softmax_csr_heads(d_rp, d_ci, d_sr[:, 0].contiguous(), d_sc)
    with pytest.raises(RuntimeError, match="a_num_rows"):
        _C.gat_softmax_csr_heads(d_rp, d_ci, d_sr[:-1], d_sc)
    with pytest.raises(RuntimeError, match="number of heads"):
        _C.gat_softmax_csr_heads(d_rp, d_ci, d_sr, d_sc[:, :2])
    with pytest.raises(RuntimeError, match="nnz"):
        _C.gat_softmax_csr_heads_grad(d_rp, d_ci, d_sr, d_sc, y[:-1], d_g[:-1])
    with pytest.raises(TypeError, match="dtype of a_csr_row_ptr"):
        _C.gat_softmax_csr_heads(d_rp, d_ci.int(), d_sr, d_sc)
    with pytest.raises(TypeError, match="equal to s_row"):
        _C.gat_softmax_csr_heads(d_rp, d_ci, d_sr, d_sc.double())
    with pytest.raises(_lib.OfxError, match="negative_slope"):
        _C.gat_softmax_csr_heads(d_rp, d_ci, d_sr, d_sc, 0.0)
    # the functional entries themselves: the op's own inference refuses what the Python layer does
    o = torch.empty_like(y)
    byref = lambda *ts: [ctypes.byref(_C.desc(t)) for t in ts]  # noqa: E731
    size = ctypes.c_size_t(123)
    fwd, bwd = LIB.ofx_functional_gat_softmax_csr_heads, LIB.ofx_functional_gat_softmax_csr_heads_grad
    check(fwd(None, *byref(d_rp, d_ci, d_sr, d_sc), 0.2, None, None, 0, ctypes.byref(size)), "tmp")
    assert size.value == 0
    check(fwd(current_stream_handle(d_sr), *byref(d_rp, d_ci, d_sr, d_sc), 0.2,
              *byref(o), None, 0, None), "run")
    assert_same(o, run_forward(d_rp, d_ci, d_sr, d_sc, 0.2), "functional entry")
    rc = fwd(None, *byref(d_rp, d_ci, d_sr, d_sc[:, :2].contiguous()), 0.2, None, None, 0,
             ctypes.byref(size))
    assert rc != 0 and b"heads" in LIB.ofx_last_error()
    rc = fwd(None, *byref(d_rp, d_ci, d_sr[:-1].contiguous(), d_sc), 0.2, None, None, 0,
             ctypes.byref(size))
    assert rc != 0 and b"a_num_rows" in LIB.ofx_last_error()
    rc = bwd(None, *byref(d_rp, d_ci, d_sr, d_sc, y, d_g[:-1].contiguous()), 0.2, None, None, None,
             0, ctypes.byref(size))
    assert rc != 0 and b"nnz" in LIB.ofx_last_error()


def check_public_api(dev):
    """gat_softmax on 1-D and 2-D inputs, out=, the error for out= under autograd, non-contiguous
    inputs, and CPU and GPU tensors giving the same bits."""
    rp, ci, s_row, s_col, g = problem([0, 1, 7, 9, 33, 65, 129, 600], 3, torch.float32, seed=31)
    d_rp, d_ci, d_sr, d_sc, d_g = to_dev(dev, rp, ci, s_row, s_col, g)
    want = run_forward(rp, ci, s_row, s_col, 0.2)  # the kCPU entry
    got = flow_spmm.gat_softmax(d_rp, d_ci, d_sr, d_sc)
    assert_same(got, want, "2-D inputs, the default slope")
    assert_same(flow_spmm.gat_softmax(d_rp, d_ci, d_sr, d_sc, 0.01),
                run_forward(rp, ci, s_row, s_col, 0.01), "negative_slope=0.01")
    flat = flow_spmm.gat_softmax(d_rp, d_ci, d_sr[:, 1], d_sc[:, 1])  # non-contiguous columns
    assert flat.dim() == 1
    assert_same(flat, run_forward(rp, ci, s_row[:, 1:2], s_col[:, 1:2], 0.2)[:, 0], "1-D inputs")
    out = sentinel(tuple(got.shape), got.dtype, dev)
    assert flow_spmm.gat_softmax(d_rp, d_ci, d_sr, d_sc, out=out) is out
    assert_same(out, want, "out=")
    out1 = sentinel((ci.numel(),), got.dtype, dev)
    assert flow_spmm.gat_softmax(d_rp, d_ci, d_sr[:, 1], d_sc[:, 1], out=out1) is out1
    assert_same(out1, flat, "out= with 1-D inputs")
    a = d_sr.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="out="):
        flow_spmm.gat_softmax(d_rp, d_ci, a, d_sc, out=out)
    with pytest.raises(RuntimeError, match="out must be"):
        flow_spmm.gat_softmax(d_rp, d_ci, d_sr, d_sc, out=torch.empty_like(got).t().contiguous().t())
    with pytest.raises(RuntimeError, match="expected"):
        flow_spmm.gat_softmax(d_rp, d_ci, d_sr, d_sc[:, 0])
    wide_r = torch.zeros((d_sr.shape[0], 5), dtype=d_sr.dtype, device=dev)
    wide_c = torch.zeros((d_sc.shape[0], 5), dtype=d_sc.dtype, device=dev)
    wide_r[:, 1:4], wide_c[:, 1:4] = d_sr, d_sc
    assert_same(flow_spmm.gat_softmax(d_rp, d_ci, wide_r[:, 1:4], wide_c[:, 1:4]), want,
                "non-contiguous inputs")
    # gat_attention is the composition of the two ops
    v = torch.from_numpy(np.random.default_rng(2).uniform(-1, 1, size=(K, 3, 4))).float().to(dev)
    out, attn = flow_spmm.gat_attention(d_rp, d_ci, d_sr, d_sc, v, return_attention=True)
    assert_same(attn, want, "gat_attention's weights")
    assert_same(out, flow_spmm.spmm(d_rp, d_ci, got, rp.numel() - 1, K, v), "gat_attention")
    out1 = flow_spmm.gat_attention(d_rp, d_ci, d_sr[:, 1], d_sc[:, 1], v[:, 1, :], 0.2)
    assert_same(out1, out[:, 1, :], "gat_attention with 1-D scores")


def check_grads(dev, heads, dtype, col_range=None):
    """s_row.grad and s_col.grad of gat_softmax against the reference chain, bit for bit: the
    existing kCPU edge softmax and ref_backward for de, numpy for ds and d_row, grad_b_heads on
    host tensors for d_col."""
    rp, ci, s_row, s_col, g = problem([3, 1, 0, 5, 2, 12, 4, 1, 7, 600, 33, 64, 130], heads, dtype,
                                      seed=21, col_range=col_range)
    m = rp.numel() - 1
    e, z = ref_scores(rp, ci, s_row, s_col, 0.2)
    y = hc.run_forward(rp, e, m)
    want_ds, want_d_row = ref_grad(rp, ci, y, g, z, 0.2)
    want_d_col = autograd.TRANSPOSE_CACHE.grad_b_heads(rp, ci, want_ds, m, K,
                                                       torch.ones_like(s_row))
    d_rp, d_ci, d_g = to_dev(dev, rp, ci, g)
    a, b = (t.clone().to(dev).requires_grad_(True) for t in (s_row, s_col))
    attn = flow_spmm.gat_softmax(d_rp, d_ci, a, b)
    assert_same(attn, y, "forward under autograd")
    attn.backward(d_g)
    assert_same(a.grad, want_d_row, f"s_row.grad H={heads} {dtype}")
    assert_same(b.grad, want_d_col, f"s_col.grad H={heads} {dtype}")


def check_needs_input_grad(dev):
    """Only the gradients that are asked for are computed, with the full backward's bits; no
    transpose is built when only s_row needs one."""
    rp, ci, s_row, s_col, g = problem([3, 1, 0, 5, 2, 12, 4, 1, 7, 600], 3, torch.float32, seed=22)
    d_rp, d_ci, d_g = to_dev(dev, rp.clone(), ci.clone(), g)  # a CSR the cache has not met
    full = tuple(t.clone().to(dev).requires_grad_(True) for t in (s_row, s_col))
    only_row = s_row.clone().to(dev).requires_grad_(True)
    before = len(autograd.TRANSPOSE_CACHE.entries)
    keys = set(autograd.TRANSPOSE_CACHE.entries)
    flow_spmm.gat_softmax(d_rp, d_ci, only_row, s_col.to(dev)).backward(d_g)
    assert set(autograd.TRANSPOSE_CACHE.entries) == keys and \
        len(autograd.TRANSPOSE_CACHE.entries) == before, "s_row alone built a transpose"
    flow_spmm.gat_softmax(d_rp, d_ci, *full).backward(d_g)
    assert set(autograd.TRANSPOSE_CACHE.entries) != keys, "s_col's gradient goes through A^T"
    assert_same(only_row.grad, full[0].grad, "d(s_row) alone")
    only_col = s_col.clone().to(dev).requires_grad_(True)
    flow_spmm.gat_softmax(d_rp, d_ci, s_row.to(dev), only_col).backward(d_g)
    assert_same(only_col.grad, full[1].grad, "d(s_col) alone")


def check_gradcheck(dev):
    """torch.autograd.gradcheck in f64 at torch's default tolerances.  The inputs are multiples of
    1/4 (s_row) and multiples of 1/4 plus 1/8 (s_col), so every |z| >= 1/8 and no probe (eps =
    1e-6) crosses LeakyReLU's kink: a condition on the inputs, not a tolerance."""
    rng = np.random.default_rng(3)
    lens = [3, 1, 0, 5, 2, 12, 9]
    rp, _ = hc.csr_of(lens, torch.int32)
    ci = torch.from_numpy(rng.integers(0, 6, size=int(rp[-1]))).int()
    s_row = torch.from_numpy(rng.integers(-8, 9, size=(len(lens), 2)) / 4.0)
    s_col = torch.from_numpy(rng.integers(-8, 9, size=(6, 2)) / 4.0 + 0.125)
    d_rp, d_ci = to_dev(dev, rp, ci)
    a, b = (t.to(dev).requires_grad_(True) for t in (s_row, s_col))
    assert torch.autograd.gradcheck(lambda x, y: flow_spmm.gat_softmax(d_rp, d_ci, x, y), (a, b))
    assert torch.autograd.gradcheck(lambda x, y: flow_spmm.gat_softmax(d_rp, d_ci, x, y, 0.01),
                                    (a, b))


def check_dense_reference_f32(dev, h=3, d=5):
    """gat_attention in f32 against a dense float64 GAT layer: output and the three gradients
    within atol = 1e-5, the tolerance graph_attention_cases.check_dense_reference_f32 uses
    (everything after the scores is the same arithmetic)."""
    from edge_softmax_cases import attention_problem
    rp, ci, _, _, _ = attention_problem(torch.float64)
    m = rp.numel() - 1
    rng = np.random.default_rng(12)
    s_row, s_col = (torch.from_numpy(rng.uniform(-2, 2, size=(12, h))) for _ in range(2))
    v, w = (torch.from_numpy(rng.uniform(-1, 1, size=(12, h, d))) for _ in range(2))
    dense = tuple(t.clone().requires_grad_(True) for t in (s_row, s_col, v))
    rows = torch.repeat_interleave(torch.arange(m), torch.diff(rp.long()))
    mask = torch.zeros((m, 12), dtype=torch.bool)
    mask[rows, ci.long()] = True
    z = dense[0][:, None, :] + dense[1][None, :, :]                       # [M, K, H]
    s = torch.nn.functional.leaky_relu(z, 0.2).masked_fill(~mask[:, :, None], float("-inf"))
    p = torch.where(mask[:, :, None], torch.softmax(s, dim=1), torch.zeros_like(s))
    ref = torch.einsum("mkh,khd->mhd", p, dense[2])
    (ref * w).sum().backward()
    d_rp, d_ci = to_dev(dev, rp, ci)
    ours = tuple(t.float().to(dev).requires_grad_(True) for t in (s_row, s_col, v))
    out = flow_spmm.gat_attention(d_rp, d_ci, *ours)
    assert tuple(out.shape) == (m, h, d)
    torch.testing.assert_close(out.detach().cpu().double(), ref.detach(), rtol=0, atol=1e-5)
    (out * w.float().to(dev)).sum().backward()
    for name, x, y in zip(("s_row", "s_col", "v"), ours, dense):
        torch.testing.assert_close(x.grad.cpu().double(), y.grad, rtol=0, atol=1e-5,
                                   msg=lambda s, n=name: f"d({n}): {s}")


def check_threads_do_not_matter():
    """The kCPU result does not depend on num_threads."""
    rp, ci, s_row, s_col, g = problem(hc.BOUNDARY, 5, torch.float32, m=60, seed=9)
    outs = []
    for threads in (1, 3, 8):
        y = run_forward(rp, ci, s_row, s_col, 0.2, threads=threads)
        outs.append((y, *run_backward(rp, ci, s_row, s_col, 0.2, y, g, threads=threads)))
    for got in outs[1:]:
        for name, x, want in zip(("attn", "ds", "d_row"), got, outs[0]):
            assert_same(x, want, f"{name} across thread counts")

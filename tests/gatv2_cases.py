"""The checks of the GATv2 attention scores (ops "gatv2_scores_csr_heads" and its gradient), written
once for both devices (test_gatv2_cpu.py runs them on host tensors, test_gatv2_gpu.py on the GPU,
where every result is also compared with the kCPU entry's bits).  Every comparison is bit for bit
unless it says otherwise.

The reference is never the code under test.  The contract's per-nonzero tensors are restated in
vectorised numpy (U = the activated sum, T1 and T2 = the gradient's terms, each rounded to T with
reduce_helpers.store) and fed to EXISTING kCPU entries on the CSR (row_ptr, arange(nnz)):
ops.sddmm_csr_heads with a = att repeated per row and b = U for the scores, ops.spmm_csr_heads with
values of ones and b = T1 / T2 for d_x / p, ops.relu_bias_grad for d(att), and the same chain on the
oracle's transpose for d(x_col)."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch

import oneflow_spmm as flow_spmm
from edge_softmax_helpers import tree_sum
from gat_softmax_cases import tensor_of
from heads_cases import SCHEDULES, opts_of
from helpers import DTYPES, random_dense
from oneflow_spmm import _C, _lib, autograd, ops
from oneflow_spmm._C import current_stream_handle
from oneflow_spmm._lib import LIB, check
from reduce_helpers import (PAD, acc, assert_same, is_sentinel, options, padded, sentinel, store,
                            transpose_t)

K = 37  # columns: far fewer than the nonzeros of the long rows, so columns repeat within a row
M = 40
# LG batches, the 256-nonzero item cut, the default hub split of 512 at D = 16, short rows under
# split=8 / chunk=4 / chunk=8 / ordered
LENGTHS = [0, 1, 2, 7, 8, 9, 63, 64, 65, 130, 255, 256, 257, 513, 1030]
SHORT = [0, 1, 2, 7, 8, 9, 17, 33, 65, 130]  # the gradient's wide shapes: every schedule, few nonzeros
SLOPES = [0.2, 1.0, 0.01]
# one per LG x L configuration of the forward's fast path; (16, 64), (8, 256): the 16-bit types only
FAST_HD = [(1, 8), (2, 8), (4, 8), (8, 8), (8, 16), (8, 32), (8, 64), (16, 64), (8, 256)]
GENERAL_HD = [(3, 5), (5, 1), (2, 12), (2, 24)]  # D / 8 = 3 is not a power of two


def fwd_cases(hds):
    return [(h, d, dt) for (h, d) in hds for dt in ("f32", "f64", "bf16", "f16")
            if h * d <= 512 or dt in ("bf16", "f16")]


# the gradient's N = H * D: every LPR (1, 4, 16, 32, 64) and a second column tile
GRAD_HD = {"f32": [(1, 4), (2, 8), (4, 16), (8, 16), (8, 32), (8, 64)],           # N = 4 .. 512
           "f64": [(1, 2), (4, 8), (8, 16), (8, 32)],                              # N = 2 .. 256
           "bf16": [(1, 8), (4, 8), (8, 16), (8, 32), (8, 64), (16, 64)],          # N = 8 .. 1024
           "f16": [(1, 8), (8, 16), (16, 64)]}
GRAD_GENERAL_HD = [(3, 5), (5, 1), (2, 12)]  # odd D, D < VEC: the general path


def to_dev(dev, *ts):
    return tuple(t.to(dev) if t is not None else None for t in ts)


@functools.lru_cache(maxsize=None)
def problem(h, d, dt, it="i32", lengths=None, m=M, seed=0, col_range=None, exact=False, k=K):
    """(rp, ci, x_row [M, H*D], x_col [K, H*D], att [H*D], de [nnz, H]) on the host; shared, never
    written.  Columns are drawn with repetition from [0, k), or from col_range = (lo, hi)."""
    rng = np.random.default_rng(seed + 1000 * h + d)
    dtype, idt = DTYPES[dt], torch.int32 if it == "i32" else torch.int64
    base = list(lengths) if lengths is not None else LENGTHS
    lens = np.array([base[i % len(base)] for i in range(max(m, len(base)))])
    if lengths is None:  # every boundary length once, short rows for the rest
        lens[len(base):] = [base[i % 10] for i in range(len(lens) - len(base))]
    rng.shuffle(lens)
    rp = np.zeros(len(lens) + 1, dtype=np.int64)
    rp[1:] = np.cumsum(lens)
    lo, hi = col_range if col_range is not None else (0, k)
    ci = torch.from_numpy(rng.integers(lo, hi, size=int(rp[-1]))).to(idt)
    x_row = random_dense(len(lens), h * d, rng, dtype, exact)
    x_col = random_dense(k, h * d, rng, dtype, exact)
    att = random_dense(1, h * d, rng, dtype, exact)[0].contiguous()
    de = random_dense(int(rp[-1]), h, rng, dtype, exact)
    return torch.from_numpy(rp).to(idt), ci, x_row, x_col, att, de


# ---- the contract's steps 1-3 in numpy --------------------------------------------------------------
def ref_terms(rp, ci, x_row, x_col, att, slope, heads, de=None):
    """(U [nnz, N], T1, T2) as torch tensors of the storage type; T1 = T2 = None without de."""
    dtype = x_row.dtype
    A = np.float64 if dtype == torch.float64 else np.float32
    rpn = rp.numpy().astype(np.int64)
    rows = np.repeat(np.arange(len(rpn) - 1), np.diff(rpn))
    c = ci.numpy().astype(np.int64)
    k, n = x_col.shape
    ok = (c >= 0) & (c < k)
    gathered = np.zeros((len(c), n), dtype=A)  # a column outside [0, K) reads +0
    gathered[ok] = acc(x_col).astype(A)[c[ok]]
    with np.errstate(invalid="ignore", over="ignore"):
        z = (acc(x_row).astype(A)[rows] + gathered).astype(A)
        u = np.where(z > 0, z, (z * A(slope)).astype(A))
        U = tensor_of(store(u, dtype), dtype)
        if de is None:
            return U, None, None
        w_pos = acc(att).astype(A)
        w_neg = (w_pos * A(slope)).astype(A)
        g = np.repeat(acc(de).astype(A), n // heads, axis=1)
        T1 = tensor_of(store((g * np.where(z > 0, w_pos[None, :], w_neg[None, :])).astype(A), dtype),
                       dtype)
        T2 = tensor_of(store((g * acc(U).astype(A)).astype(A), dtype), dtype)
    return U, T1, T2


def _identity_csr(rp, nnz):
    return rp, torch.arange(nnz, dtype=rp.dtype)


def ref_scores(rp, ci, x_row, x_col, att, slope, heads):
    """The existing kCPU multi-head SDDMM on (rp, arange(nnz)) with a = att per row and b = U."""
    m, nnz = rp.numel() - 1, ci.numel()
    U, _, _ = ref_terms(rp, ci, x_row, x_col, att, slope, heads)
    if nnz == 0:
        return torch.empty((0, heads), dtype=x_row.dtype)
    a = att[None, :].repeat(m, 1).contiguous()
    return ops.sddmm_csr_heads(*_identity_csr(rp, nnz), a, U, m, nnz, heads)


def ref_grad(rp, ci, x_row, x_col, att, slope, heads, de, opts=None):
    """(d_x, p) by the existing kCPU multi-head SpMM on (rp, arange(nnz)) with ones and T1 / T2."""
    m, nnz = rp.numel() - 1, ci.numel()
    _, T1, T2 = ref_terms(rp, ci, x_row, x_col, att, slope, heads, de)
    ones = torch.ones((nnz, heads), dtype=x_row.dtype)
    ident = _identity_csr(rp, nnz)
    return tuple(ops.spmm_csr_heads(*ident, ones, t, m, nnz, heads, options=opts) for t in (T1, T2))


def ref_d_att(p):
    return ops.relu_bias_grad(None, p, relu=False, bias_grad=True)[1]


def ref_d_col(rp, ci, x_row, x_col, att, slope, heads, de):
    """The same chain on the oracle's transpose: rows are A^T's, x_row and x_col swapped, de gathered
    by perm."""
    rp_t, ci_t, perm = transpose_t(rp, ci, x_col.shape[0])
    return ref_grad(rp_t, ci_t, x_col, x_row, att, slope, heads,
                    de.index_select(0, perm.long()).contiguous())[0]


# ---- checks ----------------------------------------------------------------------------------------
def run_scores(dev, rp, ci, x_row, x_col, att, slope, heads, pad=0, shift=0, **kw):
    d = to_dev(dev, rp, ci, x_row, x_col, att)
    xr, xc = padded(d[2], pad, shift), padded(d[3], pad, shift)
    w = padded(d[4][None, :], 0, shift)[0]
    return ops.gatv2_scores_csr_heads(d[0], d[1], xr, xc, w, rp.numel() - 1, x_col.shape[0], heads,
                                      slope, **kw)


def run_grad(dev, rp, ci, x_row, x_col, att, slope, heads, de, pad=0, shift=0, with_att=True, **kw):
    d = to_dev(dev, rp, ci, x_row, x_col, att, de)
    m, n = x_row.shape
    xr, xc = padded(d[2], pad, shift), padded(d[3], pad, shift)
    w = padded(d[4][None, :], 0, shift)[0]
    d_x = padded(sentinel((m, n), x_row.dtype, dev), pad, shift)
    p = padded(sentinel((m, n), x_row.dtype, dev), pad, shift) if with_att else None
    ops.gatv2_scores_csr_heads_grad(d[0], d[1], xr, xc, w, d[5], rp.numel() - 1, x_col.shape[0],
                                    heads, slope, with_att=with_att, d_x=d_x, p=p, **kw)
    for t in (d_x, p):
        if pad and t is not None:
            assert bool(is_sentinel(t._base[shift:].view(m, n + pad)[:, n:]).all()), \
                "wrote into the padding"
    return d_x, p


def check_forward(dev, h, d, dt, it="i32", slope=0.2, **kw):
    """The scores against the reference chain and, on the GPU, the kCPU entry; one element off the
    alignment and a padded leading dimension give the aligned bits."""
    rp, ci, x_row, x_col, att, _ = p = problem(h, d, dt, it, **kw)
    what = f"scores H={h} D={d} {dt} {it} slope={slope}"
    want = ref_scores(rp, ci, x_row, x_col, att, slope, h)
    got = run_scores(dev, *p[:5], slope, h)
    assert_same(got, want, f"{what} vs sddmm_csr_heads on the numpy U")
    if dev != "cpu":
        assert_same(got, run_scores("cpu", *p[:5], slope, h), f"{what} vs kCPU")
    assert_same(run_scores(dev, *p[:5], slope, h, pad=PAD, shift=1), want, f"{what} unaligned")
    return got


def check_grad(dev, h, d, dt, it="i32", slope=0.2, schedules=SCHEDULES, unaligned=True, **kw):
    """d_x and p against the reference chain under every schedule, with_att on and off."""
    rp, ci, x_row, x_col, att, de = p = problem(h, d, dt, it, **kw)
    for name in schedules:
        o = opts_of(name)
        what = f"grad H={h} D={d} {dt} {it} {name}"
        want_dx, want_p = ref_grad(rp, ci, x_row, x_col, att, slope, h, de, o)
        d_x, pp = run_grad(dev, *p[:5], slope, h, de, options=o)
        assert_same(d_x, want_dx, f"{what} d_x vs spmm_csr_heads on the numpy T1")
        assert_same(pp, want_p, f"{what} p vs spmm_csr_heads on the numpy T2")
        only, none = run_grad(dev, *p[:5], slope, h, de, with_att=False, options=o)
        assert none is None
        assert_same(only, want_dx, f"{what} d_x without p")
        if dev != "cpu":
            k_dx, k_p = run_grad("cpu", *p[:5], slope, h, de, options=o)
            assert_same(d_x, k_dx, f"{what} d_x vs kCPU")
            assert_same(pp, k_p, f"{what} p vs kCPU")
    if unaligned:
        u_dx, u_p = run_grad(dev, *p[:5], slope, h, de, pad=PAD, shift=1)
        w_dx, w_p = ref_grad(rp, ci, x_row, x_col, att, slope, h, de)
        assert_same(u_dx, w_dx, f"grad H={h} D={d} {dt} unaligned d_x")
        assert_same(u_p, w_p, f"grad H={h} D={d} {dt} unaligned p")


def check_tree_sum(dev, dt):
    """Small cases, per nonzero and head: edge_softmax_helpers.tree_sum over the numpy products."""
    for h, d in ((2, 8), (3, 5), (2, 24), (1, 64)):
        rp, ci, x_row, x_col, att, _ = p = problem(h, d, dt, lengths=(0, 1, 3, 9), m=4, seed=3)
        U, _, _ = ref_terms(rp, ci, x_row, x_col, att, 0.2, h)
        A = np.float64 if x_row.dtype == torch.float64 else np.float32
        prod = (acc(att).astype(A)[None, :] * acc(U).astype(A)).astype(A)
        want = np.array([[tree_sum(prod[j, i * d:(i + 1) * d]) for i in range(h)]
                         for j in range(ci.numel())], dtype=A)
        assert_same(run_scores(dev, *p[:5], 0.2, h), tensor_of(store(want, x_row.dtype), x_row.dtype),
                    f"tree_sum H={h} D={d} {dt}")


def check_sddmm_identity(dev, dt):
    """x_row = +0 and x_col > 0: the activation is the identity, so the scores are
    sddmm_csr_heads(rp, ci, att repeated, x_col)."""
    for h, d in ((8, 16), (3, 5)):
        rp, ci, x_row, x_col, att, _ = problem(h, d, dt, seed=4)
        m = rp.numel() - 1
        zero, pos = torch.zeros_like(x_row), x_col.abs() + 1
        got = run_scores(dev, rp, ci, zero, pos, att, 0.2, h)
        a = att[None, :].repeat(m, 1).contiguous()
        d_rp, d_ci, d_a, d_pos = to_dev(dev, rp, ci, a, pos)
        assert_same(got, ops.sddmm_csr_heads(d_rp, d_ci, d_a, d_pos, m, K, h), f"identity H={h} {dt}")


def check_row_ranges(dev, h, d, dt):
    """A range reads x_row and writes d_x / p from row_begin on, and writes exactly its own
    nonzeros of e; sentinels around stay untouched."""
    rp, ci, x_row, x_col, att, de = problem(h, d, dt)
    m, n, nnz = rp.numel() - 1, h * d, ci.numel()
    o = opts_of("split8_chunk4")
    full = ref_scores(rp, ci, x_row, x_col, att, 0.2, h)
    full_dx, full_p = ref_grad(rp, ci, x_row, x_col, att, 0.2, h, de, o)
    d_rp, d_ci, d_xr, d_xc, d_att, d_de = to_dev(dev, rp, ci, x_row, x_col, att, de)
    rpn = rp.numpy().astype(np.int64)
    for lo, hi in ((1, m - 1), (3, 4), (2, 9), (5, 5), (0, 0), (m, m), (0, m)):
        j0, j1 = int(rpn[lo]), int(rpn[hi])
        e = sentinel((nnz, h), x_row.dtype, dev)
        ops.gatv2_scores_csr_heads(d_rp, d_ci, d_xr[lo:], d_xc, d_att, m, K, h, 0.2, out=e,
                                   row_begin=lo, row_end=hi)
        assert_same(e[j0:j1], full[j0:j1], f"e rows [{lo}, {hi})")
        kept = is_sentinel(e)
        assert bool(kept[:j0].all()) and bool(kept[j1:].all()), f"e rows [{lo}, {hi}): wrote outside"
        bufs = [sentinel((m + 2, n + PAD), x_row.dtype, dev) for _ in range(2)]
        outs = [b[1:1 + m - lo, :n] for b in bufs]
        ops.gatv2_scores_csr_heads_grad(d_rp, d_ci, d_xr[lo:], d_xc, d_att, d_de, m, K, h, 0.2,
                                        d_x=outs[0], p=outs[1], row_begin=lo, row_end=hi, options=o)
        for name, buf, out, want in (("d_x", bufs[0], outs[0], full_dx), ("p", bufs[1], outs[1], full_p)):
            assert_same(out[:hi - lo], want[lo:hi], f"{name} rows [{lo}, {hi})")
            kept = is_sentinel(buf)
            kept[1:1 + hi - lo, :n] = True
            assert bool(kept.all()), f"{name} rows [{lo}, {hi}): wrote outside its rows"


def check_columns_out_of_range(dev, dt):
    """Columns outside [0, K) read x_col = +0: negative ones in the forward, those >= K in both."""
    for h, d in ((8, 8), (3, 5)):
        p = problem(h, d, dt, lengths=(0, 1, 7, 9, 33, 65, 129, 300), m=8, seed=5,
                    col_range=(-5, 2 * K))
        assert int((p[1] >= K).sum()) > 0 and int((p[1] < 0).sum()) > 0
        check_forward(dev, h, d, dt, lengths=(0, 1, 7, 9, 33, 65, 129, 300), m=8, seed=5,
                      col_range=(-5, 2 * K))
        check_grad(dev, h, d, dt, lengths=(0, 1, 7, 9, 33, 65, 129, 300), m=8, seed=6,
                   col_range=(0, 2 * K), schedules=("default", "split8_chunk4"))


def check_activation_edges(dev, dtype, slope):
    """Exact inputs at the activation's edges, one row each, D = 2 with att = (1, 1/2): z = +0,
    z = -0, cancellation, the smallest negative z, and sums that T cannot hold (257 in bf16, 2049 in
    f16).  Forward and gradient against the reference chain."""
    tiny = {torch.float32: 2.0 ** -149, torch.float64: 5e-324, torch.bfloat16: 2.0 ** -133,
            torch.float16: 2.0 ** -24}[dtype]
    big = {torch.bfloat16: 256.0, torch.float16: 2048.0}.get(dtype, 4.0)
    rows = [(0.0, [0.0, 1.0, -2.0]), (-0.0, [-0.0, 1.0, -2.0]), (3.0, [-3.0, -3.0, 1.0]),
            (-tiny, [0.0, tiny, -tiny]), (big, [1.0, 0.0]), (-big, [-1.0, 0.0, 1.0])]
    heads, d = 2, 2
    lens = [len(c) for _, c in rows]
    rp = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
    key = lambda v: (float(v), bool(np.signbit(v)))  # noqa: E731  (+0 and -0 are two columns)
    cols = sorted({key(v) for _, c in rows for v in c})
    col_of = {kv: i for i, kv in enumerate(cols)}
    cols = [-0.0 if neg and v == 0 else v for v, neg in cols]
    ci = torch.tensor([col_of[key(v)] for _, c in rows for v in c], dtype=torch.int32)
    f64 = np.float64 if dtype == torch.float64 else np.float32
    mk = lambda vals: torch.from_numpy(np.array(vals, dtype=f64)).to(dtype)  # noqa: E731
    x_row = mk([[r] * (heads * d) for r, _ in rows])
    x_col = mk([[v] * (heads * d) for v in cols])
    att = mk([1.0, 0.5, -1.0, 2.0])
    de = mk(np.random.default_rng(4).integers(-2, 3, size=(ci.numel(), heads)).astype(f64))
    assert x_row[3, 0].item() == -tiny and bool(np.signbit(x_row[1, 0].item()))
    what = f"activation edges {dtype} slope {slope}"
    want = ref_scores(rp, ci, x_row, x_col, att, slope, heads)
    assert_same(run_scores(dev, rp, ci, x_row, x_col, att, slope, heads), want, what)
    if dtype in (torch.bfloat16, torch.float16):
        j = int(rp[4])  # big + 1 is rounded to T before the dot product: it ties with big
        assert want[j, 0].item() == want[j + 1, 0].item() == 1.5 * big
    w_dx, w_p = ref_grad(rp, ci, x_row, x_col, att, slope, heads, de)
    d_x, p = run_grad(dev, rp, ci, x_row, x_col, att, slope, heads, de)
    assert_same(d_x, w_dx, f"{what} d_x")
    assert_same(p, w_p, f"{what} p")
    if slope == 1.0:  # the identity activation: the SDDMM on the rounded z
        z = tensor_of(store(acc(x_row)[np.repeat(np.arange(len(rows)), lens)] +
                            acc(x_col)[ci.numpy()], dtype), dtype)
        a = att[None, :].repeat(len(rows), 1).contiguous()
        assert_same(want, ops.sddmm_csr_heads(rp, torch.arange(ci.numel(), dtype=torch.int32), a, z,
                                              len(rows), ci.numel(), heads), "slope 1 vs sddmm on z")


def check_special_confined(dev, dt):
    """A NaN / +inf / -inf in one head of one row's x_row stays in that head's scores of that row
    (where -inf meets att = 0 IEEE decides: confinement only is asserted)."""
    for h, d in ((8, 8), (3, 5)):
        rp, ci, x_row, x_col, att, _ = problem(h, d, dt, lengths=(3, 11, 0, 70, 5, 300), m=6, seed=7)
        x_row, att = x_row.clone(), att.clone()
        att[(4 % h) * d + d // 2] = 0.0  # meets row 4's -inf: 0 * -inf
        marks = {1: float("nan"), 3: float("inf"), 4: float("-inf")}
        for r, v in marks.items():
            x_row[r, (r % h) * d + (d // 2)] = v
        e = run_scores(dev, rp, ci, x_row, x_col, att, 0.2, h).cpu().double()
        clean = run_scores(dev, *problem(h, d, dt, lengths=(3, 11, 0, 70, 5, 300), m=6, seed=7)[:2],
                           x_row.nan_to_num(0.0, 0.0, 0.0), x_col, att, 0.2, h).cpu().double()
        rpn = rp.numpy()
        for r in range(6):
            j0, j1 = int(rpn[r]), int(rpn[r + 1])
            for i in range(h):
                if r in marks and i == r % h:
                    assert not bool(torch.isfinite(e[j0:j1, i]).any()), f"row {r} head {i}"
                else:
                    assert bool(torch.equal(e[j0:j1, i], clean[j0:j1, i])), \
                        f"row {r} head {i}: a special value leaked"


def check_degenerate(dev, dt):
    """H == 0, nnz == 0 and an empty range write nothing (the gradient's +0 rows excepted); H = 1
    through the 2-D public form."""
    dtype = DTYPES[dt]
    rp, ci, x_row, x_col, att, de = problem(1, 16, dt, seed=8)
    d_rp, d_ci, d_xr, d_xc, d_att, d_de = to_dev(dev, rp, ci, x_row, x_col, att, de)
    m, nnz = rp.numel() - 1, ci.numel()
    want = ref_scores(rp, ci, x_row, x_col, att, 0.2, 1)
    flat = flow_spmm.gatv2_scores(d_rp, d_ci, d_xr, d_xc, d_att)
    assert tuple(flat.shape) == (nnz,)
    assert_same(flat, want[:, 0], "H = 1 through the 2-D public form")
    none_m, none_k = (torch.empty((r, 0), dtype=dtype, device=dev) for r in (m, K))
    none_w = torch.empty((0,), dtype=dtype, device=dev)
    assert ops.gatv2_scores_csr_heads(d_rp, d_ci, none_m, none_k, none_w, m, K, 0).shape == (nnz, 0)
    rp0 = torch.zeros(4, dtype=torch.int32, device=dev)
    e0 = ops.gatv2_scores_csr_heads(rp0, rp0[:0], d_xr[:3], d_xc, d_att, 3, K, 1)
    assert tuple(e0.shape) == (0, 1)
    d_x0, p0 = ops.gatv2_scores_csr_heads_grad(rp0, rp0[:0], d_xr[:3], d_xc, d_att, d_de[:0], 3, K, 1,
                                               d_x=sentinel((3, 16), dtype, dev),
                                               p=sentinel((3, 16), dtype, dev))
    assert not bool(d_x0.any()) and not bool(p0.any()), "nnz == 0: every row is +0"
    part = sentinel((nnz, 1), dtype, dev)
    ops.gatv2_scores_csr_heads(d_rp, d_ci, d_xr[2:], d_xc, d_att, m, K, 1, out=part, row_begin=2,
                               row_end=2)
    assert bool(is_sentinel(part).all()), "an empty range writes nothing"
    d_xe = sentinel((m, 16), dtype, dev)
    ops.gatv2_scores_csr_heads_grad(d_rp, d_ci, d_xr[2:], d_xc, d_att, d_de, m, K, 1, d_x=d_xe,
                                    with_att=False, row_begin=2, row_end=2)
    assert bool(is_sentinel(d_xe).all()), "an empty range writes nothing (gradient)"
    assert tuple(flow_spmm.gatv2_scores(rp0, rp0[:0], d_xr[:3], d_xc, d_att).shape) == (0,)
    a = d_xr[:3].clone().requires_grad_(True)
    flow_spmm.gatv2_scores(rp0, rp0[:0], a, d_xc, d_att).sum().backward()
    assert a.grad is not None and not bool(a.grad.any()), "nnz == 0: d(x_row) is +0"


def check_argument_checks(dev):
    """NULLs, overlaps, a bad slope, D > 2048, planned / variant on the gradient and a workspace that
    is too small return the documented code and launch nothing: the outputs keep their sentinels."""
    f32 = torch.float32
    rp = torch.tensor([0, 2, 3], dtype=torch.int32, device=dev)
    ci = torch.tensor([0, 1, 1], dtype=torch.int32, device=dev)
    x_row = torch.arange(8, dtype=f32, device=dev).view(2, 4) - 3
    x_col = torch.arange(8, dtype=f32, device=dev).view(2, 4) / 4 - 1
    att = torch.tensor([1.0, -1.0, 0.5, 2.0], device=dev)
    de = torch.ones((3, 2), device=dev)
    e, d_x, p = (sentinel(s, f32, dev) for s in ((3, 2), (2, 4), (2, 4)))
    I, F, EINVAL = _lib.DT_INT32, _lib.DT_FLOAT, _lib.OFX_EINVAL
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    if dev == "cpu":
        fwd = lambda *a: LIB.ofx_gatv2_scores_csr_heads_cpu(0, *a)  # noqa: E731
        bwd = lambda *a, o=None: LIB.ofx_gatv2_scores_csr_heads_grad_cpu(0, *a, o)  # noqa: E731
    else:
        s = current_stream_handle(de)
        fwd = lambda *a: LIB.ofx_gatv2_scores_csr_heads(s, *a, ws.data_ptr(), ws.numel())  # noqa: E731
        bwd = lambda *a, o=None: LIB.ofx_gatv2_scores_csr_heads_grad(  # noqa: E731
            s, *a, ws.data_ptr(), ws.numel(), o)
    ins = (rp.data_ptr(), ci.data_ptr(), x_row.data_ptr(), x_col.data_ptr(), att.data_ptr())

    def f(slope=0.2, h=2, d=2, nnz=3, q=ins, out=e.data_ptr(), rb=0, re=2, it=I, vt=F, k=2, ld=4):
        return fwd(it, vt, 2, k, h, d, nnz, q[0], q[1], q[2], ld, q[3], ld, q[4], slope, out, rb, re)

    def b(slope=0.2, h=2, d=2, nnz=3, q=ins, g=de.data_ptr(), out=d_x.data_ptr(), pp=p.data_ptr(),
          rb=0, re=2, it=I, vt=F, k=2, ld=4, o=None):
        return bwd(it, vt, 2, k, h, d, nnz, q[0], q[1], q[2], ld, q[3], ld, q[4], slope, g, out, ld,
                   pp, ld, rb, re, o=o)

    for call in (f, b):
        assert call(h=-1) == EINVAL and call(nnz=-3) == EINVAL and call(k=-1) == EINVAL
        assert call(rb=1, re=3) == EINVAL and call(rb=2, re=1) == EINVAL
        assert call(ld=3) == EINVAL
        for bad in (0.0, -0.2, float("nan"), float("inf"), 1e-60, 1e60):  # the slope, as f32
            assert call(slope=bad) == EINVAL, bad
        for i in range(5):
            assert call(q=ins[:i] + (None,) + ins[i + 1:]) == EINVAL, i
        assert call(out=None) == EINVAL
        for i in range(5):
            assert call(out=ins[i]) == EINVAL, i
        assert call(vt=_lib.DT_INT64) == _lib.OFX_EUNSUPPORTED
        assert call(it=F) == _lib.OFX_EUNSUPPORTED
        assert call(h=1, d=2049, ld=2049) == _lib.OFX_EUNSUPPORTED
        assert call(nnz=1 << 31) == EINVAL
        assert call(rb=1, re=1) == _lib.OFX_OK
    assert f(h=0, d=0) == _lib.OFX_OK
    assert b(g=None) == EINVAL and b(pp=d_x.data_ptr()) == EINVAL and b(out=de.data_ptr()) == EINVAL
    assert b(pp=att.data_ptr()) == EINVAL
    for bad in (options(planned=True), ops.make_options(variant=1)):
        assert b(o=ctypes.byref(bad)) == EINVAL
    broken = _lib.Options()
    broken.magic = 0
    assert b(o=ctypes.byref(broken)) == EINVAL
    # f64 keeps slopes that f32 cannot hold
    x64 = tuple(t.double() for t in (x_row, x_col, att))
    e64 = torch.empty((3, 2), dtype=torch.float64, device=dev)
    q64 = ins[:2] + tuple(t.data_ptr() for t in x64)
    assert f(slope=1e-60, vt=_lib.DT_DOUBLE, q=q64, out=e64.data_ptr()) == _lib.OFX_OK
    if dev != "cpu":  # a workspace one byte too small, or NULL, on a CSR whose rows need a plan
        rp2, ci2, xr2, xc2, w2, de2 = to_dev(dev, *problem(2, 8, "f32"))
        m2, nnz2 = rp2.numel() - 1, ci2.numel()
        e2, dx2, p2 = (sentinel(sh, f32, dev) for sh in ((nnz2, 2), (m2, 16), (m2, 16)))
        s = current_stream_handle(de)
        body = (I, F, m2, K, 2, 8, nnz2, rp2.data_ptr(), ci2.data_ptr(), xr2.data_ptr(), 16,
                xc2.data_ptr(), 16, w2.data_ptr(), 0.2)
        need = ctypes.c_size_t(0)
        check(LIB.ofx_gatv2_scores_csr_heads_workspace_size(I, F, m2, 2, 8, nnz2,
                                                            ctypes.byref(need)), "query")
        assert 0 < need.value <= ws.numel()
        for wptr, wsize in ((None, 0), (None, need.value), (ws.data_ptr(), need.value - 1)):
            assert LIB.ofx_gatv2_scores_csr_heads(s, *body, e2.data_ptr(), 0, m2, wptr, wsize) == \
                _lib.OFX_EWORKSPACE
        sizes = []
        for with_p, pp in ((1, p2.data_ptr()), (0, None)):
            check(LIB.ofx_gatv2_scores_csr_heads_grad_workspace_size(
                I, F, m2, K, 2, 8, nnz2, with_p, None, ctypes.byref(need)), "query")
            assert 0 < need.value <= ws.numel()
            sizes.append(need.value)
            assert LIB.ofx_gatv2_scores_csr_heads_grad(
                s, *body, de2.data_ptr(), dx2.data_ptr(), 16, pp, 16, 0, m2, ws.data_ptr(),
                need.value - 1, None) == _lib.OFX_EWORKSPACE
        assert sizes[0] > sizes[1], "p asks for a second plane of partials"
        torch.cuda.synchronize()
        assert all(bool(is_sentinel(t).all()) for t in (e2, dx2, p2)), "an error launched"
    assert all(bool(is_sentinel(t).all()) for t in (e, d_x, p)), "an error launched"
    size = ctypes.c_size_t(7)
    assert LIB.ofx_gatv2_scores_csr_heads_workspace_size(I, F, 2, 2, 2, 3, None) == EINVAL
    assert LIB.ofx_gatv2_scores_csr_heads_workspace_size(I, F, 2, -2, 2, 3, ctypes.byref(size)) == EINVAL
    assert LIB.ofx_gatv2_scores_csr_heads_grad_workspace_size(I, F, 2, 2, 2, 2, 3, 1, None, None) == EINVAL
    assert f() == _lib.OFX_OK and b() == _lib.OFX_OK
    if dev != "cpu":
        torch.cuda.synchronize()
    assert not any(bool(is_sentinel(t).any()) for t in (e, d_x, p))


def check_registrations():
    """Both ops for every dtype x index type x device, through the tmp-size query of the functional
    entries (inference and kernel choice; nothing is launched, the descriptors carry NULL): one
    kernel matches and its tmp size is the workspace query's."""
    m, k, nnz, heads, dd = 2, 4, 601, 2, 8
    n = heads * dd
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
                xr, xc, w, dy = d(vt, m, n), d(vt, k, n), d(vt, n), d(vt, nnz, heads)
                want = ctypes.c_size_t(5)
                check(LIB.ofx_gatv2_scores_csr_heads_workspace_size(it, vt, m, heads, dd, nnz,
                                                                    ctypes.byref(want)), "query")
                got = ctypes.c_size_t(1 << 40)
                check(LIB.ofx_functional_gatv2_scores_csr_heads(
                    None, rp, ci, xr, xc, w, heads, 0.2, None, None, 0, ctypes.byref(got)), "fwd")
                assert got.value == (want.value if dev == 0 else 0), (dev, vt, it)
                assert want.value > 0
                for with_att in (1, 0):
                    check(LIB.ofx_gatv2_scores_csr_heads_grad_workspace_size(
                        it, vt, m, k, heads, dd, nnz, with_att, None, ctypes.byref(want)), "query")
                    got = ctypes.c_size_t(1 << 40)
                    check(LIB.ofx_functional_gatv2_scores_csr_heads_grad(
                        None, rp, ci, xr, xc, w, dy, heads, 0.2, with_att, None, None, None, 0,
                        ctypes.byref(got)), "bwd")
                    assert got.value == (want.value if dev == 0 else 0), (dev, vt, it, with_att)


def check_sbp():
    """One all-broadcast signature each; the index inputs take no gradient."""
    for op, vals in (("gatv2_scores_csr_heads", ("x_row", "x_col", "att", "out")),
                     ("gatv2_scores_csr_heads_grad", ("x_row", "x_col", "att", "dy", "d_x", "p"))):
        s = _C.sbp_signatures(op)
        sigs, no_grad = s.split("|")
        assert len(sigs.split(";")) == 1, s
        want = {"a_csr_row_ptr:B", "a_csr_col_idx:B"} | {f"{v}:B" for v in vals}
        assert set(sigs.split(",")) == want, s
        assert set(no_grad.split(":")[1].split(",")) == {"a_csr_row_ptr", "a_csr_col_idx"}, s


def check_op_layer(dev):
    """Both ops through the registry dispatch against the C-ABI, for every dtype and index type, and
    the refusals of the Python layer and of the op's own inference."""
    for dt, it, h, d in (("f32", "i32", 4, 8), ("f64", "i64", 3, 5), ("bf16", "i32", 8, 16),
                         ("f16", "i64", 2, 12)):
        p = problem(h, d, dt, it, lengths=(3, 0, 9, 40, 600), m=5, seed=9)
        d_rp, d_ci, d_xr, d_xc, d_att, d_de = to_dev(dev, *p)
        m = d_rp.numel() - 1
        e = _C.gatv2_scores_csr_heads(d_rp, d_ci, d_xr, d_xc, d_att, h, 0.01)
        assert_same(e, ops.gatv2_scores_csr_heads(d_rp, d_ci, d_xr, d_xc, d_att, m, K, h, 0.01),
                    f"op vs C-ABI {dt} {it}")
        for with_att in (True, False):
            d_x, pp = _C.gatv2_scores_csr_heads_grad(d_rp, d_ci, d_xr, d_xc, d_att, d_de, h, 0.01,
                                                     with_att)
            w_dx, w_p = ops.gatv2_scores_csr_heads_grad(d_rp, d_ci, d_xr, d_xc, d_att, d_de, m, K, h,
                                                        0.01, with_att=with_att)
            assert_same(d_x, w_dx, f"grad op d_x vs C-ABI {dt} {it}")
            assert (pp is None and w_p is None) if not with_att else True
            if with_att:
                assert_same(pp, w_p, f"grad op p vs C-ABI {dt} {it}")
    with pytest.raises(RuntimeError, match="2-D"):
        _C.gatv2_scores_csr_heads(d_rp, d_ci, d_xr[:, 0].contiguous(), d_xc, d_att, h)
    with pytest.raises(RuntimeError, match="a_num_rows"):
        _C.gatv2_scores_csr_heads(d_rp, d_ci, d_xr[:-1], d_xc, d_att, h)
    with pytest.raises(RuntimeError, match="multiple"):
        _C.gatv2_scores_csr_heads(d_rp, d_ci, d_xr, d_xc, d_att, 5)
    with pytest.raises(RuntimeError, match="same number of columns"):
        _C.gatv2_scores_csr_heads(d_rp, d_ci, d_xr, d_xc, d_att[:-2], h)
    with pytest.raises(RuntimeError, match="nnz"):
        _C.gatv2_scores_csr_heads_grad(d_rp, d_ci, d_xr, d_xc, d_att, d_de[:-1], h)
    with pytest.raises(TypeError, match="dtype of a_csr_row_ptr"):
        _C.gatv2_scores_csr_heads(d_rp, d_ci.int(), d_xr, d_xc, d_att, h)
    with pytest.raises(TypeError, match="equal to x_col"):
        _C.gatv2_scores_csr_heads(d_rp, d_ci, d_xr.double(), d_xc, d_att, h)
    with pytest.raises(_lib.OfxError, match="negative_slope"):
        _C.gatv2_scores_csr_heads(d_rp, d_ci, d_xr, d_xc, d_att, h, 0.0)
    # the functional entry itself: the op's own inference refuses what the Python layer does
    byref = lambda *ts: [ctypes.byref(_C.desc(t)) for t in ts]  # noqa: E731
    size = ctypes.c_size_t(123)
    fwd = LIB.ofx_functional_gatv2_scores_csr_heads
    rc = fwd(None, *byref(d_rp, d_ci, d_xr, d_xc, d_att), 5, 0.2, None, None, 0, ctypes.byref(size))
    assert rc != 0 and b"multiple" in LIB.ofx_last_error()
    rc = fwd(None, *byref(d_rp, d_ci, d_xr[:-1].contiguous(), d_xc, d_att), h, 0.2, None, None, 0,
             ctypes.byref(size))
    assert rc != 0 and b"a_num_rows" in LIB.ofx_last_error()


def check_public_api(dev):
    """gatv2_scores on 2-D and 3-D inputs, out=, the error for out= under autograd, non-contiguous
    inputs; gatv2_softmax and gatv2_attention are the composition of the ops they call."""
    h, d = 3, 8
    rp, ci, x_row, x_col, att, _ = problem(h, d, "f32", lengths=(0, 1, 7, 9, 33, 65, 129, 600), m=8,
                                           seed=10)
    m, nnz = rp.numel() - 1, ci.numel()
    d_rp, d_ci, d_xr, d_xc, d_att = to_dev(dev, rp, ci, x_row, x_col, att)
    xr3, xc3, att2 = d_xr.view(m, h, d), d_xc.view(K, h, d), d_att.view(h, d)
    want = ref_scores(rp, ci, x_row, x_col, att, 0.2, h)
    got = flow_spmm.gatv2_scores(d_rp, d_ci, xr3, xc3, att2)
    assert_same(got, want, "3-D inputs, the default slope")
    assert_same(flow_spmm.gatv2_scores(d_rp, d_ci, xr3, xc3, att2, 0.01),
                ref_scores(rp, ci, x_row, x_col, att, 0.01, h), "negative_slope=0.01")
    flat = flow_spmm.gatv2_scores(d_rp, d_ci, xr3[:, 1], xc3[:, 1], att2[1])  # non-contiguous
    assert tuple(flat.shape) == (nnz,)
    want1 = ref_scores(rp, ci, x_row[:, d:2 * d].contiguous(), x_col[:, d:2 * d].contiguous(),
                       att[d:2 * d].contiguous(), 0.2, 1)[:, 0]
    assert_same(flat, want1, "2-D inputs")
    out = sentinel((nnz, h), got.dtype, dev)
    assert flow_spmm.gatv2_scores(d_rp, d_ci, xr3, xc3, att2, out=out) is out
    assert_same(out, want, "out=")
    out1 = sentinel((nnz,), got.dtype, dev)
    assert flow_spmm.gatv2_scores(d_rp, d_ci, xr3[:, 1], xc3[:, 1], att2[1], out=out1) is out1
    assert_same(out1, want1, "out= with 2-D inputs")
    a = xr3.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="out="):
        flow_spmm.gatv2_scores(d_rp, d_ci, a, xc3, att2, out=out)
    with pytest.raises(RuntimeError, match="out must be"):
        flow_spmm.gatv2_scores(d_rp, d_ci, xr3, xc3, att2, out=torch.empty_like(got).t().contiguous().t())
    with pytest.raises(RuntimeError, match="expected"):
        flow_spmm.gatv2_scores(d_rp, d_ci, xr3, xc3, d_att)
    with pytest.raises(RuntimeError, match="agree"):
        flow_spmm.gatv2_scores(d_rp, d_ci, xr3, xc3[:, :2], att2)
    wide = torch.zeros((m, h, d + 3), dtype=got.dtype, device=dev)
    wide[:, :, 1:d + 1] = xr3
    assert_same(flow_spmm.gatv2_scores(d_rp, d_ci, wide[:, :, 1:d + 1], xc3, att2), want,
                "non-contiguous inputs")
    w = flow_spmm.gatv2_softmax(d_rp, d_ci, xr3, xc3, att2)
    assert_same(w, flow_spmm.edge_softmax(d_rp, d_ci, got), "gatv2_softmax")
    res, attn = flow_spmm.gatv2_attention(d_rp, d_ci, xr3, xc3, att2, return_attention=True)
    assert_same(attn, w, "gatv2_attention's weights")
    assert_same(res, flow_spmm.spmm(d_rp, d_ci, w, m, K, xc3), "gatv2_attention, v = x_col")
    v = torch.from_numpy(np.random.default_rng(2).uniform(-1, 1, size=(K, h, 4))).float().to(dev)
    assert_same(flow_spmm.gatv2_attention(d_rp, d_ci, xr3, xc3, att2, v=v),
                flow_spmm.spmm(d_rp, d_ci, w, m, K, v), "gatv2_attention, v given")
    res1 = flow_spmm.gatv2_attention(d_rp, d_ci, xr3[:, 1], xc3[:, 1], att2[1])
    assert tuple(res1.shape) == (m, d)


def grad_case(dt, h, d, seed=11, col_range=None):
    return problem(h, d, dt, lengths=(3, 1, 0, 5, 2, 12, 4, 1, 7, 600, 33, 64, 130), m=13, seed=seed,
                   col_range=col_range)


def check_grads(dev, h, d, dt):
    """x_row.grad, x_col.grad and att.grad of gatv2_scores against the reference chain, bit for
    bit."""
    rp, ci, x_row, x_col, att, de = grad_case(dt, h, d)
    want_dx, want_p = ref_grad(rp, ci, x_row, x_col, att, 0.2, h, de)
    want_dc = ref_d_col(rp, ci, x_row, x_col, att, 0.2, h, de)
    d_rp, d_ci, d_de = to_dev(dev, rp, ci, de)
    m = rp.numel() - 1
    a, b, w = (t.clone().to(dev).requires_grad_(True)
               for t in (x_row.view(m, h, d), x_col.view(K, h, d), att.view(h, d)))
    e = flow_spmm.gatv2_scores(d_rp, d_ci, a, b, w)
    assert_same(e, ref_scores(rp, ci, x_row, x_col, att, 0.2, h), "forward under autograd")
    e.backward(d_de)
    assert_same(a.grad.view(m, h * d), want_dx, f"x_row.grad H={h} D={d} {dt}")
    assert_same(b.grad.view(K, h * d), want_dc, f"x_col.grad H={h} D={d} {dt}")
    assert_same(w.grad.view(h * d), ref_d_att(want_p), f"att.grad H={h} D={d} {dt}")


def check_needs_input_grad(dev, monkeypatch):
    """Only the gradients that are asked for are computed, with the full backward's bits: no
    transpose when only x_row / att need one, no p when att does not."""
    rp, ci, x_row, x_col, att, de = grad_case("f32", 3, 8, seed=12)
    d_rp, d_ci, d_de = to_dev(dev, rp.clone(), ci.clone(), de)  # a CSR the cache has not met
    full = tuple(t.clone().to(dev).requires_grad_(True) for t in (x_row, x_col, att))
    calls = []
    real = _C.gatv2_scores_csr_heads_grad
    monkeypatch.setattr(_C, "gatv2_scores_csr_heads_grad",
                        lambda *a, **kw: calls.append(kw.get("with_att")) or real(*a, **kw))

    def run(xr, xc, w):
        return autograd.Gatv2ScoresFunction.apply(d_rp, d_ci, xr, xc, w, 3, 0.2)

    keys = set(autograd.TRANSPOSE_CACHE.entries)
    only_row = x_row.clone().to(dev).requires_grad_(True)
    run(only_row, x_col.to(dev), att.to(dev)).backward(d_de)
    assert calls == [False], "x_row alone: one launch, without p"
    only_att = att.clone().to(dev).requires_grad_(True)
    run(x_row.to(dev), x_col.to(dev), only_att).backward(d_de)
    assert calls == [False, True]
    assert set(autograd.TRANSPOSE_CACHE.entries) == keys, "x_row / att alone built a transpose"
    run(*full).backward(d_de)
    assert calls[2:] == [True, False], "one launch on A with p, one on the transpose without"
    assert set(autograd.TRANSPOSE_CACHE.entries) != keys, "x_col's gradient goes through A^T"
    assert_same(only_row.grad, full[0].grad, "d(x_row) alone")
    assert_same(only_att.grad, full[2].grad, "d(att) alone")
    only_col = x_col.clone().to(dev).requires_grad_(True)
    del calls[:]
    run(x_row.to(dev), only_col, att.to(dev)).backward(d_de)
    assert calls == [False]
    assert_same(only_col.grad, full[1].grad, "d(x_col) alone")


def check_gradcheck(dev):
    """torch.autograd.gradcheck in f64 at torch's default tolerances.  x_row holds multiples of 1/4
    and x_col multiples of 1/4 plus 1/8, so every |z| >= 1/8 and no probe (eps = 1e-6) crosses
    LeakyReLU's kink: a condition on the inputs, not a tolerance."""
    rng = np.random.default_rng(3)
    lens = np.array([3, 1, 0, 5, 2, 12, 9])
    rp = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)])).int()
    ci = torch.from_numpy(rng.integers(0, 6, size=int(rp[-1]))).int()
    h, d = 2, 3
    x_row = torch.from_numpy(rng.integers(-8, 9, size=(len(lens), h, d)) / 4.0)
    x_col = torch.from_numpy(rng.integers(-8, 9, size=(6, h, d)) / 4.0 + 0.125)
    att = torch.from_numpy(rng.uniform(-1, 1, size=(h, d)))
    d_rp, d_ci = to_dev(dev, rp, ci)
    a, b, w = (t.to(dev).requires_grad_(True) for t in (x_row, x_col, att))
    for slope in (0.2, 0.01):
        assert torch.autograd.gradcheck(
            lambda x, y, z: flow_spmm.gatv2_scores(d_rp, d_ci, x, y, z, slope), (a, b, w))
    assert torch.autograd.gradcheck(
        lambda x, y, z: flow_spmm.gatv2_attention(d_rp, d_ci, x, y, z), (a, b, w))


def check_dense_reference_f32(dev, h=3, d=5):
    """gatv2_attention in f32 against a dense float64 GATv2 layer: output and the three gradients
    within atol = 1e-5, the tolerance gat_softmax_cases.check_dense_reference_f32 uses for the same
    downstream arithmetic (the score adds a D = 5 term sum of O(1) terms: a few f32 ulps)."""
    from edge_softmax_cases import attention_problem
    rp, ci, _, _, _ = attention_problem(torch.float64)
    m = rp.numel() - 1
    rng = np.random.default_rng(12)
    x_row, x_col = (torch.from_numpy(rng.uniform(-1, 1, size=(12, h, d))) for _ in range(2))
    att = torch.from_numpy(rng.uniform(-1, 1, size=(h, d)))
    w = torch.from_numpy(rng.uniform(-1, 1, size=(12, h, d)))
    dense = tuple(t.clone().requires_grad_(True) for t in (x_row, x_col, att))
    rows = torch.repeat_interleave(torch.arange(m), torch.diff(rp.long()))
    mask = torch.zeros((m, 12), dtype=torch.bool)
    mask[rows, ci.long()] = True
    z = dense[0][:, None] + dense[1][None, :]                                   # [M, K, H, D]
    s = (torch.nn.functional.leaky_relu(z, 0.2) * dense[2]).sum(-1)             # [M, K, H]
    s = s.masked_fill(~mask[:, :, None], float("-inf"))
    p = torch.where(mask[:, :, None], torch.softmax(s, dim=1), torch.zeros_like(s))
    ref = torch.einsum("mkh,khd->mhd", p, dense[1])
    (ref * w).sum().backward()
    d_rp, d_ci = to_dev(dev, rp, ci)
    ours = tuple(t.float().to(dev).requires_grad_(True) for t in (x_row, x_col, att))
    out = flow_spmm.gatv2_attention(d_rp, d_ci, *ours)
    assert tuple(out.shape) == (m, h, d)
    torch.testing.assert_close(out.detach().cpu().double(), ref.detach(), rtol=0, atol=1e-5)
    (out * w.float().to(dev)).sum().backward()
    for name, x, y in zip(("x_row", "x_col", "att"), ours, dense):
        torch.testing.assert_close(x.grad.cpu().double(), y.grad, rtol=0, atol=1e-5,
                                   msg=lambda s, n=name: f"d({n}): {s}")


def check_threads_do_not_matter():
    """The kCPU results do not depend on num_threads."""
    rp, ci, x_row, x_col, att, de = problem(5, 12, "f32", m=60, seed=13)
    m = rp.numel() - 1
    outs = []
    for threads in (1, 3, 8):
        e = ops.gatv2_scores_csr_heads(rp, ci, x_row, x_col, att, m, K, 5, num_threads=threads)
        outs.append((e, *ops.gatv2_scores_csr_heads_grad(rp, ci, x_row, x_col, att, de, m, K, 5,
                                                         num_threads=threads)))
    for got in outs[1:]:
        for name, x, want in zip(("e", "d_x", "p"), got, outs[0]):
            assert_same(x, want, f"{name} across thread counts")


def check_graph_capture(h, d, dt):
    """The forward and both gradient launches captured once and replayed on new inputs: the bits of
    the eager launches and of the kCPU entries."""
    dev = "cuda"
    first = problem(h, d, dt, seed=14)
    second = problem(h, d, dt, seed=15)
    rp, ci = first[0], first[1]
    m, n, nnz = rp.numel() - 1, h * d, ci.numel()
    rp_t, ci_t, perm = transpose_t(rp, ci, K)
    st = [t.clone().to(dev) for t in first[2:]]                 # x_row, x_col, att, de
    d_rp, d_ci, d_rp_t, d_ci_t, d_perm = to_dev(dev, rp, ci, rp_t, ci_t, perm.long())
    de_t = torch.empty_like(st[3])
    e = torch.empty((nnz, h), dtype=st[0].dtype, device=dev)
    d_x, p = (torch.empty((m, n), dtype=st[0].dtype, device=dev) for _ in range(2))
    d_c = torch.empty((K, n), dtype=st[0].dtype, device=dev)
    it, vt = _C.dtype_code(rp.dtype), _C.dtype_code(st[0].dtype)
    size = ctypes.c_size_t(0)
    check(LIB.ofx_gatv2_scores_csr_heads_workspace_size(it, vt, m, h, d, nnz, ctypes.byref(size)), "q")
    ws_f = torch.empty(max(size.value, 1), dtype=torch.uint8, device=dev)
    check(LIB.ofx_gatv2_scores_csr_heads_grad_workspace_size(it, vt, m, K, h, d, nnz, 1, None,
                                                             ctypes.byref(size)), "q")
    ws_g = torch.empty(max(size.value, 1), dtype=torch.uint8, device=dev)
    check(LIB.ofx_gatv2_scores_csr_heads_grad_workspace_size(it, vt, K, m, h, d, nnz, 0, None,
                                                             ctypes.byref(size)), "q")
    ws_t = torch.empty(max(size.value, 1), dtype=torch.uint8, device=dev)

    def launches():
        s = current_stream_handle(e)
        check(LIB.ofx_gatv2_scores_csr_heads(
            s, it, vt, m, K, h, d, nnz, d_rp.data_ptr(), d_ci.data_ptr(), st[0].data_ptr(), n,
            st[1].data_ptr(), n, st[2].data_ptr(), 0.2, e.data_ptr(), 0, m, ws_f.data_ptr(),
            ws_f.numel()), "fwd")
        check(LIB.ofx_gatv2_scores_csr_heads_grad(
            s, it, vt, m, K, h, d, nnz, d_rp.data_ptr(), d_ci.data_ptr(), st[0].data_ptr(), n,
            st[1].data_ptr(), n, st[2].data_ptr(), 0.2, st[3].data_ptr(), d_x.data_ptr(), n,
            p.data_ptr(), n, 0, m, ws_g.data_ptr(), ws_g.numel(), None), "grad")
        torch.index_select(st[3], 0, d_perm, out=de_t)
        check(LIB.ofx_gatv2_scores_csr_heads_grad(
            s, it, vt, K, m, h, d, nnz, d_rp_t.data_ptr(), d_ci_t.data_ptr(), st[1].data_ptr(), n,
            st[0].data_ptr(), n, st[2].data_ptr(), 0.2, de_t.data_ptr(), d_c.data_ptr(), n, None, n,
            0, K, ws_t.data_ptr(), ws_t.numel(), None), "grad on the transpose")

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launches()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launches()
    for t, src in zip(st, second[2:]):
        t.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    captured = [t.clone() for t in (e, d_x, p, d_c)]
    launches()
    torch.cuda.synchronize()
    x_row, x_col, att, de = second[2:]
    k_e = ops.gatv2_scores_csr_heads(rp, ci, x_row, x_col, att, m, K, h)
    k_dx, k_p = ops.gatv2_scores_csr_heads_grad(rp, ci, x_row, x_col, att, de, m, K, h)
    k_dc, _ = ops.gatv2_scores_csr_heads_grad(rp_t, ci_t, x_col, x_row, att,
                                              de.index_select(0, perm.long()).contiguous(), K, m, h,
                                              with_att=False)
    for name, got, eager, cpu in zip(("e", "d_x", "p", "d_x_col"), captured, (e, d_x, p, d_c),
                                     (k_e, k_dx, k_p, k_dc)):
        assert_same(got, eager, f"{name}: replay vs eager")
        assert_same(got, cpu, f"{name}: replay vs kCPU")

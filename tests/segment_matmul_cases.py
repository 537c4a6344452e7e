"""What test_segment_matmul_cpu.py and test_segment_matmul_gpu.py share: the case table of
`segment_matmul` at the smallest shapes the tiling can go wrong at (from the kernels' own BM / BN /
BK), the float64 reference (a torch loop over segments), the error bound of the numeric contract
(include/ofx_spmm.h) and the argument errors."""
from __future__ import annotations

import pytest
import torch

import oneflow_spmm as flow_spmm
from oneflow_spmm import _C, ops

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
P_BITS = {torch.float32: 24, torch.bfloat16: 8, torch.float16: 11}
INDEX = {"i32": torch.int32, "i64": torch.int64}


def table_lengths(bm):
    """Empty segments first, in the middle and last; tiles that straddle two and three segments."""
    return [0, 1, bm - 1, bm, bm + 1, 0, 2 * bm + 2, 0]


# name -> (segment lengths, F_in, F_out, idx?, padding of x's leading dimension, forced parts)
# as functions of (BM, BN, BK).  F_in covers {1, 15, 17, 40, 2 BK + 8}, F_out {1, 31, 40, BN + 8}.
CASES = {
    "table_wide": lambda bm, bn, bk: (table_lengths(bm), 2 * bk + 8, bn + 8, False, 0, 0),
    "table_idx": lambda bm, bn, bk: (table_lengths(bm), 17, 31, True, 0, 0),
    "one_segment": lambda bm, bn, bk: ([5], 1, 1, False, 0, 0),
    "no_rows": lambda bm, bn, bk: ([0, 0], 15, 40, False, 0, 0),
    "narrow_idx": lambda bm, bn, bk: ([3, 0, 70], 15, 1, True, 0, 0),
    "long_unaligned": lambda bm, bn, bk: ([3 * bm + 5], 40, 40, False, 3, 3),
}


def make_case(name, dtype, itype, device, seed=0, exact=True, f_in=None):
    lengths, fi, fo, with_idx, pad, parts = CASES[name](*_C.segment_matmul_tiles(dtype))
    fi = f_in or fi
    g = torch.Generator().manual_seed(seed)
    draw = (lambda *shape: torch.tensor([0., .5, -.5, 1., -1., 2., -2.])[
        torch.randint(0, 7, shape, generator=g)]) if exact else (
        lambda *shape: torch.randn(*shape, generator=g))
    s, t = sum(lengths), len(lengths)
    seg_ptr = torch.tensor([0] + lengths, dtype=torch.int64).cumsum(0).to(itype)
    r = max(s // 2, 1) if with_idx else s  # R < S
    idx = None
    if with_idx:
        idx = torch.randint(0, r, (s,), generator=g)  # repeated rows
        idx[0], idx[-1] = -1, r  # outside [0, R): zero rows
        idx = idx.to(itype).to(device)
    x = draw(r, fi + pad).to(dtype).to(device)[:, :fi]  # pad > 0: rows are not 16-byte aligned
    w = draw(t, fi, fo).to(dtype).to(device)
    dy = draw(s, fo).to(dtype).to(device)
    return x, w, seg_ptr.to(device), idx, dy, parts


def reference(x, w, seg_ptr, idx, dy, trans_w, round_rows_to=None):
    """(out, dx, dw, dx_rows) in float64 from a torch loop over the segments under torch autograd
    (dx_rows [S, F_in]: the gradient in the gathered rows); an idx outside [0, R) reads a zero row.
    round_rows_to: the dtype the [S, F_in] rows of dx are rounded to before they are summed over
    equal idx (the composition autograd.py documents)."""
    x, w, dy = (v.detach().double().cpu() for v in (x, w, dy))
    x, w = x.requires_grad_(), w.requires_grad_()
    bounds = seg_ptr.tolist()
    rows = None
    if idx is not None:
        rows = idx.long().cpu()
        ok = (rows >= 0) & (rows < x.shape[0])
        xs = torch.where(ok[:, None], x[rows.clamp(0, max(x.shape[0] - 1, 0))], 0.) \
            if x.shape[0] else torch.zeros(rows.numel(), x.shape[1], dtype=torch.float64)
    else:
        xs = x
    xs.retain_grad()
    outs = [xs[a:b] @ (w[t].T if trans_w else w[t]) for t, (a, b) in
            enumerate(zip(bounds[:-1], bounds[1:]))]
    out = torch.cat(outs) if outs else xs.new_zeros(0, w.shape[1 if trans_w else 2])
    out.backward(dy)
    dx = x.grad if x.grad is not None else torch.zeros_like(x)
    if idx is not None and round_rows_to is not None:
        dx = torch.zeros_like(x).index_add_(0, rows[ok], xs.grad[ok].to(round_rows_to).double())
    return out.detach(), dx, w.grad if w.grad is not None else torch.zeros_like(w), xs.grad


def run(x, w, seg_ptr, idx, dy, trans_w):
    """(out, dx, dw) through the public function and autograd."""
    x, w = x.detach().requires_grad_(), w.detach().requires_grad_()
    out = flow_spmm.segment_matmul(x, w, seg_ptr, idx, trans_w)
    dx, dw = torch.autograd.grad(out, (x, w), dy)
    return out.detach(), dx, dw


def check_exact(device, name, dt, it, trans_w):
    """Inputs from {0, +-0.5, +-1, +-2}: every partial sum is exact in f32, so forward, dw and dx
    equal the float64 results converted to the dtype, whatever the order of the sums."""
    dtype = DTYPES[dt]
    x, w, seg_ptr, idx, dy, parts = make_case(name, dtype, INDEX[it], device)
    if trans_w:
        w = w.transpose(1, 2).contiguous()
    got = run(x, w, seg_ptr, idx, dy, trans_w)
    want = reference(x, w, seg_ptr, idx, dy, trans_w, round_rows_to=dtype)
    for g, r, what in zip(got, want, ("out", "dx", "dw")):
        assert torch.equal(g.cpu(), r.to(dtype)), f"{name} {dt} {it} trans_w={trans_w}: {what}"
    if parts:  # the w-gradient's partial sums of >= 3 row parts, combined in order
        dw = _C.segment_matmul_grad_w(x, dy, seg_ptr, idx, parts=parts)
        if trans_w:
            dw = dw.transpose(1, 2)
        assert torch.equal(dw.cpu(), want[2].to(dtype)), f"{name} {dt} {it}: dw, parts={parts}"


def check_bound(device, dt, with_idx):
    """Seeded normal inputs at F_in = 136 over the table's segments, gradients of a scalar loss
    through autograd against the float64 torch loop: forward, dw and dx within
        2 n 2^-24 sum|a||b| + 2^-p |ref|        (n: the length of the sum; sum|a||b|: the same loop
    on the absolute values), and a second call gives the same bits.  With idx, dx is the rounded
    sum over c equal-idx rows of rows each rounded to the dtype first (autograd.py), so its bound
    is the sum B of those rows' own bounds plus the second sum's, on summands of magnitude at most
    A = sum of the rows' |ref_row| + B:
        B + 2 c 2^-24 A + 2^-p (|ref| + B).
    A result below the dtype's smallest normal number (a float16 product of two small normals in a
    segment of one row) is rounded to a subnormal, whose spacing is fixed: there the output rounding
    is half that spacing, which no correctly rounded result can beat, instead of 2^-p |ref|."""
    dtype, eps, u = DTYPES[dt], 2.0 ** -24, 2.0 ** -P_BITS[DTYPES[dt]]
    name = "table_idx" if with_idx else "table_wide"
    x, w, seg_ptr, idx, dy, _ = make_case(name, dtype, torch.int32, device, seed=1, exact=False,
                                          f_in=136)
    got = run(x, w, seg_ptr, idx, dy, False)
    for a, b, what in zip(got, run(x, w, seg_ptr, idx, dy, False), ("out", "dx", "dw")):
        assert torch.equal(a, b), f"{dt}: {what} differs between two calls"
    ref = reference(x, w, seg_ptr, idx, dy, False)
    mag = reference(x.abs(), w.abs(), seg_ptr, idx, dy.abs(), False)
    lengths = seg_ptr.cpu().diff().double()
    n = (torch.tensor(float(x.shape[1])), torch.tensor(float(dy.shape[1])), lengths[:, None, None])
    bounds = [2 * k * eps * m + u * r.abs() for k, m, r in zip(n, mag, ref)]
    if with_idx:
        rows = idx.long().cpu()
        ok = (rows >= 0) & (rows < x.shape[0])
        c = torch.zeros(x.shape[0], dtype=torch.float64).index_add_(0, rows[ok], torch.ones(
            int(ok.sum()), dtype=torch.float64))[:, None]
        row_bound = (2 * n[1] * eps * mag[3] + u * ref[3].abs())[ok]
        b = torch.zeros_like(ref[1]).index_add_(0, rows[ok], row_bound)
        a = torch.zeros_like(ref[1]).index_add_(0, rows[ok], ref[3].abs()[ok]) + b
        bounds[1] = b + 2 * c * eps * a + u * (ref[1].abs() + b)
    fi = torch.finfo(dtype)
    for g, r, bd, what in zip(got, ref, bounds, ("out", "dx", "dw")):
        bd = bd + (r.abs() < fi.tiny) * (fi.tiny * fi.eps / 2)  # tiny * eps: subnormal spacing
        err = (g.double().cpu() - r).abs()
        print(f"{dt} idx={with_idx} {what}: max err / bound = "
              f"{float((err / bd.clamp_min(1e-300)).max()) if err.numel() else 0.0:.3f}")
        assert bool((err <= bd).all()), f"{dt} idx={with_idx}: {what} outside the bound"
    empty = lengths == 0
    assert not bool(got[2][empty.to(got[2].device)].any()), "an empty segment's dw is not zero"


def check_errors(device):
    dev = torch.device(device)
    x = torch.ones(6, 4, device=dev)
    w = torch.ones(2, 4, 3, device=dev)
    sp = torch.tensor([0, 2, 6], dtype=torch.int32, device=dev)
    idx = torch.zeros(6, dtype=torch.int32, device=dev)
    f = flow_spmm.segment_matmul
    with pytest.raises(TypeError, match="x should be float32.*float64"):
        f(x.double(), w.double(), sp)
    with pytest.raises(TypeError, match="w datatype should be equal to x"):
        f(x, w.half(), sp)
    with pytest.raises(RuntimeError, match=r"w should be 3-D \[T, F_in, F_out\]"):
        f(x, w[0], sp)
    with pytest.raises(RuntimeError, match="x should have F_in = 3 columns as w \\(trans_w\\)"):
        f(x, w, sp, trans_w=True)
    assert f(x[:, :3], w, sp, trans_w=True).shape == (6, 4)
    with pytest.raises(RuntimeError, match="with T = 3 as seg_ptr"):
        f(x, w, torch.tensor([0, 2, 4, 6], dtype=torch.int32, device=dev))
    with pytest.raises(TypeError, match="seg_ptr should be int32 or int64"):
        f(x, w, sp.to(torch.int16))
    with pytest.raises(TypeError, match="idx should have the dtype of seg_ptr"):
        f(x, w, sp, idx.long())
    with pytest.raises(flow_spmm.OfxError, match="without idx the output has x's rows"):
        ops.segment_matmul(x, w, sp, s=5)
    with pytest.raises(flow_spmm.OfxError, match="the output overlaps an input"):
        ops.segment_matmul(x, torch.ones(2, 4, 4, device=dev), sp, out=x)
    if dev.type == "cpu":
        with pytest.raises(flow_spmm.OfxError, match="seg_ptr is decreasing at segment 1"):
            f(x, w, torch.tensor([0, 4, 2], dtype=torch.int32))
        with pytest.raises(flow_spmm.OfxError, match=r"seg_ptr\[T\] = 5 does not equal the 6"):
            f(x, w, torch.tensor([0, 2, 5], dtype=torch.int32))

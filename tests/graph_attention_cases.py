"""The checks of the fused multi-head graph attention (op "graph_attention_csr_heads", public
`oneflow_spmm.graph_attention`), written once for both devices (test_graph_attention_cpu.py runs
them on host tensors, test_graph_attention_gpu.py on the GPU, where every result is also compared
with the kCPU kernel's bits).  The rule under test (include/ofx_spmm.h): attn has
exactly the bits of ofx_edge_softmax_csr_heads on the output of ofx_sddmm_csr_heads(q, k), and out
exactly the bits of ofx_spmm_csr_heads(attn, v) under the same options.  The comparison object is
that composition through the three C-ABI entries, on the same device; every comparison is bit for
bit."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch

import edge_softmax_heads_cases as ehc
import heads_cases
import oneflow_spmm as flow_spmm
from helpers import DTYPES, random_csr, random_dense
from oneflow_spmm import _C, _lib, ops
from oneflow_spmm._C import current_stream_handle
from oneflow_spmm._lib import LIB
from reduce_cases import row_ranges
from reduce_helpers import PAD, assert_same, is_sentinel, options, padded, sentinel

M, K = heads_cases.M, heads_cases.K
# heads_cases.LENGTHS, then every boundary of the fused kernel's three phases: the softmax's
# lane-group capacities 8 G for G = 4, 16, 32 (a row beyond is taken over by the wave; 8, for
# G = 1, is in LENGTHS), its registers -> tiles boundary 512, which is also the default hub split
# at D <= 128, and two and three hub chunks with the remainder rule
LENGTHS = heads_cases.LENGTHS + [31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512, 513,
                                 1023, 1024, 1025, 1537]
HD_DT = heads_cases.HD_DT
SCHEDULES = heads_cases.SCHEDULES


@functools.lru_cache(maxsize=None)
def problem(h, d, dt, it="i32", exact=False, lengths=None, k=K, seed=0):
    """(rp, ci, q [M, H*D], k [K, H*D], v [K, H*D]) on the host; shared, never written."""
    rng = np.random.default_rng(seed + 1000 * h + d)
    dtype, idt = DTYPES[dt], torch.int32 if it == "i32" else torch.int64
    lens = list(lengths) if lengths is not None else [LENGTHS[r % len(LENGTHS)] for r in range(M)]
    rp, ci, _ = random_csr(len(lens), k, lens, rng, idx_dtype=idt, val_dtype=dtype)
    q = random_dense(len(lens), h * d, rng, dtype, exact)
    kk = random_dense(k, h * d, rng, dtype, exact)
    v = random_dense(k, h * d, rng, dtype, exact)
    return rp, ci, q, kk, v


def to_dev(dev, *ts):
    return tuple(t.to(dev) for t in ts)


def compose(rp, ci, q, kk, v, m, k, h, opts=None, row_begin=0, row_end=None):
    """The three C-ABI entries one after the other on the tensors' device: (out of the range's
    rows, attn [nnz, H] with sentinels outside the range's nonzeros)."""
    row_end = m if row_end is None else row_end
    e = sentinel((ci.numel(), h), kk.dtype, kk.device)
    ops.sddmm_csr_heads(rp, ci, q, kk, m, k, h, out=e, row_begin=row_begin, row_end=row_end)
    y = ehc.run_forward(rp, e, m, row_begin=row_begin, row_end=row_end, opts=opts)
    out = ops.spmm_csr_heads(rp, ci, y, v, m, k, h, row_begin=row_begin, row_end=row_end,
                             options=opts)
    return out, y


def fused(rp, ci, q, kk, v, m, k, h, opts=None, row_begin=0, row_end=None, pad=0, shift=0):
    """ofx_graph_attention_csr_heads(_cpu): out in a sentinel-filled (padded, shifted) buffer, attn
    in a sentinel-filled [nnz, H] buffer that starts `shift` elements into its allocation."""
    row_end = m if row_end is None else row_end
    n = kk.shape[1]
    out = padded(sentinel((row_end - row_begin, n), kk.dtype, kk.device), pad, shift)
    attn = sentinel((ci.numel() * h + shift,), kk.dtype, kk.device)[shift:].view(ci.numel(), h)
    ops.graph_attention_csr_heads(rp, ci, q, kk, v, m, k, h, out=out, attn=attn,
                                  row_begin=row_begin, row_end=row_end, options=opts)
    return out, attn


def assert_same_outside_nan(a, b, what):
    """The same elements are NaN, and every other element is bit-equal (the SpMM contract does not
    canonicalise a NaN's payload)."""
    a, b = a.contiguous(), b.contiguous().to(a.device)
    na, nb = torch.isnan(a), torch.isnan(b)
    assert torch.equal(na, nb), f"{what}: different elements are NaN"
    zero = torch.zeros((), dtype=a.dtype, device=a.device)
    assert_same(torch.where(na, zero, a), torch.where(nb, zero, b), what)


def check_forward(dev, h, d, dt, it="i32", exact=False, schedules=("default",), pad=0, shift=0,
                  lengths=None, k=K):
    """The fused entry on `dev` against the composition on `dev` and, on a device, against the
    kCPU fused kernel; q, k, v and out with leading dimension n + pad, `shift` elements into
    their buffers (attn shifted as well)."""
    rp, ci, q, kk, v = problem(h, d, dt, it, exact, lengths, k)
    m = rp.numel() - 1
    d_rp, d_ci, d_q, d_k, d_v = to_dev(dev, rp, ci, q, kk, v)
    pq, pk, pv = (padded(t, pad, shift) for t in (d_q, d_k, d_v))
    for name in schedules:
        o = heads_cases.opts_of(name)
        out, attn = fused(d_rp, d_ci, pq, pk, pv, m, k, h, o, pad=pad, shift=shift)
        what = f"graph attention H={h} D={d} {dt} {it} {name} pad={pad} shift={shift}"
        want_out, want_attn = compose(d_rp, d_ci, d_q, d_k, d_v, m, k, h, o)
        assert_same(attn, want_attn, f"{what}: attn vs composition")
        assert_same(out, want_out, f"{what}: out vs composition")
        if dev != "cpu":
            c_out, c_attn = ops.graph_attention_csr_heads(rp, ci, q, kk, v, m, k, h, options=o)
            assert_same(attn, c_attn, f"{what}: attn vs kCPU")
            assert_same(out, c_out, f"{what}: out vs kCPU")
        if pad:
            assert bool(is_sentinel(out._base[shift:].view(m, h * d + pad)[:, h * d:]).all()), \
                f"{what}: wrote into the padding"


def check_row_ranges(dev, h, d, dt, schedule="split8"):
    """A range writes exactly its own rows of out (rebased to the range) and its own nonzeros of
    attn (global positions): sentinels around stay untouched."""
    rp, ci, q, kk, v = problem(h, d, dt)
    m, n = rp.numel() - 1, h * d
    d_rp, d_ci, d_q, d_k, d_v = to_dev(dev, rp, ci, q, kk, v)
    o = heads_cases.opts_of(schedule)
    full_out, full_attn = compose(d_rp, d_ci, d_q, d_k, d_v, m, K, h, o)
    rpn = rp.numpy()
    for lo, hi in row_ranges(m):
        buf = sentinel((m + 2, n + PAD), kk.dtype, dev)
        out = buf[1:1 + hi - lo, :n]
        attn = sentinel((ci.numel(), h), kk.dtype, dev)
        ops.graph_attention_csr_heads(d_rp, d_ci, d_q[lo:hi], d_k, d_v, m, K, h, out=out, attn=attn,
                                      row_begin=lo, row_end=hi, options=o)
        assert_same(out, full_out[lo:hi], f"rows [{lo}, {hi}): out")
        kept = is_sentinel(buf)
        kept[1:1 + hi - lo, :n] = True
        assert bool(kept.all()), f"rows [{lo}, {hi}): wrote outside its rows of out"
        j0, j1 = int(rpn[lo]), int(rpn[hi])
        assert_same(attn[j0:j1], full_attn[j0:j1], f"rows [{lo}, {hi}): attn")
        kept = is_sentinel(attn)
        assert bool(kept[:j0].all()) and bool(kept[j1:].all()), \
            f"rows [{lo}, {hi}): wrote outside its nonzeros of attn"
        c_out, c_attn = compose(d_rp, d_ci, d_q[lo:hi], d_k, d_v, m, K, h, o, lo, hi)
        assert_same(out, c_out, f"rows [{lo}, {hi}): out vs the composition on the range")
        assert_same(attn, c_attn, f"rows [{lo}, {hi}): attn vs the composition on the range")


def check_columns_out_of_range(dev, dt):
    """Columns >= K (a zero row in both gathers) on the fast path (8, 16) and the general one
    (3, 5)."""
    for h, d in ((8, 16), (3, 5)):
        rp, ci, q, kk, v = problem(h, d, dt)
        m = rp.numel() - 1
        kcut = K // 2  # half of the columns now lie outside [0, kcut)
        d_rp, d_ci, d_q, d_k, d_v = to_dev(dev, rp, ci, q, kk[:kcut], v[:kcut])
        out, attn = fused(d_rp, d_ci, d_q, d_k, d_v, m, kcut, h)
        want_out, want_attn = compose(d_rp, d_ci, d_q, d_k, d_v, m, kcut, h)
        assert_same(attn, want_attn, f"columns >= K, H={h} D={d} {dt}: attn")
        assert_same(out, want_out, f"columns >= K, H={h} D={d} {dt}: out")


def check_special_confined(dev, dt, h=4, d=16):
    """Head 0's q row holds a NaN and head 1's is so large that its scores overflow to +inf (k's
    head-1 columns are made positive), in rows 5 and 9 (lengths 9 and 130): attn equals the
    composition bit for bit, NaN in those heads only; out has the same NaN elements as the
    composition's and is bit-equal elsewhere."""
    rp, ci, q, kk, v = problem(h, d, dt)
    m = rp.numel() - 1
    dtype = DTYPES[dt]
    big = {torch.float16: 6.0e4, torch.float64: 1.0e308}.get(dtype, 3.0e38)
    q, kk = q.clone(), kk.clone()
    kk[:, d:2 * d] = kk[:, d:2 * d].abs() + 0.25
    rows = (5, 9)
    for r in rows:
        q[r, 3] = float("nan")
        q[r, d:2 * d] = big
    d_rp, d_ci, d_q, d_k, d_v = to_dev(dev, rp, ci, q, kk, v)
    out, attn = fused(d_rp, d_ci, d_q, d_k, d_v, m, K, h)
    want_out, want_attn = compose(d_rp, d_ci, d_q, d_k, d_v, m, K, h)
    what = f"special values {dt}"
    assert_same(attn, want_attn, f"{what}: attn vs composition")
    assert_same_outside_nan(out, want_out, f"{what}: out vs composition")
    if dev != "cpu":
        c_out, c_attn = ops.graph_attention_csr_heads(rp, ci, q, kk, v, m, K, h)
        assert_same(attn, c_attn, f"{what}: attn vs kCPU")
        assert_same_outside_nan(out, c_out, f"{what}: out vs kCPU")
    rpn = rp.numpy()
    nan = torch.isnan(attn.cpu().float())
    expect = torch.zeros_like(nan)
    for r in rows:
        j0, j1 = int(rpn[r]), int(rpn[r + 1])
        assert j1 - j0 > 1
        expect[j0:j1, 0] = True   # a NaN score: the whole row of the head is the canonical NaN
        expect[j0:j1, 1] = True   # every score +inf: inf - inf
    assert torch.equal(nan, expect), f"{what}: NaN outside heads 0 and 1 of rows {rows}"
    onan = torch.isnan(out.cpu().float()).view(m, h, d)
    assert bool(onan[list(rows), :2].all()) and not bool(onan[list(rows), 2:].any())
    onan[list(rows)] = False
    assert not bool(onan.any()), f"{what}: a NaN leaked into another row of out"


def check_single_head_and_empty(dev, dt):
    """H == 1 gives the single-head composition's bits; heads == 0, nnz == 0 and an empty row
    range return OFX_OK, and out gets the composition's zeros."""
    rp, ci, q, kk, v = problem(1, 16, dt)
    m = rp.numel() - 1
    d_rp, d_ci, d_q, d_k, d_v = to_dev(dev, rp, ci, q, kk, v)
    out, attn = fused(d_rp, d_ci, d_q, d_k, d_v, m, K, 1)
    e = _C.sddmm_csr(d_rp, d_ci, d_q, d_k, m, K)
    y = _C.edge_softmax_csr(d_rp, d_ci, e)
    assert_same(attn[:, 0], y, "H == 1: attn")
    assert_same(out, _C.spmm_csr(d_rp, d_ci, y, m, K, d_v), "H == 1: out")
    dtype = DTYPES[dt]
    rp0 = torch.zeros(4, dtype=torch.int32, device=dev)
    q3 = d_q[:3].contiguous()
    out = sentinel((3, 16), dtype, dev)
    ops.graph_attention_csr_heads(rp0, rp0[:0], q3, d_k, d_v, 3, K, 1, out=out,
                                  attn=torch.empty((0, 1), dtype=dtype, device=dev))
    assert_same(out, torch.zeros((3, 16), dtype=dtype), "nnz == 0: zeros in out")
    out = sentinel((m, 16), dtype, dev)
    att = sentinel((ci.numel(), 1), dtype, dev)
    ops.graph_attention_csr_heads(d_rp, d_ci, d_q, d_k, d_v, m, K, 1, out=out, attn=att,
                                  row_begin=7, row_end=7)
    empty = torch.empty((m, 0), dtype=dtype, device=dev)
    ops.graph_attention_csr_heads(d_rp, d_ci, empty, d_k[:, :0], d_v[:, :0], m, K, 0, out=empty,
                                  attn=torch.empty((ci.numel(), 0), dtype=dtype, device=dev))
    assert bool(is_sentinel(out).all()) and bool(is_sentinel(att).all())


def check_public_api(dev):
    """graph_attention equals spmm(edge_softmax(sddmm(q, k)), v) bit for bit in the 3-D and 2-D
    forms, with and without the weights, for non-contiguous inputs; shapes and argument errors."""
    h, d = 3, 5
    rp, ci, q, kk, v = problem(h, d, "f32")
    m = rp.numel() - 1
    d_rp, d_ci, d_q, d_k, d_v = to_dev(dev, rp, ci, q, kk, v)
    q3, k3, v3 = d_q.view(m, h, d), d_k.view(K, h, d), d_v.view(K, h, d)
    y = flow_spmm.edge_softmax(d_rp, d_ci, flow_spmm.sddmm(d_rp, d_ci, q3, k3))
    want = flow_spmm.spmm(d_rp, d_ci, y, m, K, v3)
    out = flow_spmm.graph_attention(d_rp, d_ci, q3, k3, v3)
    assert tuple(out.shape) == (m, h, d)
    assert_same(out, want, "3-D out")
    out, attn = flow_spmm.graph_attention(d_rp, d_ci, q3, k3, v3, return_attention=True)
    assert tuple(attn.shape) == (ci.numel(), h)
    assert_same(out, want, "3-D out (return_attention)")
    assert_same(attn, y, "3-D attn")
    # non-contiguous inputs are made contiguous
    wide = torch.cat([q3, q3], dim=2)[:, :, :d]
    kt = k3.transpose(1, 2).contiguous().transpose(1, 2)
    assert not wide.is_contiguous() and not kt.is_contiguous()
    assert_same(flow_spmm.graph_attention(d_rp, d_ci, wide, kt, v3), want, "non-contiguous")
    # the 2-D forms mean H = 1
    q2, k2, v2 = q3[:, 0].contiguous(), k3[:, 0].contiguous(), v3[:, 0].contiguous()
    y1 = flow_spmm.edge_softmax(d_rp, d_ci, flow_spmm.sddmm(d_rp, d_ci, q2, k2))
    out, attn = flow_spmm.graph_attention(d_rp, d_ci, q2, k2, v2, return_attention=True)
    assert tuple(out.shape) == (m, d) and tuple(attn.shape) == (ci.numel(), 1)
    assert_same(attn[:, 0], y1, "2-D attn")
    assert_same(out, flow_spmm.spmm(d_rp, d_ci, y1, m, K, v2), "2-D out")
    # argument errors
    with pytest.raises(RuntimeError, match="same heads and D"):
        flow_spmm.graph_attention(d_rp, d_ci, q3, k3[:, :2], v3[:, :2])          # H
    with pytest.raises(RuntimeError, match="same heads and D"):
        flow_spmm.graph_attention(d_rp, d_ci, q3, k3[:, :, :4], v3[:, :, :4])    # D
    with pytest.raises(RuntimeError, match="same heads and D"):
        flow_spmm.graph_attention(d_rp, d_ci, q3, k3, v3[:-1])                   # K of v
    with pytest.raises(RuntimeError, match="expected"):
        flow_spmm.graph_attention(d_rp, d_ci, q3, k2, v2)                        # 3-D with 2-D
    with pytest.raises(TypeError, match="one dtype"):
        flow_spmm.graph_attention(d_rp, d_ci, q3.double(), k3, v3)
    with pytest.raises(TypeError):
        flow_spmm.graph_attention(d_rp, d_ci, q3.int(), k3.int(), v3.int())
    with pytest.raises(TypeError, match="dtype of a_csr_row_ptr"):
        flow_spmm.graph_attention(d_rp, d_ci.long(), q3, k3, v3)
    with pytest.raises(RuntimeError, match="a_num_rows"):
        flow_spmm.graph_attention(d_rp, d_ci, q3[:-1], k3, v3)
    if dev != "cpu":
        with pytest.raises(RuntimeError, match="same device"):
            flow_spmm.graph_attention(d_rp, d_ci, q3, k3.cpu(), v3)


def _entry(dev, like):
    """The C-ABI entry of `dev` as call(*body) -> rc with a NULL workspace and default options."""
    if dev == "cpu":
        return lambda *a, opts=None: LIB.ofx_graph_attention_csr_heads_cpu(0, *a, opts)
    s = current_stream_handle(like)
    return lambda *a, opts=None: LIB.ofx_graph_attention_csr_heads(s, *a, None, 0, opts)


def check_argument_checks(dev):
    """attn aliasing an input, a NULL attn, planned / variant, D > 2048, bad strides, ranges and
    dtypes return the documented code, and nothing is launched: the outputs keep their sentinels."""
    h, d = 2, 4
    rp, ci, q, kk, v = problem(h, d, "f32", lengths=(3, 0, 5, 2), k=16)
    m, n, nnz = 4, h * d, ci.numel()
    d_rp, d_ci, d_q, d_k, d_v = to_dev(dev, rp, ci, q, kk, v)
    out = sentinel((m, n), torch.float32, dev)
    attn = sentinel((nnz, h), torch.float32, dev)
    I, F = _lib.DT_INT32, _lib.DT_FLOAT
    call = _entry(dev, d_k)
    P = lambda t: t.data_ptr()  # noqa: E731

    def body(idt=I, vdt=F, heads=h, dd=d, nz=nnz, qp=P(d_q), ldq=n, kp=P(d_k), ldk=n, vp=P(d_v),
             ldv=n, op=P(out), ldo=n, ap=P(attn), lo=0, hi=m):
        return (idt, vdt, m, 16, heads, dd, nz, P(d_rp), P(d_ci), qp, ldq, kp, ldk, vp, ldv, op, ldo,
                ap, lo, hi)

    E = _lib.OFX_EINVAL
    assert call(*body(ap=None)) == E and b"attn" in LIB.ofx_last_error()       # NULL attn
    for alias in (d_q, d_k, d_v, out):                                         # attn aliases
        assert call(*body(ap=P(alias))) == E and b"overlaps" in LIB.ofx_last_error()
    assert call(*body(ap=P(d_k) + 4 * n)) == E                                 # inside k
    for bad in (options(planned=True), ops.make_options(variant=1)):
        assert call(*body(), opts=ctypes.byref(bad)) == E
        assert b"not supported" in LIB.ofx_last_error()
    assert call(*body(dd=2049, ldq=h * 2049, ldk=h * 2049, ldv=h * 2049, ldo=h * 2049)) == \
        _lib.OFX_EUNSUPPORTED                                                  # D > 2048
    assert call(*body(heads=-1)) == E
    assert call(*body(nz=-3)) == E
    assert call(*body(ldq=n - 1)) == E and call(*body(ldo=n - 1)) == E         # strides < H*D
    assert call(*body(ldk=n - 1)) == E and call(*body(ldv=n - 1)) == E
    assert call(*body(lo=1, hi=m + 1)) == E and call(*body(lo=2, hi=1)) == E   # row range
    assert call(*body(qp=None)) == E and call(*body(op=None)) == E             # NULL pointers
    assert call(*body(vdt=_lib.DT_INT64)) == _lib.OFX_EUNSUPPORTED
    assert call(*body(idt=F)) == _lib.OFX_EUNSUPPORTED
    bad = _lib.Options()
    bad.magic = 0
    assert call(*body(), opts=ctypes.byref(bad)) == E
    size = ctypes.c_size_t(7)
    assert LIB.ofx_graph_attention_csr_heads_workspace_size(I, F, m, 16, h, d, nnz, None,
                                                            ctypes.byref(size)) == _lib.OFX_OK
    assert size.value == 0
    assert LIB.ofx_graph_attention_csr_heads_workspace_size(I, F, m, 16, h, d, nnz, None,
                                                            None) == E
    if dev != "cpu":
        s = current_stream_handle(d_k)
        assert LIB.ofx_graph_attention_csr_heads(s, *body(), None, 16, None) == \
            _lib.OFX_EWORKSPACE                                # a NULL workspace of 16 bytes
        torch.cuda.synchronize()
    assert bool(is_sentinel(out).all()) and bool(is_sentinel(attn).all())
    assert call(*body()) == _lib.OFX_OK
    assert not bool(is_sentinel(out).any()) and not bool(is_sentinel(attn).any())


def check_op_layer(dev):
    """The op through the registry dispatch against the C-ABI, out= / attn_out=, the functional
    entry's two phases, the refusals of the binding and of the op's own inference, its SBP."""
    h, d = 3, 5
    rp, ci, q, kk, v = problem(h, d, "f32")
    m, n, nnz = rp.numel() - 1, h * d, ci.numel()
    d_rp, d_ci, d_q, d_k, d_v = to_dev(dev, rp, ci, q, kk, v)
    want_out, want_attn = ops.graph_attention_csr_heads(d_rp, d_ci, d_q, d_k, d_v, m, K, h)
    out, attn = _C.graph_attention_csr_heads(d_rp, d_ci, d_q, d_k, d_v, h)
    assert_same(out, want_out, "op vs C-ABI (out)")
    assert_same(attn, want_attn, "op vs C-ABI (attn)")
    for dt, it, hh, dd in (("f64", "i64", 4, 16), ("bf16", "i32", 8, 16), ("f16", "i64", 5, 1)):
        x = to_dev(dev, *problem(hh, dd, dt, it))
        o2, a2 = _C.graph_attention_csr_heads(*x, hh)
        w_o, w_a = ops.graph_attention_csr_heads(*x, x[0].numel() - 1, K, hh)
        assert_same(o2, w_o, f"op vs C-ABI {dt} {it} (out)")
        assert_same(a2, w_a, f"op vs C-ABI {dt} {it} (attn)")
    # out= (row-strided) and attn_out= are written directly
    buf = sentinel((m, n + PAD), torch.float32, dev)
    att = sentinel((nnz, h), torch.float32, dev)
    o2, a2 = _C.graph_attention_csr_heads(d_rp, d_ci, d_q, d_k, d_v, h, out=buf[:, :n],
                                          attn_out=att)
    assert o2.data_ptr() == buf.data_ptr() and a2 is att
    assert_same(buf[:, :n], want_out, "out=")
    assert_same(att, want_attn, "attn_out=")
    assert bool(is_sentinel(buf[:, n:]).all())
    with pytest.raises(RuntimeError, match="contiguous"):
        _C.graph_attention_csr_heads(d_rp, d_ci, d_q, d_k, d_v, h,
                                     attn_out=sentinel((nnz, 2 * h), torch.float32, dev)[:, :h])
    with pytest.raises(RuntimeError, match="multiple"):
        _C.graph_attention_csr_heads(d_rp, d_ci, d_q, d_k, d_v, 4)   # 15 % 4
    with pytest.raises(RuntimeError, match="same number of columns"):
        _C.graph_attention_csr_heads(d_rp, d_ci, d_q[:, :10].contiguous(), d_k, d_v, h)
    with pytest.raises(RuntimeError, match="same number of rows"):
        _C.graph_attention_csr_heads(d_rp, d_ci, d_q, d_k, d_v[:-1], h)
    with pytest.raises(TypeError, match="q datatype should be equal to k"):
        _C.graph_attention_csr_heads(d_rp, d_ci, d_q.half(), d_k, d_v, h)
    with pytest.raises(TypeError, match="dtype of a_csr_row_ptr"):
        _C.graph_attention_csr_heads(d_rp, d_ci.long(), d_q, d_k, d_v, h)
    # the functional entry itself: the tmp size first, then the run; the op's own inference
    o3, a3 = torch.empty_like(want_out), torch.empty_like(want_attn)
    byref = lambda *ts: [ctypes.byref(_C.desc(t)) for t in ts]  # noqa: E731
    fn = LIB.ofx_functional_graph_attention_csr_heads
    size = ctypes.c_size_t(123)
    _lib.check(fn(None, *byref(d_rp, d_ci, d_q, d_k, d_v), h, *byref(o3, a3), None, 0,
                  ctypes.byref(size)), "tmp")
    # the HIP kernel's hub rows need the planner's work list and the chunks' partials
    assert (size.value == 0) == (dev == "cpu")
    tmp = torch.empty(max(size.value, 1), dtype=torch.uint8, device=dev)
    _lib.check(fn(current_stream_handle(d_k), *byref(d_rp, d_ci, d_q, d_k, d_v), h, *byref(o3, a3),
                  tmp.data_ptr() if size.value else None, size.value, None), "run")
    assert_same(o3, want_out, "functional entry (out)")
    assert_same(a3, want_attn, "functional entry (attn)")
    rc = fn(None, *byref(d_rp, d_ci, d_q, d_k, d_v), 4, *byref(o3, a3), None, 0,
            ctypes.byref(size))
    assert rc == _lib.OFX_EINVAL and "multiple" in _lib.last_error()
    rc = fn(None, *byref(d_rp, d_ci, d_q, d_k, d_v[:-1]), h, *byref(o3, a3), None, 0,
            ctypes.byref(size))
    assert rc == _lib.OFX_EINVAL and "rows" in _lib.last_error()
    s = _C.sbp_signatures("graph_attention_csr_heads")
    sigs, no_grad = s.split("|")
    assert len(sigs.split(";")) == 1, s  # all-broadcast only
    assert set(sigs.split(",")) == {f"{x}:B" for x in ("a_csr_row_ptr", "a_csr_col_idx", "q", "k",
                                                       "v", "out", "attn")}, s
    assert set(no_grad.split(":")[1].split(",")) == {"a_csr_row_ptr", "a_csr_col_idx"}, s


# ---- autograd -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grad_graph(h, d, seed=21):
    """A 40-row graph with a hub (600 > the split of 512) and q, k, v [*, H, D] in f32 (host)."""
    rng = np.random.default_rng(seed)
    lens = [3, 1, 0, 5, 2, 12, 4, 1, 7, 600] + [LENGTHS[r % 10] for r in range(30)]
    rp, ci, _ = random_csr(len(lens), 700, lens, rng)
    mk = lambda rows: torch.from_numpy(rng.uniform(-1, 1, size=(rows, h, d))).float()  # noqa: E731
    return rp, ci, mk(len(lens)), mk(700), mk(700)


def check_grads_match_composition(dev, h, d, with_attn):
    """d(q), d(k), d(v) of graph_attention = the composed layer's autograd, bit for bit; with_attn:
    the returned weights enter the loss as well."""
    rp, ci, q, kk, v = grad_graph(h, d)
    m, k = rp.numel() - 1, kk.shape[0]
    d_rp, d_ci = to_dev(dev, rp, ci)
    rng = np.random.default_rng(9)
    w = torch.from_numpy(rng.uniform(-1, 1, size=(m, h, d))).float().to(dev)
    wa = torch.from_numpy(rng.uniform(-1, 1, size=(ci.numel(), h))).float().to(dev)
    a = tuple(t.clone().to(dev).requires_grad_(True) for t in (q, kk, v))
    b = tuple(t.clone().to(dev).requires_grad_(True) for t in (q, kk, v))
    out, attn = flow_spmm.graph_attention(d_rp, d_ci, *a, return_attention=True)
    y = flow_spmm.edge_softmax(d_rp, d_ci, flow_spmm.sddmm(d_rp, d_ci, b[0], b[1]))
    ref = flow_spmm.spmm(d_rp, d_ci, y, m, k, b[2])
    assert_same(out, ref, "forward out")
    assert_same(attn, y, "forward attn")
    loss, loss_ref = (out * w).sum(), (ref * w).sum()
    if with_attn:
        loss, loss_ref = loss + (attn * wa).sum(), loss_ref + (y * wa).sum()
    loss.backward()
    loss_ref.backward()
    for name, x, z in zip("qkv", a, b):
        assert_same(x.grad, z.grad, f"d({name}) H={h} D={d} with_attn={with_attn}")


def check_needs_input_grad(dev):
    """Only the gradients that are asked for are computed, each with the full backward's bits."""
    h, d = 3, 5
    rp, ci, q, kk, v = grad_graph(h, d)
    d_rp, d_ci = to_dev(dev, rp, ci)
    full = tuple(t.clone().to(dev).requires_grad_(True) for t in (q, kk, v))
    flow_spmm.graph_attention(d_rp, d_ci, *full).sum().backward()
    for i, name in enumerate("qkv"):
        one = [t.clone().to(dev) for t in (q, kk, v)]
        one[i].requires_grad_(True)
        flow_spmm.graph_attention(d_rp, d_ci, *one).sum().backward()
        assert_same(one[i].grad, full[i].grad, f"d({name}) alone")
        assert all(t.grad is None for j, t in enumerate(one) if j != i)


def check_gradcheck(dev):
    rp, ci, _, b, a = heads_cases.grad_problem(torch.float64)
    d_rp, d_ci = to_dev(dev, rp, ci)
    rng = np.random.default_rng(2)
    v = torch.from_numpy(rng.uniform(-1, 1, size=tuple(b.shape)))
    q, kk, vv = (t.to(dev).requires_grad_(True) for t in (a, b, v))
    assert torch.autograd.gradcheck(lambda x, y, z: flow_spmm.graph_attention(d_rp, d_ci, x, y, z),
                                    (q, kk, vv))
    assert torch.autograd.gradcheck(
        lambda x, y, z: flow_spmm.graph_attention(d_rp, d_ci, x, y, z, return_attention=True),
        (q, kk, vv))


def check_dense_reference_f32(dev, h=3, d=5):
    """graph_attention with H = 3, D = 5 on attention_problem's graph in f32 against the float64
    dense reference per head: output and the three gradients within atol = 1e-5
    (check_attention_heads_f32's tolerance, taken over unchanged)."""
    from edge_softmax_cases import attention_problem
    from edge_softmax_helpers import dense_attention
    rp, ci, _, _, _ = attention_problem(torch.float64)
    rng = np.random.default_rng(12)
    q, k, v, w = (torch.from_numpy(rng.uniform(-1, 1, size=(12, h, d))) for _ in range(4))
    dense = tuple(t.clone().requires_grad_(True) for t in (q, k, v))
    ref = torch.stack([dense_attention(rp, ci, *(t[:, i, :] for t in dense)) for i in range(h)], 1)
    (ref * w).sum().backward()
    d_rp, d_ci = to_dev(dev, rp, ci)
    ours = tuple(t.float().to(dev).requires_grad_(True) for t in (q, k, v))
    out = flow_spmm.graph_attention(d_rp, d_ci, *ours)
    assert tuple(out.shape) == (12, h, d)
    torch.testing.assert_close(out.detach().cpu().double(), ref.detach(), rtol=0, atol=1e-5)
    (out * w.float().to(dev)).sum().backward()
    for name, x, y in zip("qkv", ours, dense):
        torch.testing.assert_close(x.grad.cpu().double(), y.grad, rtol=0, atol=1e-5,
                                   msg=lambda s, n=name: f"d({n}): {s}")


def check_threads_do_not_matter():
    rp, ci, q, kk, v = problem(3, 5, "f32")
    m = rp.numel() - 1
    one = ops.graph_attention_csr_heads(rp, ci, q, kk, v, m, K, 3, num_threads=1)
    many = ops.graph_attention_csr_heads(rp, ci, q, kk, v, m, K, 3, num_threads=7)
    assert_same(one[0], many[0], "out")
    assert_same(one[1], many[1], "attn")

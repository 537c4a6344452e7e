"""Cases of the multi-head SpMM / SDDMM tests (ops "spmm_csr_heads", "sddmm_csr_heads"), shared by
test_heads_cpu.py and test_heads_gpu.py.  The rule under test (include/ofx_spmm.h):
every head's slice has exactly the bits of the single-head op on that slice.  All comparisons are
bit for bit; a device run is compared both with the kCPU heads kernel and with the per-head loop
of the single-head op on the same device."""
from __future__ import annotations

import functools

import numpy as np
import torch

import oneflow_spmm as flow_spmm
from helpers import DTYPES, random_csr, random_dense
from oneflow_spmm import _C, ops
from reduce_cases import row_ranges
from reduce_helpers import PAD, assert_same, is_sentinel, options, padded, sentinel

LENGTHS = [0, 1, 2, 7, 8, 9, 63, 64, 65, 130]
M = 40
K = 2048
HD = [(1, 16), (2, 4), (3, 5), (5, 1), (4, 16), (8, 16), (8, 64), (16, 64)]
# (16, 64) is N = 1024: the 16-bit types only
HD_DT = [(h, d, dt) for (h, d) in HD for dt in ("f32", "f64", "bf16", "f16")
         if (h, d) != (16, 64) or dt in ("bf16", "f16")]
SCHEDULES = {"default": None, "split8": dict(split=8, chunk=8), "split8_chunk4": dict(split=8, chunk=4),
             "ordered": dict(ordered=True)}


def opts_of(name):
    kw = SCHEDULES[name]
    return None if kw is None else options(**kw)


@functools.lru_cache(maxsize=None)
def problem(h, d, dt, it="i32", exact=False, lengths=None, m=M, k=K, seed=0):
    """(rp, ci, values [nnz, H], b [K, H*D], a [M, H*D]) on the host; shared, never written."""
    rng = np.random.default_rng(seed + 1000 * h + d)
    dtype, idt = DTYPES[dt], torch.int32 if it == "i32" else torch.int64
    lens = list(lengths) if lengths is not None else [LENGTHS[r % len(LENGTHS)] for r in range(m)]
    rp, ci, _ = random_csr(len(lens), k, lens, rng, idx_dtype=idt, val_dtype=dtype)
    vals = random_dense(ci.numel(), h, rng, dtype, exact)
    b = random_dense(k, h * d, rng, dtype, exact)
    a = random_dense(len(lens), h * d, rng, dtype, exact)
    return rp, ci, vals, b, a


def to_dev(dev, *ts):
    return tuple(t.to(dev) for t in ts)


def head(t, h, d):
    """Head h's D columns of a [rows, H*D] tensor: a row-strided view."""
    return t[:, h * d:(h + 1) * d]


# ---- the per-head compositions --------------------------------------------------------------------
def spmm_loop(rp, ci, vals, b, m, k, heads, opts=None, row_begin=0, row_end=None):
    """The single-head op per head, on the tensors' device (kCPU kernel or HIP kernel)."""
    d = b.shape[1] // heads
    row_end = m if row_end is None else row_end
    out = torch.empty((row_end - row_begin, b.shape[1]), dtype=b.dtype, device=b.device)
    run = ops.spmm_csr_cpu if b.device.type == "cpu" else ops.spmm_csr_device
    for h in range(heads):
        run(rp, ci, vals[:, h].contiguous(), head(b, h, d), m, k, out=head(out, h, d),
            row_begin=row_begin, row_end=row_end, options=opts)
    return out


def sddmm_loop(rp, ci, a, b, heads):
    d = b.shape[1] // heads
    m, k = rp.numel() - 1, b.shape[0]
    return torch.stack([_C.sddmm_csr(rp, ci, head(a, h, d), head(b, h, d), m, k)
                        for h in range(heads)], dim=1)


# ---- checks ---------------------------------------------------------------------------------------
def check_spmm(dev, h, d, dt, it="i32", exact=False, schedules=SCHEDULES, pad=0, shift=0,
               lengths=None, k=K):
    """ofx_spmm_csr_heads(_cpu) on `dev` against the per-head loop on `dev` and, on a device,
    against the kCPU heads kernel; b and out with leading dimension n + pad, `shift` elements into
    their buffers."""
    rp, ci, vals, b, _ = problem(h, d, dt, it, exact, lengths, k=k)
    m = rp.numel() - 1
    d_rp, d_ci, d_vals, d_b = to_dev(dev, rp, ci, vals, b)
    bb = padded(d_b, pad, shift)
    for name in schedules:
        o = opts_of(name)
        out = padded(sentinel((m, h * d), b.dtype, dev), pad, shift)
        ops.spmm_csr_heads(d_rp, d_ci, d_vals, bb, m, k, h, out=out, options=o)
        what = f"spmm heads H={h} D={d} {dt} {it} {name} pad={pad} shift={shift}"
        assert_same(out, spmm_loop(d_rp, d_ci, d_vals, d_b, m, k, h, o), f"{what} vs per-head loop")
        if dev != "cpu":
            assert_same(out, ops.spmm_csr_heads(rp, ci, vals, b, m, k, h, options=o),
                        f"{what} vs kCPU")
        if pad:
            assert bool(is_sentinel(out._base[shift:].view(m, h * d + pad)[:, h * d:]).all()), \
                f"{what}: wrote into the padding"


def check_sddmm(dev, h, d, dt, it="i32", exact=False, pad=0, shift=0, lengths=None, k=K):
    rp, ci, _, b, a = problem(h, d, dt, it, exact, lengths, k=k)
    m = rp.numel() - 1
    d_rp, d_ci, d_a, d_b = to_dev(dev, rp, ci, a, b)
    out = ops.sddmm_csr_heads(d_rp, d_ci, padded(d_a, pad, shift), padded(d_b, pad, shift), m, k, h)
    what = f"sddmm heads H={h} D={d} {dt} {it} pad={pad} shift={shift}"
    assert_same(out, sddmm_loop(d_rp, d_ci, d_a, d_b, h), f"{what} vs per-head loop")
    if dev != "cpu":
        assert_same(out, ops.sddmm_csr_heads(rp, ci, a, b, m, k, h), f"{what} vs kCPU")


def check_row_ranges(dev, h, d, dt, schedule="split8"):
    """A range writes exactly its own rows (SpMM) or nonzeros (SDDMM): sentinels around and
    between stay untouched."""
    rp, ci, vals, b, a = problem(h, d, dt)
    m, n, nnz = rp.numel() - 1, h * d, ci.numel()
    d_rp, d_ci, d_vals, d_b, d_a = to_dev(dev, rp, ci, vals, b, a)
    o = opts_of(schedule)
    full = ops.spmm_csr_heads(d_rp, d_ci, d_vals, d_b, m, K, h, options=o)
    full_sd = ops.sddmm_csr_heads(d_rp, d_ci, d_a, d_b, m, K, h)
    rpn = rp.numpy()
    for lo, hi in row_ranges(m):
        buf = sentinel((m + 2, n + PAD), b.dtype, dev)
        out = buf[1:1 + hi - lo, :n]
        ops.spmm_csr_heads(d_rp, d_ci, d_vals, d_b, m, K, h, out=out, row_begin=lo, row_end=hi,
                           options=o)
        assert_same(out, full[lo:hi], f"spmm heads rows [{lo}, {hi})")
        kept = is_sentinel(buf)
        kept[1:1 + hi - lo, :n] = True
        assert bool(kept.all()), f"spmm heads rows [{lo}, {hi}): wrote outside its rows"
        sd = sentinel((nnz, h), b.dtype, dev)
        ops.sddmm_csr_heads(d_rp, d_ci, d_a[lo:hi], d_b, m, K, h, out=sd, row_begin=lo, row_end=hi)
        j0, j1 = int(rpn[lo]), int(rpn[hi])
        assert_same(sd[j0:j1], full_sd[j0:j1], f"sddmm heads rows [{lo}, {hi})")
        kept = is_sentinel(sd)
        assert bool(kept[:j0].all()) and bool(kept[j1:].all()), \
            f"sddmm heads rows [{lo}, {hi}): wrote outside its nonzeros"


def check_single_head(dev, dt):
    """H = 1 is the single-head op."""
    rp, ci, vals, b, a = problem(1, 16, dt)
    m = rp.numel() - 1
    d_rp, d_ci, d_vals, d_b, d_a = to_dev(dev, rp, ci, vals, b, a)
    assert_same(_C.spmm_csr_heads(d_rp, d_ci, d_vals, m, K, d_b),
                _C.spmm_csr(d_rp, d_ci, d_vals[:, 0].contiguous(), m, K, d_b), "H=1 spmm")
    assert_same(_C.sddmm_csr_heads(d_rp, d_ci, d_a, d_b, 1)[:, 0],
                _C.sddmm_csr(d_rp, d_ci, d_a, d_b, m, K), "H=1 sddmm")


def check_op_layer(dev):
    import pytest
    h, d = 3, 5
    rp, ci, vals, b, a = problem(h, d, "f32")
    m, n, nnz = rp.numel() - 1, h * d, ci.numel()
    d_rp, d_ci, d_vals, d_b, d_a = to_dev(dev, rp, ci, vals, b, a)
    want = ops.spmm_csr_heads(d_rp, d_ci, d_vals, d_b, m, K, h)
    want_sd = ops.sddmm_csr_heads(d_rp, d_ci, d_a, d_b, m, K, h)
    assert_same(_C.spmm_csr_heads(d_rp, d_ci, d_vals, m, K, d_b), want, "op vs C-ABI (spmm)")
    assert_same(_C.sddmm_csr_heads(d_rp, d_ci, d_a, d_b, h), want_sd, "op vs C-ABI (sddmm)")
    # out= is honoured (a row-strided out for the SpMM)
    buf = sentinel((m, n + PAD), b.dtype, dev)
    res = _C.spmm_csr_heads(d_rp, d_ci, d_vals, m, K, d_b, out=buf[:, :n])
    assert res.data_ptr() == buf.data_ptr()
    assert_same(buf[:, :n], want, "out= (spmm)")
    assert bool(is_sentinel(buf[:, n:]).all())
    sd = sentinel((nnz, h), b.dtype, dev)
    assert _C.sddmm_csr_heads(d_rp, d_ci, d_a, d_b, h, out=sd) is sd
    assert_same(sd, want_sd, "out= (sddmm)")
    # the public 3-D entry points
    b3, a3 = d_b.view(K, h, d), d_a.view(m, h, d)
    assert_same(flow_spmm.spmm(d_rp, d_ci, d_vals, m, K, b3).reshape(m, n), want, "spmm 3-D")
    assert_same(flow_spmm.sddmm(d_rp, d_ci, a3, b3), want_sd, "sddmm 3-D")
    assert_same(flow_spmm.spmm(d_rp, d_ci, d_vals, m, K, b3, static_csr=1).reshape(m, n), want,
                "spmm 3-D static_csr")
    o3 = torch.empty((m, h, d), dtype=b.dtype, device=dev)
    assert flow_spmm.spmm(d_rp, d_ci, d_vals, m, K, b3, out=o3) is o3
    assert_same(o3.view(m, n), want, "spmm 3-D out=")
    # errors
    with pytest.raises(RuntimeError, match="multiple"):
        _C.spmm_csr_heads(d_rp, d_ci, d_vals[:, :2].contiguous(), m, K, d_b)   # 15 % 2
    with pytest.raises(RuntimeError, match="multiple"):
        _C.sddmm_csr_heads(d_rp, d_ci, d_a, d_b, 4)
    with pytest.raises(RuntimeError, match="nnz"):
        _C.spmm_csr_heads(d_rp, d_ci, d_vals[:-1], m, K, d_b)
    with pytest.raises(TypeError, match="equal to b"):
        _C.spmm_csr_heads(d_rp, d_ci, d_vals.double(), m, K, d_b)
    with pytest.raises(TypeError, match="equal to b"):
        _C.sddmm_csr_heads(d_rp, d_ci, d_a.half(), d_b, h)
    with pytest.raises(TypeError, match="dtype of a_csr_row_ptr"):
        _C.spmm_csr_heads(d_rp, d_ci.long(), d_vals, m, K, d_b)
    with pytest.raises(ValueError, match="sum"):
        flow_spmm.spmm(d_rp, d_ci, d_vals, m, K, b3, reduce="max")
    with pytest.raises(RuntimeError, match="out="):
        flow_spmm.spmm(d_rp, d_ci, d_vals.clone().requires_grad_(True), m, K, b3, out=o3)
    # the op's own inference (the functional entry, past the binding's checks)
    import ctypes
    from oneflow_spmm._lib import LIB, OFX_EINVAL
    bad = d_vals[:, :2].contiguous()
    descs = [_C.desc(t) for t in (d_rp, d_ci, bad, d_b)]
    size = ctypes.c_size_t(0)
    rc = LIB.ofx_functional_spmm_csr_heads(None, *(ctypes.byref(x) for x in descs), m, K, None,
                                           None, 0, ctypes.byref(size))
    assert rc == OFX_EINVAL and "multiple" in flow_spmm._lib.last_error()
    for bad_opts in (options(planned=True), ops.make_options(variant=1)):
        with pytest.raises(flow_spmm.OfxError, match="not supported"):
            ops.spmm_csr_heads(d_rp, d_ci, d_vals, d_b, m, K, h, options=bad_opts)


# ---- autograd -------------------------------------------------------------------------------------
def grad_problem(dtype, h=3, d=5, seed=5):
    rng = np.random.default_rng(seed)
    lens = [3, 1, 0, 5, 2, 12, 4, 1, 7, 2, 3, 6]
    rp, ci, _ = random_csr(12, 12, lens, rng)
    mk = lambda *s: torch.from_numpy(rng.uniform(-1, 1, size=s)).to(dtype)  # noqa: E731
    return rp, ci, mk(ci.numel(), h), mk(12, h, d), mk(12, h, d)


def check_gradcheck(dev):
    rp, ci, vals, b, a = grad_problem(torch.float64)
    d_rp, d_ci = to_dev(dev, rp, ci)
    v, bb, aa = (t.to(dev).requires_grad_(True) for t in (vals, b, a))
    assert torch.autograd.gradcheck(lambda x, y: flow_spmm.spmm(d_rp, d_ci, x, 12, 12, y), (v, bb))
    assert torch.autograd.gradcheck(lambda x, y: flow_spmm.sddmm(d_rp, d_ci, x, y), (aa, bb))


def check_grads_match_loop(dev):
    """f32 gradients of the multi-head functions = those of the per-head loop through the
    single-head functions, bit for bit (no sum crosses heads)."""
    rp, ci, vals, b, a = grad_problem(torch.float32)
    h = b.shape[1]
    d_rp, d_ci = to_dev(dev, rp, ci)
    rng = np.random.default_rng(9)
    w = torch.from_numpy(rng.uniform(-1, 1, size=(12, h, 5))).float().to(dev)
    we = torch.from_numpy(rng.uniform(-1, 1, size=(ci.numel(), h))).float().to(dev)
    v1, b1, a1, v2, b2, a2 = (t.clone().to(dev).requires_grad_(True)
                              for t in (vals, b, a, vals, b, a))
    out = flow_spmm.spmm(d_rp, d_ci, v1, 12, 12, b1)
    loop = torch.stack([flow_spmm.spmm(d_rp, d_ci, v2[:, i].contiguous(), 12, 12,
                                       b2[:, i, :].contiguous()) for i in range(h)], dim=1)
    assert_same(out, loop, "spmm heads forward")
    (out * w).sum().backward()
    (loop * w).sum().backward()
    assert_same(v1.grad, v2.grad, "d(values)")
    assert_same(b1.grad, b2.grad, "d(b) of spmm")
    b1.grad = b2.grad = None
    e = flow_spmm.sddmm(d_rp, d_ci, a1, b1)
    e_loop = torch.stack([flow_spmm.sddmm(d_rp, d_ci, a2[:, i, :].contiguous(),
                                          b2[:, i, :].contiguous()) for i in range(h)], dim=1)
    assert_same(e, e_loop, "sddmm heads forward")
    (e * we).sum().backward()
    (e_loop * we).sum().backward()
    assert_same(a1.grad, a2.grad, "d(a)")
    assert_same(b1.grad, b2.grad, "d(b) of sddmm")


def check_attention_heads_f32(dev, h=3, d=5):
    """spmm(edge_softmax(sddmm(q, k)), v) with H = 3, D = 5 on attention_problem's graph in f32
    against the float64 dense reference per head: output and the three gradients within
    atol = 1e-5 (check_attention_f32's tolerance)."""
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
    e = flow_spmm.sddmm(d_rp, d_ci, ours[0], ours[1])
    assert tuple(e.shape) == (ci.numel(), h)
    out = flow_spmm.spmm(d_rp, d_ci, flow_spmm.edge_softmax(d_rp, d_ci, e), 12, 12, ours[2])
    assert tuple(out.shape) == (12, h, d)
    torch.testing.assert_close(out.detach().cpu().double(), ref.detach(), rtol=0, atol=1e-5)
    (out * w.float().to(dev)).sum().backward()
    for name, x, y in zip("qkv", ours, dense):
        torch.testing.assert_close(x.grad.cpu().double(), y.grad, rtol=0, atol=1e-5,
                                   msg=lambda s, n=name: f"d({n}): {s}")

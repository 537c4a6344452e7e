"""The checks of the multi-head SpMM over an FP8 feature table (op "spmm_csr_heads_fp8"), written
once for both devices (test_spmm_fp8_cpu.py runs them on host tensors, test_spmm_fp8_gpu.py on the
GPU, where every result is also compared with the kCPU entry's bits).  Every comparison is bit for
bit unless it says otherwise.

The reference is never the code under test: the contract's two tensors are restated in torch (Bd =
b_q.to(T), exact; V' = (values.float() * b_scale[col]).to(T), +0 scale for a column outside [0, K))
and fed to the EXISTING kCPU entry ops.spmm_csr_heads under the same options."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch

import oneflow_spmm as flow_spmm
from heads_cases import SCHEDULES, opts_of
from helpers import DTYPES, random_dense
from oneflow_spmm import _C, _lib, ops
from oneflow_spmm._C import current_stream_handle
from oneflow_spmm._lib import LIB, check
from reduce_cases import row_ranges
from reduce_helpers import PAD, assert_same, is_sentinel, options, padded, sentinel

M = 40
K = 2048
# LPR batches, the default hub split of 512 (513: one chunk, 1030: two), short rows under
# split=8 / chunk=4 / chunk=8 / ordered
LENGTHS = [0, 1, 2, 7, 8, 9, 63, 64, 65, 130, 513, 1030]
FORMATS = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
TYPES = ("f32", "bf16", "f16")
# one per step of the fast path's lane ladder (1, 4, 8, 16, 32, 64 lanes of 16 columns) ...
FAST_HD = [(1, 16), (4, 16), (8, 16), (16, 16), (8, 64), (16, 64)]
TILE_HD = (32, 64)  # ... and N = 2048: 128 lanes, a second column tile
GENERAL_HD = [(3, 5), (5, 1), (2, 4), (1, 24)]  # odd D, D < 16, D % 16 != 0
FILL = 0x7F  # a NaN code in both formats: what padding and unread rows hold


def grid(hds):
    return [(h, d, f, dt) for (h, d) in hds for f in FORMATS for dt in TYPES]


def codes(rng, shape, fmt):
    """Random bytes with the NaN codes (and e5m2's infinities) replaced by -0: every finite code
    occurs, subnormals and both zeros included."""
    c = rng.integers(0, 256, size=shape, dtype=np.uint8)
    bad = ((c & 0x7F) == 0x7F) if fmt == "e4m3" else ((c & 0x7F) >= 0x7C)
    c[bad] = 0x80
    return torch.from_numpy(c)


def scales(rng, k):
    """Positive f32 scales with full mantissas in [2^-8, 2^-2): f16 products of e5m2's largest
    codes stay finite."""
    return torch.from_numpy(np.exp2(rng.uniform(-8, -2, size=k)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def problem(h, d, fmt, dt, it="i32", lengths=None, m=M, k=K, seed=0, col_range=None):
    """(rp, ci, values [nnz, H], codes uint8 [K, H*D], scale f32 [K]) on the host; shared, never
    written.  Columns are drawn with repetition from [0, k), or from col_range = (lo, hi)."""
    rng = np.random.default_rng(seed + 1000 * h + d)
    idt = torch.int32 if it == "i32" else torch.int64
    lens = np.array(list(lengths) if lengths is not None
                    else [LENGTHS[r % len(LENGTHS)] for r in range(m)])
    rp = np.zeros(len(lens) + 1, dtype=np.int64)
    rp[1:] = np.cumsum(lens)
    lo, hi = col_range if col_range is not None else (0, k)
    ci = torch.from_numpy(rng.integers(lo, hi, size=int(rp[-1]))).to(idt)
    vals = random_dense(int(rp[-1]), h, rng, DTYPES[dt])
    return torch.from_numpy(rp).to(idt), ci, vals, codes(rng, (k, h * d), fmt), scales(rng, k)


def to_dev(dev, *ts):
    return tuple(t.to(dev) if t is not None else None for t in ts)


def pad_codes(c, pad, shift):
    """padded() for code bytes: leading dimension n + pad, `shift` bytes into the buffer, the rest
    holding FILL."""
    if pad == 0 and shift == 0:
        return c.contiguous()
    rows, n = c.shape
    flat = torch.full((rows * (n + pad) + shift,), FILL, dtype=torch.uint8, device=c.device)
    view = flat[shift:].view(rows, n + pad)[:, :n]
    view.copy_(c)
    return view


# ---- the contract's composition ---------------------------------------------------------------------
def ref_tensors(ci, vals, cq, scale, fmt):
    """(V', Bd) in the values' type."""
    k = cq.shape[0]
    bd = cq.view(FORMATS[fmt]).to(vals.dtype)
    if scale is None:
        return vals, bd
    c = ci.long()
    ok = (c >= 0) & (c < k)
    s = torch.where(ok, scale[c.clamp(0, max(k - 1, 0))], torch.zeros((), dtype=torch.float32))
    return (vals.float() * s[:, None]).to(vals.dtype), bd


def reference(rp, ci, vals, cq, scale, fmt, heads, opts=None, row_begin=0, row_end=None):
    """The existing kCPU multi-head SpMM on (rp, ci, V', Bd)."""
    vp, bd = ref_tensors(ci, vals, cq, scale, fmt)
    return ops.spmm_csr_heads(rp, ci, vp, bd, rp.numel() - 1, cq.shape[0], heads, options=opts,
                              row_begin=row_begin, row_end=row_end)


def run(dev, rp, ci, vals, cq, scale, fmt, heads, pad=0, shift=0, opts=None, row_begin=0,
        row_end=None, **kw):
    """The entry under test on `dev`; out starts as sentinels and its padding must keep them."""
    d_rp, d_ci, d_vals, d_cq, d_scale = to_dev(dev, rp, ci, vals, cq, scale)
    m, n = rp.numel() - 1, cq.shape[1]
    row_end = m if row_end is None else row_end
    out = padded(sentinel((row_end - row_begin, n), vals.dtype, dev), pad, shift)
    ops.spmm_csr_heads_fp8(d_rp, d_ci, d_vals, pad_codes(d_cq, pad, shift), d_scale, m, cq.shape[0],
                           heads, b_format=_C.FP8_FORMATS[FORMATS[fmt]], out=out, options=opts,
                           row_begin=row_begin, row_end=row_end, **kw)
    if pad:
        assert bool(is_sentinel(out._base[shift:].view(-1, n + pad)[:, n:]).all()), \
            "wrote into the padding"
    return out


def check_forward(dev, h, d, fmt, dt, it="i32", schedules=SCHEDULES, **kw):
    """With and without the scale, under every schedule, against the composition and (on the GPU)
    the kCPU entry; a base off the 16-byte alignment with a padded leading dimension (the general
    path) gives the aligned bits."""
    rp, ci, vals, cq, scale = problem(h, d, fmt, dt, it, **kw)
    for sc in (scale, None):
        for name in schedules:
            o = opts_of(name)
            what = f"H={h} D={d} {fmt} {dt} {it} {name} scale={'yes' if sc is not None else 'no'}"
            want = reference(rp, ci, vals, cq, sc, fmt, h, o)
            got = run(dev, rp, ci, vals, cq, sc, fmt, h, opts=o)
            assert_same(got, want, f"{what} vs spmm_csr_heads on (V', Bd)")
            if dev != "cpu":
                assert_same(got, run("cpu", rp, ci, vals, cq, sc, fmt, h, opts=o), f"{what} vs kCPU")
        got = run(dev, rp, ci, vals, cq, sc, fmt, h, pad=PAD, shift=1)
        assert_same(got, reference(rp, ci, vals, cq, sc, fmt, h), f"{what} unaligned")


def check_every_code(dev, fmt, dt):
    """All 256 codes through an identity CSR with values of one: the kernel's dequantisation is
    torch's conversion of the code to T for every finite code, which converts back to the code
    (the dequantisation is exact); NaN codes give NaN."""
    dtype = DTYPES[dt]
    rp = torch.arange(257, dtype=torch.int32)
    ci = torch.arange(256, dtype=torch.int32)
    cq = torch.arange(256, dtype=torch.int64).to(torch.uint8)[:, None].repeat(1, 16).contiguous()
    vals = torch.ones((256, 1), dtype=dtype)
    got = run(dev, rp, ci, vals, cq, None, fmt, 1).cpu()
    want = cq.view(FORMATS[fmt]).to(dtype)
    nan = torch.isnan(want.float())
    assert bool(torch.equal(torch.isnan(got.float()), nan)), "NaN codes"
    assert int(nan[:, 0].sum()) == (2 if fmt == "e4m3" else 6)
    summed = want.clone()
    summed[0x80] = 0.0  # the row's sum starts at +0: +0 + (1 * -0) is +0
    assert_same(torch.where(nan, torch.zeros_like(got), got),
                torch.where(nan, torch.zeros_like(want), summed), f"{fmt} codes in {dt}")
    back = want.to(FORMATS[fmt]).view(torch.uint8)
    assert bool(torch.equal(back[~nan], cq[~nan])), "a finite code is not exact in T"


def check_special_values(dev, fmt, dt):
    """The NaN codes, and e5m2's infinities, in one head of the B rows only one CSR row reads: NaN
    positions agree with the composition and every other element is bit-equal."""
    h, d = 4, 16
    rp, ci, vals, cq, scale = problem(h, d, fmt, dt, lengths=(3, 11, 0, 70, 5, 600), m=6, seed=7,
                                      col_range=(0, K - 80))
    ci, cq = ci.clone(), cq.clone()
    r, hh = 3, 2
    j0, j1 = int(rp[r]), int(rp[r + 1])
    own = torch.arange(K - 80, K - 80 + (j1 - j0))  # B rows that only row r reads
    ci[j0:j1] = own.to(ci.dtype)
    special = [0x7F, 0xFF] if fmt == "e4m3" else [0x7C, 0xFC, 0x7D, 0x7E, 0x7F, 0xFD, 0xFE, 0xFF]
    for i, row in enumerate(own.tolist()):
        cq[row, hh * d + (i % d)] = special[i % len(special)]
    for sc in (scale, None):
        for name in ("default", "split8"):
            o = opts_of(name)
            want = reference(rp, ci, vals, cq, sc, fmt, h, o)
            got = run(dev, rp, ci, vals, cq, sc, fmt, h, opts=o).cpu()
            nan_w, nan_g = torch.isnan(want.float()), torch.isnan(got.float())
            assert bool(torch.equal(nan_w, nan_g)), f"{fmt} {dt} {name}: NaN positions differ"
            assert bool(nan_w[r, hh * d:(hh + 1) * d].any())
            outside = nan_w.clone()
            outside[r, hh * d:(hh + 1) * d] = False
            assert not bool(outside.any()), "a special value left its head and row"
            zero = torch.zeros_like(want)
            assert_same(torch.where(nan_g, zero, got), torch.where(nan_w, zero, want),
                        f"{fmt} {dt} {name}: elements beside the NaNs")


def check_repeated_columns(dev, h, d, fmt, dt):
    """K = 37: far fewer columns than the long rows have nonzeros, so columns repeat in a row."""
    check_forward(dev, h, d, fmt, dt, k=37, seed=3, schedules=("default", "split8_chunk4"))


def check_columns_out_of_range(dev, fmt, dt):
    """Columns in [K, K + 8) read a zero row and the scale +0: the scale tensor is a view of a
    buffer whose next 8 elements are NaN, b_q's of one whose next rows hold NaN codes.  A negative
    column is refused by the kCPU kernel and reads as out of range on the GPU."""
    for h, d in ((4, 16), (3, 5)):
        k = 37
        rp, ci, vals, cq, scale = problem(h, d, fmt, dt, k=k, seed=4, col_range=(0, k + 8))
        assert bool((ci >= k).any())
        sbuf = torch.full((k + 8,), float("nan"))
        sbuf[:k] = scale
        cbuf = torch.full((k + 8, h * d), FILL, dtype=torch.uint8)
        cbuf[:k] = cq
        d_sbuf, d_cbuf = sbuf.to(dev), cbuf.to(dev)  # moved whole: the views keep their neighbours
        for sc, d_sc in ((scale, d_sbuf[:k]), (None, None)):
            want = reference(rp, ci, vals, cq, sc, fmt, h)
            assert not bool(torch.isnan(want.float()).any())
            got = run(dev, rp, ci, vals, d_cbuf[:k], d_sc, fmt, h)
            assert_same(got, want, f"columns >= K, H={h} D={d} {fmt} {dt}")
        neg = ci.clone()
        neg[ci >= k] = -3
        if dev == "cpu":
            with pytest.raises(flow_spmm.OfxError, match="negative column") as e:
                run(dev, rp, neg, vals, cq, scale, fmt, h)
            assert e.value.code == _lib.OFX_EINVAL
        else:
            assert_same(run(dev, rp, neg, vals, cq, scale, fmt, h),
                        reference(rp, ci, vals, cq, scale, fmt, h), "negative columns on the GPU")
    # K = 0: every column is out of range and b_q is empty
    rp, ci, vals, cq, scale = problem(2, 16, fmt, dt, seed=5, lengths=(3, 0, 9), m=3)
    got = run(dev, rp, ci, vals, cq[:0], scale[:0], fmt, 2)
    assert_same(got, torch.zeros_like(got), "K = 0: every product is a zero, every sum +0")


def check_row_ranges(dev, h, d, fmt, dt, schedule="split8"):
    """A range writes exactly its own rows: sentinels around and between stay untouched."""
    rp, ci, vals, cq, scale = problem(h, d, fmt, dt)
    m, n = rp.numel() - 1, h * d
    o = opts_of(schedule)
    full = reference(rp, ci, vals, cq, scale, fmt, h, o)
    d_rp, d_ci, d_vals, d_cq, d_scale = to_dev(dev, rp, ci, vals, cq, scale)
    for lo, hi in row_ranges(m):
        buf = sentinel((m + 2, n + PAD), vals.dtype, dev)
        out = buf[1:1 + hi - lo, :n]
        ops.spmm_csr_heads_fp8(d_rp, d_ci, d_vals, d_cq, d_scale, m, K, h,
                               b_format=_C.FP8_FORMATS[FORMATS[fmt]], out=out, row_begin=lo,
                               row_end=hi, options=o)
        assert_same(out, full[lo:hi], f"rows [{lo}, {hi})")
        kept = is_sentinel(buf)
        kept[1:1 + hi - lo, :n] = True
        assert bool(kept.all()), f"rows [{lo}, {hi}): wrote outside its rows"


def check_no_scale_identity(dev, fmt, dt):
    """spmm_fp8(values, b_q) is spmm(values, b_q.to(T)), 2-D with values [nnz] and 3-D."""
    rp, ci, vals, cq, _ = problem(4, 16, fmt, dt, seed=6)
    d_rp, d_ci, d_vals, d_cq = to_dev(dev, rp, ci, vals, cq)
    m = rp.numel() - 1
    bq = d_cq.view(FORMATS[fmt])
    b3 = bq.view(K, 4, 16)
    assert_same(flow_spmm.spmm_fp8(d_rp, d_ci, d_vals, m, K, b3),
                flow_spmm.spmm(d_rp, d_ci, d_vals, m, K, b3.to(vals.dtype)), "3-D")
    v1 = d_vals[:, 0].contiguous()
    got = flow_spmm.spmm_fp8(d_rp, d_ci, v1, m, K, bq)
    assert tuple(got.shape) == (m, 64)
    # the single-head op's schedule is resolved from N = 64 and the heads op's from D = 64: the same
    assert_same(got, flow_spmm.spmm(d_rp, d_ci, v1, m, K, bq.to(vals.dtype)), "2-D, values [nnz]")


# ---- quantize_rows_fp8 --------------------------------------------------------------------------------
def check_quantize(dev):
    rng = np.random.default_rng(11)
    # seeded log-spaced rows: magnitudes from 2^-20 to 2^20, both signs, and two all-zero rows
    mag = np.exp2(rng.uniform(-20, 20, size=(64, 1))) * np.exp2(rng.uniform(-6, 0, size=(64, 96)))
    b = torch.from_numpy((mag * rng.choice([-1.0, 1.0], size=mag.shape)).astype(np.float32))
    b[5] = 0
    b[17] = 0
    b = b.to(dev)
    for dtype, fmax, bound in ((torch.float8_e4m3fn, 448.0, 16.0), (torch.float8_e5m2, 57344.0,
                                                                   4096.0)):
        b_q, scale = flow_spmm.quantize_rows_fp8(b, dtype)
        assert b_q.dtype == dtype and tuple(b_q.shape) == tuple(b.shape)
        assert scale.dtype == torch.float32 and tuple(scale.shape) == (64,)
        amax = b.abs().amax(dim=1)
        assert bool(torch.equal(scale, torch.where(amax > 0, amax / fmax, torch.ones_like(amax))))
        for r in (5, 17):
            assert float(scale[r]) == 1.0 and not bool(b_q[r].view(torch.uint8).any())
        deq = b_q.float()
        assert bool(torch.isfinite(deq).all()), "a NaN or infinite code for finite input"
        err = ((deq * scale[:, None] - b).abs() / scale[:, None]).max()
        print(f"quantize_rows_fp8 {dtype}: max |dequant * scale - b| / scale = {float(err):.6g}")
        assert float(err) <= bound
    b3q, s3 = flow_spmm.quantize_rows_fp8(b.view(64, 6, 16))
    assert tuple(b3q.shape) == (64, 6, 16) and b3q.dtype == torch.float8_e4m3fn
    assert bool(torch.equal(s3, flow_spmm.quantize_rows_fp8(b)[1]))
    with pytest.raises(TypeError, match="float8"):
        flow_spmm.quantize_rows_fp8(b, torch.float16)


# ---- API and op layer -----------------------------------------------------------------------------------
def check_degenerate(dev, dt):
    """heads == 0, n == 0 and an empty row range write nothing; nnz == 0 writes +0 rows, as
    spmm_csr_heads does."""
    dtype = DTYPES[dt]
    rp, ci, vals, cq, scale = problem(1, 16, "e4m3", dt, seed=8)
    d_rp, d_ci, d_vals, d_cq, d_scale = to_dev(dev, rp, ci, vals, cq, scale)
    m = rp.numel() - 1
    fmt = _lib.FP8_E4M3
    out = sentinel((m, 16), dtype, dev)
    ops.spmm_csr_heads_fp8(d_rp, d_ci, d_vals, d_cq, d_scale, m, K, 1, b_format=fmt, out=out,
                           row_begin=2, row_end=2)
    assert bool(is_sentinel(out).all()), "an empty range writes nothing"
    none = ops.spmm_csr_heads_fp8(d_rp, d_ci, d_vals[:, :0], d_cq[:, :0], d_scale, m, K, 0,
                                  b_format=fmt)
    assert tuple(none.shape) == (m, 0)
    rp0 = torch.zeros(4, dtype=torch.int32, device=dev)
    z = ops.spmm_csr_heads_fp8(rp0, rp0[:0], d_vals[:0], d_cq, d_scale, 3, K, 1, b_format=fmt,
                               out=sentinel((3, 16), dtype, dev))
    assert not bool(z.view(torch.int16 if dtype != torch.float32 else torch.int32).any()), \
        "nnz == 0: every row is +0"
    bq = d_cq.view(torch.float8_e4m3fn)
    assert tuple(flow_spmm.spmm_fp8(rp0, rp0[:0], d_vals[:0, 0], 3, K, bq, d_scale).shape) == (3, 16)
    assert tuple(flow_spmm.spmm_fp8(rp0[:1], rp0[:0], d_vals[:0, 0], 0, K, bq).shape) == (0, 16)


def check_argument_checks(dev):
    """NULLs, sizes, leading dimensions, the format code, f64, planned / variant and a workspace
    that is too small return the documented code and launch nothing."""
    f32 = torch.float32
    rp = torch.tensor([0, 2, 3], dtype=torch.int32, device=dev)
    ci = torch.tensor([0, 1, 1], dtype=torch.int32, device=dev)
    vals = torch.ones((3, 2), dtype=f32, device=dev)
    cq = torch.full((2, 4), 0x38, dtype=torch.uint8, device=dev)  # 1.0 in e4m3
    scale = torch.ones(2, dtype=f32, device=dev)
    out = sentinel((2, 4), f32, dev)
    I, F, EINVAL = _lib.DT_INT32, _lib.DT_FLOAT, _lib.OFX_EINVAL
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    if dev == "cpu":
        entry = lambda *a, o=None: LIB.ofx_spmm_csr_heads_fp8_cpu(0, *a, o)  # noqa: E731
    else:
        s = current_stream_handle(vals)
        entry = lambda *a, o=None: LIB.ofx_spmm_csr_heads_fp8(  # noqa: E731
            s, *a, ws.data_ptr(), ws.numel(), o)
    ins = (rp.data_ptr(), ci.data_ptr(), vals.data_ptr(), cq.data_ptr())

    def f(fmt=_lib.FP8_E4M3, h=2, d=2, nnz=3, q=ins, sc=scale.data_ptr(), c=out.data_ptr(), rb=0,
          re=2, it=I, vt=F, k=2, ldb=4, ldc=4, o=None):
        return entry(it, vt, fmt, 2, k, h, d, nnz, q[0], q[1], q[2], q[3], ldb, sc, c, ldc, rb, re,
                     o=o)

    assert f(h=-1) == EINVAL and f(nnz=-3) == EINVAL and f(k=-1) == EINVAL
    assert f(rb=1, re=3) == EINVAL and f(rb=2, re=1) == EINVAL
    assert f(ldb=3) == EINVAL and f(ldc=3) == EINVAL
    for bad in (0, 3, -1, _lib.DT_FLOAT16):
        assert f(fmt=bad) == EINVAL, bad
    for i in range(4):
        assert f(q=ins[:i] + (None,) + ins[i + 1:]) == EINVAL, i
    assert f(c=None) == EINVAL
    assert f(vt=_lib.DT_DOUBLE) == _lib.OFX_EUNSUPPORTED
    assert f(vt=_lib.DT_INT64) == _lib.OFX_EUNSUPPORTED and f(it=F) == _lib.OFX_EUNSUPPORTED
    assert f(nnz=1 << 31) == EINVAL
    for bad in (options(planned=True), ops.make_options(variant=1)):
        assert f(o=ctypes.byref(bad)) == EINVAL
    broken = _lib.Options()
    broken.magic = 0
    assert f(o=ctypes.byref(broken)) == EINVAL
    assert f(rb=1, re=1) == _lib.OFX_OK and f(h=0, d=0, ldb=0, ldc=0) == _lib.OFX_OK
    size = ctypes.c_size_t(7)
    q = LIB.ofx_spmm_csr_heads_fp8_workspace_size
    assert q(I, F, 1, 2, 2, 2, 2, 3, None, None) == EINVAL
    assert q(I, F, 9, 2, 2, 2, 2, 3, None, ctypes.byref(size)) == EINVAL
    assert q(I, _lib.DT_DOUBLE, 1, 2, 2, 2, 2, 3, None, ctypes.byref(size)) == _lib.OFX_EUNSUPPORTED
    assert q(I, F, 1, 2, -2, 2, 2, 3, None, ctypes.byref(size)) == EINVAL
    bad = options(planned=True)
    assert q(I, F, 1, 2, 2, 2, 2, 3, ctypes.byref(bad), ctypes.byref(size)) == EINVAL
    # the query is the multi-head SpMM's for the same shapes
    for h, d, nnz in ((2, 8, 601), (4, 16, 5000), (1, 16, 3)):
        mine, theirs = ctypes.c_size_t(1), ctypes.c_size_t(2)
        check(q(I, F, 2, 40, K, h, d, nnz, None, ctypes.byref(mine)), "query")
        check(LIB.ofx_spmm_csr_heads_workspace_size(I, F, 40, K, h, d, nnz, None,
                                                    ctypes.byref(theirs)), "query")
        assert mine.value == theirs.value, (h, d, nnz)
    if dev != "cpu":  # a workspace one byte too small, or NULL, on a CSR whose rows need a plan
        rp2, ci2, v2, c2, s2 = to_dev(dev, *problem(2, 16, "e4m3", "f32"))
        m2, nnz2 = rp2.numel() - 1, ci2.numel()
        o2 = sentinel((m2, 32), f32, dev)
        need = ctypes.c_size_t(0)
        check(q(I, F, 1, m2, K, 2, 16, nnz2, None, ctypes.byref(need)), "query")
        assert 0 < need.value <= ws.numel()
        for wptr, wsize in ((None, 0), (None, need.value), (ws.data_ptr(), need.value - 1)):
            assert LIB.ofx_spmm_csr_heads_fp8(
                current_stream_handle(v2), I, F, 1, m2, K, 2, 16, nnz2, rp2.data_ptr(),
                ci2.data_ptr(), v2.data_ptr(), c2.data_ptr(), 32, s2.data_ptr(), o2.data_ptr(), 32,
                0, m2, wptr, wsize, None) == _lib.OFX_EWORKSPACE
        torch.cuda.synchronize()
        assert bool(is_sentinel(o2).all()), "an error launched"
    assert bool(is_sentinel(out).all()), "an error launched"
    assert f() == _lib.OFX_OK and f(sc=None, fmt=_lib.FP8_E5M2) == _lib.OFX_OK
    if dev != "cpu":
        torch.cuda.synchronize()
    assert not bool(is_sentinel(out).any())


def check_registrations():
    """The op for every value dtype x index type x device, with and without b_scale, through the
    tmp-size query of the functional entry (inference and kernel choice; nothing is launched, the
    descriptors carry NULL): one kernel matches and its tmp size is the workspace query's.  There
    is no double kernel."""
    m, k, nnz, heads, dd = 2, 4, 601, 2, 8
    n = heads * dd
    for dev in (-1, 0):
        for it in (_lib.DT_INT32, _lib.DT_INT64):
            def d(dtype, *shape):
                t = _lib.TensorDesc()
                t.dtype, t.device, t.ndim, t.data = dtype, dev, len(shape), None
                for i, s in enumerate(shape):
                    t.shape[i] = s
                    t.stride[i] = shape[1] if i == 0 and len(shape) == 2 else 1
                return ctypes.byref(t)
            rp, ci = d(it, m + 1), d(it, nnz)
            b, sc = d(_lib.DT_UINT8, k, n), d(_lib.DT_FLOAT, k)
            for vt in (_lib.DT_FLOAT, _lib.DT_FLOAT16, _lib.DT_BFLOAT16):
                want = ctypes.c_size_t(5)
                check(LIB.ofx_spmm_csr_heads_fp8_workspace_size(
                    it, vt, _lib.FP8_E5M2, m, k, heads, dd, nnz, None, ctypes.byref(want)), "query")
                assert want.value > 0
                for scale in (sc, None):
                    got = ctypes.c_size_t(1 << 40)
                    check(LIB.ofx_functional_spmm_csr_heads_fp8(
                        None, rp, ci, d(vt, nnz, heads), b, scale, m, k, _lib.FP8_E5M2, None, None,
                        0, ctypes.byref(got)), "tmp size")
                    assert got.value == (want.value if dev == 0 else 0), (dev, vt, it)
            got = ctypes.c_size_t(0)
            rc = LIB.ofx_functional_spmm_csr_heads_fp8(
                None, rp, ci, d(_lib.DT_DOUBLE, nnz, heads), b, sc, m, k, _lib.FP8_E4M3, None, None,
                0, ctypes.byref(got))
            assert rc != _lib.OFX_OK and "float, float16, bfloat16" in _lib.last_error()


def check_sbp():
    """One all-broadcast signature, with and without b_scale; the index inputs and the codes take
    no gradient."""
    for present, extra in (("", ()), ("b_scale", ("b_scale",))):
        s = _C.sbp_signatures("spmm_csr_heads_fp8", present)
        sigs, no_grad = s.split("|")
        assert len(sigs.split(";")) == 1, s
        want = {f"{v}:B" for v in ("a_csr_row_ptr", "a_csr_col_idx", "a_csr_values", "b", "out")
                + extra}
        assert set(sigs.split(",")) == want, s
        assert set(no_grad.split(":")[1].split(",")) == {"a_csr_row_ptr", "a_csr_col_idx", "b"}, s


def check_op_layer(dev):
    """The op through the registry dispatch and the public API against the C-ABI, and the
    refusals of the Python layer and of the op's own inference."""
    for fmt, dt, it, h, d in (("e4m3", "f32", "i32", 4, 16), ("e5m2", "bf16", "i64", 3, 5),
                              ("e4m3", "f16", "i32", 8, 16)):
        rp, ci, vals, cq, scale = p = problem(h, d, fmt, dt, it, lengths=(3, 0, 9, 40, 600), m=5,
                                              seed=9)
        m, n = 5, h * d
        d_rp, d_ci, d_vals, d_cq, d_scale = to_dev(dev, *p)
        bq = d_cq.view(FORMATS[fmt])
        for sc, d_sc in ((scale, d_scale), (None, None)):
            want = reference(rp, ci, vals, cq, sc, fmt, h)
            assert_same(_C.spmm_csr_heads_fp8(d_rp, d_ci, d_vals, m, K, bq, d_sc), want, "op")
            assert_same(flow_spmm.spmm_fp8(d_rp, d_ci, d_vals, m, K, bq.view(K, h, d), d_sc)
                        .reshape(m, n), want, "public 3-D")
        # out= is honoured (a row-strided out; a row-strided b_q is read in place)
        buf = sentinel((m, n + PAD), vals.dtype, dev)
        wide = pad_codes(d_cq, PAD, 0).view(FORMATS[fmt])
        res = _C.spmm_csr_heads_fp8(d_rp, d_ci, d_vals, m, K, wide, d_scale, out=buf[:, :n])
        assert res.data_ptr() == buf.data_ptr()
        assert_same(buf[:, :n], reference(rp, ci, vals, cq, scale, fmt, h), "out=")
        assert bool(is_sentinel(buf[:, n:]).all())
        o3 = torch.empty((m, h, d), dtype=vals.dtype, device=dev)
        assert flow_spmm.spmm_fp8(d_rp, d_ci, d_vals, m, K, bq.view(K, h, d), d_scale, out=o3) is o3
        assert_same(o3.view(m, n), reference(rp, ci, vals, cq, scale, fmt, h), "public out=")
    with pytest.raises(TypeError, match="float8"):
        flow_spmm.spmm_fp8(d_rp, d_ci, d_vals, m, K, d_cq)
    with pytest.raises(TypeError, match="float8"):
        _C.spmm_csr_heads_fp8(d_rp, d_ci, d_vals, m, K, bq.to(torch.float16))
    with pytest.raises(TypeError, match="float, float16, bfloat16"):
        _C.spmm_csr_heads_fp8(d_rp, d_ci, d_vals.double(), m, K, bq)
    with pytest.raises(RuntimeError, match="multiple"):
        _C.spmm_csr_heads_fp8(d_rp, d_ci, d_vals[:, :3].contiguous(), m, K, bq)  # 128 % 3
    with pytest.raises(RuntimeError, match="nnz"):
        _C.spmm_csr_heads_fp8(d_rp, d_ci, d_vals[:-1], m, K, bq)
    with pytest.raises(RuntimeError, match="b_scale"):
        _C.spmm_csr_heads_fp8(d_rp, d_ci, d_vals, m, K, bq, d_scale[:-1])
    with pytest.raises(RuntimeError, match="b_scale"):
        _C.spmm_csr_heads_fp8(d_rp, d_ci, d_vals, m, K, bq, d_scale.double())
    with pytest.raises(TypeError, match="dtype of a_csr_row_ptr"):
        _C.spmm_csr_heads_fp8(d_rp, d_ci.long(), d_vals, m, K, bq)
    with pytest.raises(RuntimeError, match=r"\[nnz, H\]"):
        flow_spmm.spmm_fp8(d_rp, d_ci, d_vals[:, 0], m, K, bq.view(K, h, d))
    with pytest.raises(RuntimeError, match="out="):
        flow_spmm.spmm_fp8(d_rp, d_ci, d_vals.clone().requires_grad_(True), m, K,
                           bq.view(K, h, d), out=o3)
    # the op's own inference (the functional entry, past the binding's checks)
    size = ctypes.c_size_t(0)
    descs = [ctypes.byref(_C.desc(t)) for t in (d_rp, d_ci, d_vals)]
    bdesc = ctypes.byref(_C._codes_desc(bq))
    for kw, word in ((dict(fmt=7), "b_format"), (dict(k=K + 1), "a_num_cols rows"),
                     (dict(scale=d_scale[:-1]), "b_scale")):
        sc = kw.get("scale", d_scale)
        rc = LIB.ofx_functional_spmm_csr_heads_fp8(
            None, *descs, bdesc, ctypes.byref(_C.desc(sc)), m, kw.get("k", K), kw.get("fmt", 1),
            None, None, 0, ctypes.byref(size))
        assert rc == _lib.OFX_EINVAL and word in _lib.last_error(), _lib.last_error()
    for bad_opts in (options(planned=True), ops.make_options(variant=1)):
        with pytest.raises(flow_spmm.OfxError, match="not supported"):
            ops.spmm_csr_heads_fp8(d_rp, d_ci, d_vals, d_cq, d_scale, m, K, h, b_format=1,
                                   options=bad_opts)


# ---- autograd -----------------------------------------------------------------------------------------
def ref_public(rp, ci, vals, bq3, scale):
    """The reference composition through torch autograd and the existing `spmm`: differentiable
    in vals (f32: V' is the f32 product itself)."""
    k = bq3.shape[0]
    c = ci.long()
    ok = (c >= 0) & (c < k)
    s = torch.where(ok, scale[c.clamp(0, k - 1)], torch.zeros((), device=scale.device))
    return flow_spmm.spmm(rp, ci, vals * s[:, None], rp.numel() - 1, k, bq3.to(vals.dtype))


def check_autograd(dev, fmt):
    """d(values) in f32 is bit-equal to torch autograd through the reference composition, for a
    3-D and a 2-D b_q, columns outside [0, K) included; b_q and b_scale get no gradient."""
    h, d, k = 3, 5, 37
    rp, ci, vals, cq, scale = problem(h, d, fmt, "f32", lengths=(3, 1, 0, 5, 40, 600), m=6, k=k,
                                      seed=12, col_range=(0, k + 3))
    d_rp, d_ci, d_vals, d_cq, d_scale = to_dev(dev, rp, ci, vals, cq, scale)
    bq3 = d_cq.view(FORMATS[fmt]).view(k, h, d)
    g = torch.from_numpy(np.random.default_rng(13).uniform(-1, 1, (6, h, d)).astype(np.float32))
    g = g.to(dev)
    a = d_vals.clone().requires_grad_(True)
    out = flow_spmm.spmm_fp8(d_rp, d_ci, a, 6, k, bq3, d_scale)
    out.backward(g)
    b = d_vals.clone().requires_grad_(True)
    want = ref_public(d_rp, d_ci, b, bq3, d_scale)
    want.backward(g)
    assert_same(out.detach(), want.detach(), "forward under autograd")
    assert_same(a.grad, b.grad, f"d(values) {fmt} 3-D")
    # without a scale; 2-D b_q with values [nnz]
    a1 = d_vals[:, 0].clone().requires_grad_(True)
    bq2 = bq3.reshape(k, h * d)
    flow_spmm.spmm_fp8(d_rp, d_ci, a1, 6, k, bq2).backward(g.view(6, h * d))
    b1 = d_vals[:, 0].clone().requires_grad_(True)
    flow_spmm.spmm(d_rp, d_ci, b1, 6, k, bq2.float()).backward(g.view(6, h * d))
    assert tuple(a1.grad.shape) == (ci.numel(),)
    assert_same(a1.grad, b1.grad, f"d(values) {fmt} 2-D, no scale")
    s = d_scale.clone().requires_grad_(True)
    a2 = d_vals.clone().requires_grad_(True)
    flow_spmm.spmm_fp8(d_rp, d_ci, a2, 6, k, bq3, s).sum().backward()
    assert s.grad is None and a2.grad is not None


def check_needs_input_grad(dev, monkeypatch):
    """Nothing requires a gradient: no autograd node and no SDDMM; values alone does: one SDDMM."""
    rp, ci, vals, cq, scale = problem(2, 16, "e4m3", "f32", lengths=(3, 0, 9), m=3, seed=14)
    d_rp, d_ci, d_vals, d_cq, d_scale = to_dev(dev, rp, ci, vals, cq, scale)
    bq3 = d_cq.view(torch.float8_e4m3fn).view(K, 2, 16)
    calls = []
    real = _C.sddmm_csr_heads
    monkeypatch.setattr(_C, "sddmm_csr_heads", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    out = flow_spmm.spmm_fp8(d_rp, d_ci, d_vals, 3, K, bq3, d_scale)
    assert out.grad_fn is None
    a = d_vals.clone().requires_grad_(True)
    flow_spmm.spmm_fp8(d_rp, d_ci, a, 3, K, bq3, d_scale).sum().backward()
    assert len(calls) == 1 and a.grad is not None
    with torch.no_grad():
        assert flow_spmm.spmm_fp8(d_rp, d_ci, a, 3, K, bq3, d_scale).grad_fn is None
    assert len(calls) == 1


# ---- graph capture (GPU) --------------------------------------------------------------------------------
def check_graph_capture(h, d, fmt, dt):
    """The forward captured once and replayed on new values, codes and scales: the bits of the
    eager launch and of the kCPU entry."""
    dev = "cuda"
    first = problem(h, d, fmt, dt, seed=15)
    second = problem(h, d, fmt, dt, seed=16)
    rp, ci = first[0], first[1]
    assert bool(torch.equal(rp, second[0]))
    m, n, nnz = rp.numel() - 1, h * d, ci.numel()
    d_rp, = to_dev(dev, rp)
    st = [t.clone().to(dev) for t in first[1:]]  # ci, values, codes, scale
    out = torch.empty((m, n), dtype=st[1].dtype, device=dev)
    it, vt, f = _C.dtype_code(rp.dtype), _C.dtype_code(st[1].dtype), _C.FP8_FORMATS[FORMATS[fmt]]
    size = ctypes.c_size_t(0)
    check(LIB.ofx_spmm_csr_heads_fp8_workspace_size(it, vt, f, m, K, h, d, nnz, None,
                                                    ctypes.byref(size)), "query")
    ws = torch.empty(max(size.value, 1), dtype=torch.uint8, device=dev)

    def launch():
        check(LIB.ofx_spmm_csr_heads_fp8(
            current_stream_handle(out), it, vt, f, m, K, h, d, nnz, d_rp.data_ptr(),
            st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(), n, st[3].data_ptr(),
            out.data_ptr(), n, 0, m, ws.data_ptr(), ws.numel(), None), "spmm_csr_heads_fp8")

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for t, src in zip(st, second[1:]):
        t.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    captured = out.clone()
    launch()
    torch.cuda.synchronize()
    assert_same(captured, out, "replay vs eager")
    assert_same(captured, run("cpu", rp, *second[1:], fmt, h), "replay vs kCPU")
    assert_same(captured, reference(rp, *second[1:], fmt, h), "replay vs the composition")

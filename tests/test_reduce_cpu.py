"""max / min / mean aggregation of spmm (op "spmm_csr_reduce") on the CPU: the kCPU kernels, the
C-ABI's validation, the op layer and autograd, against numpy references written from the contract
in include/ofx_spmm.h (reduce_helpers.py, reduce_cases.py)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import oneflow_spmm as fs
from helpers import DTYPES, assert_bitwise, random_csr, random_dense
from oneflow_spmm import _C, _lib
from oneflow_spmm._lib import LIB
import reduce_cases as rc
from reduce_helpers import (PAD, assert_same, ref_extremum, ref_mean, run_grad_b, run_grad_values,
                            transpose_t)

DEV = "cpu"


@pytest.mark.parametrize("pad", [0, PAD])
@pytest.mark.parametrize("n", rc.WIDTHS)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_widths(dt, n, pad):
    rp, ci, vals, b, g = rc.base_problem(n, DTYPES[dt])
    rc.check_all(DEV, rp, ci, vals, b, g, rc.M, rc.K, pad=pad, what=f"{dt} n={n}")


@pytest.mark.parametrize("it", [torch.int32, torch.int64])
@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_dtypes(dt, it):
    rp, ci, vals, b, g = rc.base_problem(48, DTYPES[dt], idx_dtype=it, seed=3)
    rc.check_all(DEV, rp, ci, vals, b, g, rc.M, rc.K, what=f"{dt}")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_random_values(dt):
    # non-exact inputs: unique extrema, inexact products
    rp, ci, vals, b, g = rc.base_problem(33, DTYPES[dt], seed=5, exact=False)
    rc.check_all(DEV, rp, ci, vals, b, g, rc.M, rc.K, pad=PAD, what=f"random {dt}")


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_special_values(dt):
    rc.check_special(DEV, DTYPES[dt])


@pytest.mark.parametrize("dt,n", rc.WIDE_WIDTHS)
def test_wide_widths(dt, n):
    # the kCPU kernels at the widths of the GPU's test_wide_widths (its reference there)
    rp, ci, vals, b, g = rc.base_problem(n, DTYPES[dt])
    rc.check_all(DEV, rp, ci, vals, b, g, rc.M, rc.K, pad=PAD, what=f"wide {dt} n={n}")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_wide_random_values(dt):
    rp, ci, vals, b, g = rc.base_problem(1030, DTYPES[dt], seed=5, exact=False)
    rc.check_all(DEV, rp, ci, vals, b, g, rc.M, rc.K, pad=PAD, what=f"wide random {dt}")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_hub_tiny(dt):
    rc.check_hub_tiny(DEV, DTYPES[dt])


@pytest.mark.parametrize("dt,it", [("f64", torch.int32), ("f16", torch.int32),
                                   ("f32", torch.int64), ("f64", torch.int64)])
def test_hub_tiny_other_types(dt, it):
    rc.check_hub_tiny(DEV, DTYPES[dt], idx_dtype=it)


@pytest.mark.parametrize("n", [16, 128, 256])
def test_hub_default_schedule(n):
    rc.check_hub_default(DEV, torch.float32, n)


def test_binned_work_list_shape():
    rp, ci, vals, b, g, m, k = rc.binned_problem(torch.float32)
    rc.check_all(DEV, rp, ci, vals, b, g, m, k, what="binned")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_row_ranges(dt):
    rc.check_row_ranges(DEV, DTYPES[dt])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_gradient_row_ranges(dt):
    rc.check_gradient_row_ranges(DEV, DTYPES[dt])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_hub_row_ranges(dt):
    rc.check_hub_ranges(DEV, DTYPES[dt])


@pytest.mark.parametrize("it", [torch.int32, torch.int64])
@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_row_scale_out_of_place_range(dt, it):
    rc.check_row_scale(DEV, DTYPES[dt], it)


def test_degenerate_sizes():
    rc.check_degenerate(DEV, torch.float32)


# ---- properties -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_one_nonzero_per_row_equals_sum(dt):
    dtype = DTYPES[dt]
    rng = np.random.default_rng(2)
    m, k, n = 50, 30, 24
    rp, ci, vals = random_csr(m, k, rng.integers(0, 2, size=m), rng, val_dtype=dtype)
    b, g = random_dense(k, n, rng, dtype), random_dense(m, n, rng, dtype)
    s = fs.spmm(rp, ci, vals, m, k, b)
    d_b_sum = fs.autograd.TRANSPOSE_CACHE.grad_b(rp, ci, vals, m, k, g)
    d_v_sum = fs.sddmm(rp, ci, g, b)
    rp_t, ci_t, perm = transpose_t(rp, ci, k)
    for red in ("max", "min", "mean"):
        out, arg = fs.spmm_reduce(rp, ci, vals, m, k, b, red)
        assert_same(out, s, f"{red} == sum")
        if red != "mean":
            assert_same(run_grad_b(rp_t, ci_t, perm, vals, arg, g, m, k), d_b_sum, f"{red} d(b)")
            assert_same(run_grad_values(rp, ci, arg, g, b, m, k), d_v_sum, f"{red} d(values)")
    # mean's backward: the row scale by degree 1 (or 0) leaves g (or +0), then the sum backward
    vv, bb = vals.clone().requires_grad_(), b.clone().requires_grad_()
    fs.spmm(rp, ci, vv, m, k, bb, reduce="mean").backward(g)
    deg = torch.diff(rp).bool()[:, None]
    gz = torch.where(deg, g, torch.zeros_like(g))
    assert_same(bb.grad, fs.autograd.TRANSPOSE_CACHE.grad_b(rp, ci, vals, m, k, gz), "mean d(b)")
    assert_same(vv.grad, fs.sddmm(rp, ci, gz, b), "mean d(values)")


# ---- op layer ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("red", ["max", "min", "mean", "sum"])
def test_op_global_form_rows_and_columns(red):
    rp, ci, vals, b, _ = rc.base_problem(20, torch.float32, seed=9)
    out, arg = _C.spmm_csr_reduce(rp, ci, vals, rc.M, rc.K, b, red)
    if red == "sum":
        assert_same(out, fs.spmm(rp, ci, vals, rc.M, rc.K, b), "sum forwards to spmm_csr")
    assert arg.shape == ((rc.M, 20) if red in ("max", "min") else (0, 20)) and arg.dtype == rp.dtype
    for parts in (1, 3, 7):
        outs, args = zip(*[_C.spmm_csr_reduce(rp, ci, vals, rc.M, rc.K, b, red,
                                              _parallel=(r, parts, 0)) for r in range(parts)])
        assert_same(torch.cat(outs), out, f"{red} S(0) x{parts}")
        assert_same(torch.cat(args), arg, f"{red} arg S(0) x{parts}: global nonzero indices")
    outs, args = zip(*[_C.spmm_csr_reduce(rp, ci, vals, rc.M, rc.K, b[:, lo:hi], red,
                                          _parallel=(r, 2, 1, 20))
                       for r, (lo, hi) in enumerate(((0, 10), (10, 20)))])
    assert_same(torch.cat(outs, dim=1), out, f"{red} S(1)")
    assert_same(torch.cat(args, dim=1), arg, f"{red} arg S(1)")


def test_op_registration_and_errors():
    sig = _C.sbp_signatures("spmm_csr_reduce")
    assert "out:S(0)" in sig and "arg:S(0)" in sig and "out:S(1)" in sig and "arg:S(1)" in sig
    assert sig.endswith("no_grad:a_csr_col_idx,a_csr_row_ptr")
    assert "out:S(1)" in _C.sbp_signatures("spmm_csr_reduce_grad_b")
    assert "out:P" in _C.sbp_signatures("spmm_csr_reduce_grad_values")
    rp, ci, vals, b, _ = rc.base_problem(4, torch.float32)
    with pytest.raises(_lib.OfxError, match="Dim K should be equal to b's dim0"):
        _C.spmm_csr_reduce(rp, ci, vals, rc.M, rc.K + 1, b, "max")
    with pytest.raises(TypeError, match="a_csr_values datatype should be equal to b"):
        _C.spmm_csr_reduce(rp, ci, vals.double(), rc.M, rc.K, b, "max")
    with pytest.raises(_lib.OfxError, match="a_num_rows \\+ 1"):
        _C.spmm_csr_reduce(rp[:-1], ci, vals, rc.M, rc.K, b, "min")


# ---- autograd ---------------------------------------------------------------------------------------
def _composition(rp, ci, vals, b, red):
    """The materialised composition in torch: values[:, None] * b[col], then a per-row reduce."""
    prod = vals[:, None] * b[ci.long()]
    rows = []
    for r in range(rp.numel() - 1):
        seg = prod[int(rp[r]):int(rp[r + 1])]
        if seg.shape[0] == 0:
            rows.append(torch.zeros(b.shape[1], dtype=b.dtype))
        elif red == "mean":
            rows.append(seg.sum(0) / seg.shape[0])
        else:
            rows.append(seg.max(0).values if red == "max" else seg.min(0).values)
    return torch.stack(rows), prod


@pytest.mark.parametrize("red", ["max", "min", "mean"])
def test_autograd_f64_against_composition(red):
    rng = np.random.default_rng(4)
    m, k, n = 7, 9, 5
    deg = np.array([3, 0, 5, 1, 9, 2, 4])
    rp, ci, vals = random_csr(m, k, deg, rng, val_dtype=torch.float64)
    b, g = random_dense(k, n, rng, torch.float64), random_dense(m, n, rng, torch.float64)
    v1, b1 = vals.clone().requires_grad_(), b.clone().requires_grad_()
    out, arg = fs.spmm_reduce(rp, ci, v1, m, k, b1, red)
    assert not arg.requires_grad and out.requires_grad
    out.backward(g)
    v2, b2 = vals.clone().requires_grad_(), b.clone().requires_grad_()
    ref, _ = _composition(rp, ci, v2, b2, red)
    ref.backward(g)
    assert torch.allclose(out.detach(), ref.detach(), rtol=1e-15, atol=0)
    # each gradient element is a sum of at most L terms added in another order than autograd's:
    # |diff| <= L * 2^-52 * sum |term|.  d(b)[kk, c]: the terms val[j] * g[r, c] of the nonzeros of
    # column kk (L <= m); d(values)[j]: the terms g[r, c] * b[col, c] (L <= n).  For the mean the
    # terms carry the factor 1 / deg_r.
    rows = torch.repeat_interleave(torch.arange(m), torch.diff(rp).long())
    scale = 1.0 / torch.diff(rp)[rows].double() if red == "mean" else torch.ones(len(rows)).double()
    term_b = (vals.abs() * scale)[:, None] * g[rows].abs()
    term_v = scale[:, None] * (g[rows] * b[ci.long()]).abs()
    bound_b = torch.zeros(k, n, dtype=torch.float64).index_add_(0, ci.long(), term_b) * m * 2.0 ** -52
    bound_v = term_v.sum(1) * n * 2.0 ** -52
    diff_b, diff_v = (b1.grad - b2.grad).abs(), (v1.grad - v2.grad).abs()
    print(f"{red}: max |d(b) diff| {diff_b.max():.3e}, max |d(values) diff| {diff_v.max():.3e}")
    assert (diff_b <= bound_b).all() and (diff_v <= bound_v).all()
    assert b1.grad.abs().sum() > 0 and v1.grad.abs().sum() > 0


def test_autograd_interface():
    rp, ci, vals, b, _ = rc.base_problem(6, torch.float32)
    bb = b.clone().requires_grad_()
    out, arg = fs.spmm_reduce(rp, ci, vals, rc.M, rc.K, bb, "max")
    assert out.requires_grad and not arg.requires_grad and arg.dtype == rp.dtype
    assert fs.spmm(rp, ci, vals, rc.M, rc.K, bb, reduce="min").requires_grad
    with pytest.raises(RuntimeError, match="out= is not supported"):
        fs.spmm(rp, ci, vals, rc.M, rc.K, bb, reduce="max", out=torch.empty(rc.M, 6))
    with pytest.raises(ValueError, match="reduce must be one of"):
        fs.spmm(rp, ci, vals, rc.M, rc.K, b, reduce="prod")
    # without grad, out= is filled in place; the default reduce is the op as it was
    dst = torch.empty(rc.M, 6)
    res = fs.spmm(rp, ci, vals, rc.M, rc.K, b, reduce="max", out=dst)
    assert res.data_ptr() == dst.data_ptr()
    assert_bitwise(dst, ref_extremum(rp, ci, vals, b, rc.K, "max")[0], "out=")
    assert_same(fs.spmm(rp, ci, vals, rc.M, rc.K, b, reduce="sum"),
                fs.spmm(rp, ci, vals, rc.M, rc.K, b), "reduce='sum' is spmm")
    assert_bitwise(fs.spmm(rp, ci, vals, rc.M, rc.K, b, reduce="mean"),
                   ref_mean(rp, ci, vals, b), "mean")


# ---- C-ABI validation -------------------------------------------------------------------------------
def test_abi_validation():
    rp, ci, vals, b, g = rc.base_problem(4, torch.float32)
    m, k, n, nnz = rc.M, rc.K, 4, ci.numel()
    out = torch.empty(m, n)
    arg = torch.empty(m, n, dtype=torch.int32)
    p = lambda t: t.data_ptr()  # noqa: E731
    F, I32 = _lib.DT_FLOAT, _lib.DT_INT32

    def reduce_cpu(reduce=_lib.REDUCE_MAX, ldarg=n, rb=0, re=m, idx=I32, nnz_=nnz, arg_=arg):
        return LIB.ofx_spmm_csr_reduce_cpu(0, idx, F, m, k, n, nnz_, p(rp), p(ci), p(vals), p(b), n,
                                           p(out), n, p(arg_) if arg_ is not None else None, ldarg,
                                           rb, re, reduce, None)

    assert reduce_cpu() == _lib.OFX_OK
    assert reduce_cpu(arg_=None) == _lib.OFX_OK  # arg may be NULL
    assert reduce_cpu(reduce=7) == _lib.OFX_EINVAL and "reduce" in _lib.last_error()
    assert reduce_cpu(reduce=-1) == _lib.OFX_EINVAL
    assert reduce_cpu(ldarg=n - 1) == _lib.OFX_EINVAL and "ldarg" in _lib.last_error()
    assert reduce_cpu(rb=3, re=2) == _lib.OFX_EINVAL and "row range" in _lib.last_error()
    assert reduce_cpu(re=m + 1) == _lib.OFX_EINVAL
    assert reduce_cpu(nnz_=2 ** 31) == _lib.OFX_EINVAL and "int32" in _lib.last_error()
    assert reduce_cpu(idx=_lib.DT_FLOAT) == _lib.OFX_EUNSUPPORTED
    size = ctypes.c_size_t(0)
    assert LIB.ofx_spmm_csr_reduce_workspace_size(I32, F, m, k, n, nnz, 9, None,
                                                  ctypes.byref(size)) == _lib.OFX_EINVAL
    # the device entries validate before they touch the device
    assert LIB.ofx_spmm_csr_reduce(None, I32, F, m, k, n, nnz, None, None, None, None, n, None, n,
                                   None, n, 0, m, 5, None, 0, None) == _lib.OFX_EINVAL
    # a gradient entry needs arg
    rp_t, ci_t, perm = transpose_t(rp, ci, k)
    db = torch.empty(k, n)
    sel = lambda a: LIB.ofx_spmm_csr_select_cpu(  # noqa: E731
        0, I32, F, m, k, n, nnz, p(rp_t), p(ci_t), p(perm), p(vals), a, n, p(g), n, p(db), n, 0, k,
        None)
    assert sel(p(arg)) == _lib.OFX_OK
    assert sel(None) == _lib.OFX_EINVAL and "arg is NULL" in _lib.last_error()
    dv = torch.empty(nnz)
    sd = lambda a, ld=n: LIB.ofx_sddmm_csr_select_cpu(  # noqa: E731
        0, I32, F, m, k, n, nnz, p(rp), p(ci), a, ld, p(g), n, p(b), n, p(dv), 0, m)
    assert sd(p(arg)) == _lib.OFX_OK
    assert sd(None) == _lib.OFX_EINVAL and "arg is NULL" in _lib.last_error()
    assert sd(p(arg), n - 1) == _lib.OFX_EINVAL
    assert LIB.ofx_row_scale_by_degree_cpu(0, I32, F, m, n, p(rp), p(out), n - 1, p(out), n, 0,
                                           m) == _lib.OFX_EINVAL
    with pytest.raises(_lib.OfxError) as e:
        _lib.check(LIB.ofx_functional_spmm_csr_reduce(None, None, None, None, m, k, None, 4, None,
                                                      None, None, 0, 0, 1, -1, -1, 0, None))
    assert e.value.code == _lib.OFX_EINVAL


def test_row_scale_in_place_and_strided():
    rp, ci, vals, b, g = rc.base_problem(7, torch.bfloat16)
    buf = torch.zeros(rc.M, 12, dtype=torch.bfloat16)
    buf[:, :7] = g
    view = buf[:, :7]
    ref = _C.row_scale_by_degree(rp, g)
    deg = torch.diff(rp).float()[:, None]
    want = torch.where(deg > 0, (g.float() / deg), torch.zeros(1)).to(torch.bfloat16)
    assert_same(ref, want, "row scale")
    _C.row_scale_by_degree(rp, view, out=view)  # in place, rows of stride 12
    assert_same(view.contiguous(), want, "row scale in place")
    assert not buf[:, 7:].any()

"""max / min / mean aggregation of spmm (op "spmm_csr_reduce") on the GPU: the HIP kernels
(forward extremum with arg, masked A^T SpMM, masked SDDMM, row scale) against the numpy references
and, bit for bit, against the kCPU kernels (reduce_cases.py)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import oneflow_spmm as fs
from helpers import DTYPES, assert_bitwise, random_csr, random_dense
from oneflow_spmm import _C
from oneflow_spmm._C import current_stream_handle, dtype_code
from oneflow_spmm._lib import LIB, check
import reduce_cases as rc
from reduce_helpers import (PAD, assert_same, options, ref_extremum, run_grad_b, run_grad_values,
                            run_reduce, transpose_t)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pad", [0, PAD])
@pytest.mark.parametrize("n", rc.WIDTHS)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_widths(device, dt, n, pad):
    rp, ci, vals, b, g = rc.base_problem(n, DTYPES[dt])
    rc.check_all(device, rp, ci, vals, b, g, rc.M, rc.K, pad=pad, what=f"{dt} n={n}")


@pytest.mark.parametrize("it", [torch.int32, torch.int64])
@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_dtypes(device, dt, it):
    rp, ci, vals, b, g = rc.base_problem(48, DTYPES[dt], idx_dtype=it, seed=3)
    rc.check_all(device, rp, ci, vals, b, g, rc.M, rc.K, what=f"{dt}")


@pytest.mark.parametrize("dt", ["f64", "f16"])
def test_column_tiles(device, dt):
    # f64 covers 128 columns per tile: 300 columns take three
    rp, ci, vals, b, g = rc.base_problem(300, DTYPES[dt], seed=6)
    rc.check_all(device, rp, ci, vals, b, g, rc.M, rc.K, pad=PAD, what=f"tiles {dt}")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_random_values(device, dt):
    rp, ci, vals, b, g = rc.base_problem(33, DTYPES[dt], seed=5, exact=False)
    rc.check_all(device, rp, ci, vals, b, g, rc.M, rc.K, pad=PAD, what=f"random {dt}")


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_special_values(device, dt):
    rc.check_special(device, DTYPES[dt])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_hub_tiny(device, dt):
    rc.check_hub_tiny(device, DTYPES[dt])


@pytest.mark.parametrize("n", [16, 128, 256])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_hub_default_schedule(device, dt, n):
    rc.check_hub_default(device, DTYPES[dt], n)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_binned_work_list(device, dt):
    # m >= kMinBinRows: the planner's binned work list (heavy rows first) with hub chunks
    rp, ci, vals, b, g, m, k = rc.binned_problem(DTYPES[dt])
    rc.check_all(device, rp, ci, vals, b, g, m, k, what="binned")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_row_ranges(device, dt):
    rc.check_row_ranges(device, DTYPES[dt])


def test_degenerate_sizes(device):
    rc.check_degenerate(device, torch.float32)


def test_planned_launch(device):
    """opts->planned: the workspace holds the plan ofx_spmm_csr_plan built with the same
    arguments; the launch skips its planner and gives the same out and arg."""
    rp, ci, vals, b, g, m, k = rc.binned_problem(torch.float32)
    d = rc.to_dev(device, rp, ci, vals, b)
    n, nnz = b.shape[1], ci.numel()
    it, vt = dtype_code(rp.dtype), dtype_code(b.dtype)
    want, want_arg = run_reduce(*d, m, k, "max")
    o = options()
    size = ctypes.c_size_t(0)
    check(LIB.ofx_spmm_csr_reduce_workspace_size(it, vt, m, k, n, nnz, 2, ctypes.byref(o),
                                                 ctypes.byref(size)))
    assert size.value > 0
    ws = torch.empty(size.value, dtype=torch.uint8, device=device)
    s = current_stream_handle(d[3])
    check(LIB.ofx_spmm_csr_plan(s, it, vt, m, k, n, nnz, d[0].data_ptr(), 0, m, ws.data_ptr(),
                                size.value, ctypes.byref(o)))
    o.planned = 1
    out = torch.empty((m, n), dtype=b.dtype, device=device)
    arg = torch.empty((m, n), dtype=rp.dtype, device=device)
    for _ in range(2):  # the plan stays valid across launches
        check(LIB.ofx_spmm_csr_reduce(s, it, vt, m, k, n, nnz, d[0].data_ptr(), d[1].data_ptr(),
                                      d[2].data_ptr(), d[3].data_ptr(), n, out.data_ptr(), n,
                                      arg.data_ptr(), n, 0, m, 2, ws.data_ptr(), size.value,
                                      ctypes.byref(o)))
        assert_same(out, want, "planned out")
        assert_same(arg, want_arg, "planned arg")
    check(LIB.ofx_device_error_check())


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_one_nonzero_per_row_equals_sum(device, dt):
    dtype = DTYPES[dt]
    rng = np.random.default_rng(2)
    m, k, n = 50, 30, 24
    rp, ci, vals = rc.to_dev(device, *random_csr(m, k, rng.integers(0, 2, size=m), rng,
                                                 val_dtype=dtype))
    b, g = rc.to_dev(device, random_dense(k, n, rng, dtype), random_dense(m, n, rng, dtype))
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


@pytest.mark.parametrize("red", ["max", "mean"])
def test_op_and_autograd_match_cpu(device, red):
    """The Python surface on GPU tensors: forward, arg and both gradients equal the CPU run's
    bits; the row split reproduces the single call."""
    rp, ci, vals, b, g = rc.base_problem(40, torch.float32, seed=12, exact=False)
    res = {}
    for dev in ("cpu", device):
        t = rc.to_dev(dev, rp, ci, vals, b, g)
        vv, bb = t[2].clone().requires_grad_(), t[3].clone().requires_grad_()
        out, arg = fs.spmm_reduce(t[0], t[1], vv, rc.M, rc.K, bb, red)
        assert not arg.requires_grad
        out.backward(t[4])
        res[str(dev)] = (out.detach(), arg, vv.grad, bb.grad)
        parts = [_C.spmm_csr_reduce(t[0], t[1], t[2], rc.M, rc.K, t[3], red,
                                    _parallel=(r, 3, 0)) for r in range(3)]
        assert_same(torch.cat([p[0] for p in parts]), out.detach(), "S(0) out")
        assert_same(torch.cat([p[1] for p in parts]), arg, "S(0) arg")
    for x, y, name in zip(res["cpu"], res[str(device)], ("out", "arg", "d(values)", "d(b)")):
        assert_same(y, x, f"{red} {name}: GPU vs CPU")
    if red == "max":
        assert_bitwise(res[str(device)][0], ref_extremum(rp, ci, vals, b, rc.K, "max")[0], "out")

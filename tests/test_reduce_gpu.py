"""max / min / mean aggregation of spmm (op "spmm_csr_reduce") on the GPU: the HIP kernels
(forward extremum with arg, masked A^T SpMM, masked SDDMM, row scale) against the numpy references
and, bit for bit, against the kCPU kernels (reduce_cases.py)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import oneflow_spmm as fs
from helpers import DTYPES, assert_bitwise, random_csr, random_dense, to_oracle
from oneflow_spmm import _C, _lib, ops
from oneflow_spmm._C import current_stream_handle, dtype_code
from oneflow_spmm._lib import LIB, check
import reduce_cases as rc
from reduce_helpers import (PAD, assert_same, is_sentinel, options, padding_of, poisoned,
                            ref_extremum, ref_grad_b, ref_mean, run_grad_b, run_grad_values,
                            run_reduce, sentinel, transpose_t)

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


# ---- the planned path (opts->planned) ----------------------------------------------------------------
I32, F32 = dtype_code(torch.int32), dtype_code(torch.float32)


def sum_form(m, k, n, nnz, lo=0, hi=None, opts=None):
    """The form ofx_spmm_csr takes for this launch.  The small form plans nothing: there
    ofx_spmm_csr_plan is a no-op and the consumers of a plan ignore opts->planned."""
    return ops.describe(m, k, n, nnz, torch.float32, torch.int32, row_begin=lo, row_end=hi,
                        options=opts)["form"]


def zeroed_workspace(device, query):
    size = ctypes.c_size_t(0)
    check(query(ctypes.byref(size)))
    assert size.value > 0
    return torch.zeros(size.value, dtype=torch.uint8, device=device)


def plan_rows(ws, rp_dev, rows, cols, n, nnz, lo, hi, opts):
    """ofx_spmm_csr_plan of rows [lo, hi) of the rows x cols CSR behind rp_dev into ws."""
    check(LIB.ofx_spmm_csr_plan(current_stream_handle(ws), I32, F32, rows, cols, n, nnz,
                                rp_dev.data_ptr(), lo, hi, ws.data_ptr(), ws.numel(),
                                ctypes.byref(opts)), "plan")


def assert_loud_once(what):
    """The launch before found no valid plan: OFX_EPLAN, reported once."""
    torch.cuda.synchronize()
    assert LIB.ofx_device_error_check() == _lib.OFX_EPLAN, f"{what}: no error reported"
    assert "no valid work-list plan" in _lib.last_error()
    assert LIB.ofx_device_error_check() == _lib.OFX_OK, f"{what}: reported twice"


def assert_quiet():
    torch.cuda.synchronize()
    check(LIB.ofx_device_error_check())


def check_planned_forward(device, name):
    """max / min / mean with opts->planned on a problem the sum op does not run in its small form:
    loud over a workspace never planned (the launch really reads the workspace's plan), and after
    ofx_spmm_csr_plan equal to the unplanned launch and to the reference, launch after launch."""
    rp, ci, vals, b, _, m, k = rc.planned_problem(name)
    n, nnz = b.shape[1], ci.numel()
    assert sum_form(m, k, n, nnz) != "small", "the planned path is not taken: pick a larger problem"
    d = rc.to_dev(device, rp, ci, vals, b)
    o_plan, o_run = options(), options(planned=True)
    ws = zeroed_workspace(device, lambda s: LIB.ofx_spmm_csr_reduce_workspace_size(
        I32, F32, m, k, n, nnz, _lib.REDUCE_MAX, ctypes.byref(o_plan), s))
    for red in ("max", "min"):
        want, want_arg = run_reduce(*d, m, k, red)
        ref_out, ref_arg = rc.planned_reference(name, red)
        assert_bitwise(want, ref_out, f"{name} {red} out")
        assert np.array_equal(to_oracle(want_arg).astype(np.int64), ref_arg), f"{name} {red} arg"
        for fill in (0, 0xA5):  # never planned
            ws.fill_(fill)
            out, arg = run_reduce(*d, m, k, red, opts=o_run, ws=ws)
            assert_loud_once(f"{name} {red} over a workspace of {fill:#x}")
            assert poisoned(out), f"{name} {red}: out is not the canonical NaN"
            assert bool((arg == -1).all()), f"{name} {red}: arg is not -1"
        plan_rows(ws, d[0], m, k, n, nnz, 0, m, o_plan)
        for _ in range(2):  # the plan stays valid across launches
            out, arg = run_reduce(*d, m, k, red, opts=o_run, ws=ws)
            assert_same(out, want, f"{name} planned {red} out")
            assert_same(arg, want_arg, f"{name} planned {red} arg")
        assert_quiet()
    mean, _ = run_reduce(*d, m, k, "mean")
    assert_bitwise(mean, ref_mean(rp, ci, vals, b), f"{name} mean")
    plan_rows(ws, d[0], m, k, n, nnz, 0, m, o_plan)
    assert_same(run_reduce(*d, m, k, "mean", opts=o_run, ws=ws)[0], mean, f"{name} planned mean")
    assert_quiet()


def test_planned_launch(device):
    """opts->planned: the workspace holds the plan ofx_spmm_csr_plan built with the same
    arguments; the launch skips its planner and gives the same out and arg.  On the mid-form
    problem, where the plan is read (the small form would plan for itself)."""
    check_planned_forward(device, "mid")


def test_planned_launch_many_rows(device):
    # m > 32768: a planned form's binned work list with hub chunks, 33 planner blocks
    check_planned_forward(device, "many-rows")


@pytest.mark.parametrize("name", ["mid", "many-rows"])
def test_planned_select(device, name):
    """d(b) with opts->planned over the plan ofx_spmm_csr_plan built of A^T (its k rows)."""
    rp, ci, vals, b, g, m, k = rc.planned_problem(name)
    n, nnz = b.shape[1], ci.numel()
    assert sum_form(m, k, n, nnz) != "small"
    # mid: A^T is planned too.  many-rows: A^T (2000 rows) is a small-form launch of the sum op, so
    # the plan entry is a no-op and the select must plan for itself whatever `planned` says.
    reads_plan = sum_form(k, m, n, nnz) != "small"
    assert reads_plan == (name == "mid")
    t = transpose_t(rp, ci, k)
    dt = rc.to_dev(device, *t)
    d_vals, d_g = rc.to_dev(device, vals, g)
    arg = torch.from_numpy(rc.planned_reference(name, "max")[1].astype(np.int32)).to(device)
    want = run_grad_b(*dt, d_vals, arg, d_g, m, k)
    assert_bitwise(want, rc.planned_reference_grad_b(name), f"{name} d(b)")
    o_plan, o_run = options(), options(planned=True)
    ws = zeroed_workspace(device, lambda s: LIB.ofx_spmm_csr_select_workspace_size(
        I32, F32, m, k, n, nnz, ctypes.byref(o_plan), s))
    if reads_plan:
        for fill in (0, 0xA5):  # never planned
            ws.fill_(fill)
            db = run_grad_b(*dt, d_vals, arg, d_g, m, k, opts=o_run, ws=ws)
            assert_loud_once(f"{name} d(b) over a workspace of {fill:#x}")
            assert poisoned(db), f"{name}: d(b) is not the canonical NaN"
    plan_rows(ws, dt[0], k, m, n, nnz, 0, k, o_plan)
    for _ in range(2):
        db = run_grad_b(*dt, d_vals, arg, d_g, m, k, opts=o_run, ws=ws)
        assert_same(db, want, f"{name} planned d(b)")
    assert_quiet()


def test_planned_row_range(device):
    """Rows [700, 2900) of the mid problem (the hub row 1000 inside, the hub row 100 outside),
    planned and launched as a range: the slice of the full result, arg in global indices.  The
    range's estimated share of nnz would be a small-form launch, which plans for itself; with
    range_nnz (an upper bound of the range's nonzeros) it is planned, and the hub tables hold rows
    local to the range."""
    rp, ci, vals, b, g, m, k = rc.planned_problem("mid")
    n, nnz, lo, hi = b.shape[1], ci.numel(), 700, 2900
    d = rc.to_dev(device, rp, ci, vals, b, g)
    forms = []
    for kw in ({}, {"range_nnz": nnz}):
        o_plan, o_run = options(**kw), options(planned=True, **kw)
        forms.append(sum_form(m, k, n, nnz, lo, hi, o_plan))
        ws = zeroed_workspace(device, lambda s: LIB.ofx_spmm_csr_reduce_workspace_size(
            I32, F32, m, k, n, nnz, _lib.REDUCE_MAX, ctypes.byref(o_plan), s))
        for red in ("max", "min"):
            full, full_arg = run_reduce(*d[:4], m, k, red)
            if forms[-1] != "small":
                ws.fill_(0xA5)  # never planned
                out, arg = run_reduce(*d[:4], m, k, red, row_begin=lo, row_end=hi, opts=o_run,
                                      ws=ws)
                assert_loud_once(f"{red} rows [{lo}, {hi}) never planned")
                assert poisoned(out) and bool((arg == -1).all())
            plan_rows(ws, d[0], m, k, n, nnz, lo, hi, o_plan)
            for _ in range(2):
                out, arg = run_reduce(*d[:4], m, k, red, row_begin=lo, row_end=hi, opts=o_run,
                                      ws=ws)
                assert_same(out, full[lo:hi], f"planned {red} rows [{lo}, {hi})")
                assert_same(arg, full_arg[lo:hi], f"planned {red} arg rows [{lo}, {hi})")
            assert_quiet()
    assert forms[1] != "small", "the planned path is not taken for the range"
    # d(values) of the range: the masked SDDMM's own plan cuts rows 1000 (inside) and 100 (outside)
    h_arg = full_arg.cpu()
    full_dv = run_grad_values(d[0], d[1], full_arg, d[4], d[3], m, k)
    assert_same(full_dv, run_grad_values(rp, ci, h_arg, g, b, m, k), "mid d(values) vs kCPU")
    dv = run_grad_values(d[0], d[1], full_arg, d[4], d[3], m, k, row_begin=lo, row_end=hi)
    rc.assert_values_range(dv, full_dv, to_oracle(rp).astype(np.int64), lo, hi, "mid")
    assert_quiet()


# ---- loud failures --------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _reset_knobs(device):
    LIB.ofx_device_error_check()
    yield
    LIB.ofx_debug_set(_lib.DEBUG_PLAN_SPIN_LIMIT, -1)
    torch.cuda.synchronize()
    LIB.ofx_device_error_check()


def test_failed_plan_is_loud_in_all_three_kernels(device):
    """OFX_DEBUG_PLAN_SPIN_LIMIT = 0 (the library's test hook: every planner block but the first
    gives up at once, nothing faults): the max forward, d(b) and d(values) each fill their output
    with the canonical NaN (arg with -1), leave the padding alone and report OFX_EPLAN once; with
    the knob restored the same calls are exact again."""
    rp, ci, vals, b, g, m, k = rc.planned_problem("many-rows")  # several planner blocks
    rpn = to_oracle(rp).astype(np.int64)
    d = rc.to_dev(device, rp, ci, vals, b, g)
    dt = rc.to_dev(device, *transpose_t(rp, ci, k))
    lo, hi = 5000, m

    def forward():
        return run_reduce(*d[:4], m, k, "max", pad=PAD)

    def grad_b(arg):
        return run_grad_b(*dt, d[2], arg, d[4], m, k, pad=PAD)

    def grad_values(arg, **kw):
        return run_grad_values(d[0], d[1], arg, d[4], d[3], m, k, pad=PAD, **kw)

    def reported_once(what):
        torch.cuda.synchronize()
        assert LIB.ofx_device_error_check() == _lib.OFX_EPLAN, f"{what}: no error reported"
        assert LIB.ofx_device_error_check() == _lib.OFX_OK, f"{what}: reported twice"

    good_out, good_arg = forward()
    ref_out, ref_arg = rc.planned_reference("many-rows", "max")
    assert_bitwise(good_out, ref_out, "out")
    assert np.array_equal(to_oracle(good_arg).astype(np.int64), ref_arg), "arg"
    good_db, good_dv = grad_b(good_arg), grad_values(good_arg)
    assert_bitwise(good_db, rc.planned_reference_grad_b("many-rows"), "d(b)")
    assert not bool(is_sentinel(good_dv).any())
    assert_quiet()

    assert LIB.ofx_debug_set(_lib.DEBUG_PLAN_SPIN_LIMIT, 0) == _lib.OFX_OK
    out, arg = forward()
    reported_once("forward")
    assert poisoned(out), "a failed plan's forward left output that is not the canonical NaN"
    assert bool((arg == -1).all()), "a failed plan's forward left an arg that is not -1"
    assert bool(is_sentinel(padding_of(out, PAD)).all()), "the poison reached out's padding"
    assert bool((padding_of(arg, PAD) == -7).all()), "the poison reached arg's padding"
    db = grad_b(good_arg)
    reported_once("d(b)")
    assert poisoned(db), "a failed plan's d(b) is not the canonical NaN"
    assert bool(is_sentinel(padding_of(db, PAD)).all())
    dv = grad_values(good_arg)
    reported_once("d(values)")
    assert poisoned(dv), "a failed plan's d(values) is not the canonical NaN"
    dv = grad_values(good_arg, row_begin=lo, row_end=hi)  # the launch's nonzeros, no others
    reported_once("d(values) of a row range")
    j0 = int(rpn[lo])
    assert poisoned(dv[j0:]) and bool(is_sentinel(dv[:j0]).all())

    assert LIB.ofx_debug_set(_lib.DEBUG_PLAN_SPIN_LIMIT, -1) == _lib.OFX_OK
    out, arg = forward()
    assert_same(out, good_out, "out after recovery")
    assert_same(arg, good_arg, "arg after recovery")
    assert_same(grad_b(arg), good_db, "d(b) after recovery")
    assert_same(grad_values(arg), good_dv, "d(values) after recovery")
    assert_quiet()


# ---- wide widths ----------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, PAD])
@pytest.mark.parametrize("dt,n", rc.WIDE_WIDTHS)
def test_wide_widths(device, dt, n, pad):
    rp, ci, vals, b, g = rc.base_problem(n, DTYPES[dt])
    rc.check_all(device, rp, ci, vals, b, g, rc.M, rc.K, pad=pad, what=f"wide {dt} n={n}")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_wide_random_values(device, dt):
    # inexact sums: the order of the four-leaves-per-lane tree and of the column tiles is numeric
    rp, ci, vals, b, g = rc.base_problem(1030, DTYPES[dt], seed=5, exact=False)
    rc.check_all(device, rp, ci, vals, b, g, rc.M, rc.K, pad=PAD, what=f"wide random {dt}")


def test_width_beyond_the_masked_sddmm(device):
    """n = 2049: the forward and d(b) tile over the columns and have no width limit; the device
    d(values) refuses (OFX_EUNSUPPORTED) before it launches: out untouched, no device error."""
    n, m = 2049, 14
    rp, ci, vals, b, g = rc.base_problem(n, torch.float32, m=m)
    d = rc.to_dev(device, rp, ci, vals, b, g)
    dt = rc.to_dev(device, *transpose_t(rp, ci, rc.K))
    for red in ("max", "min"):
        out, arg = run_reduce(*d[:4], m, rc.K, red)
        ref_out, ref_arg = ref_extremum(rp, ci, vals, b, rc.K, red)
        assert_bitwise(out, ref_out, f"n={n} {red} out")
        assert np.array_equal(to_oracle(arg).astype(np.int64), ref_arg), f"n={n} {red} arg"
        db = run_grad_b(*dt, d[2], arg, d[4], m, rc.K)
        assert_bitwise(db, ref_grad_b(rp, ci, vals, arg, g, rc.K), f"n={n} {red} d(b)")
    assert_quiet()
    out = sentinel((ci.numel(),), torch.float32, device)
    with pytest.raises(_lib.OfxError) as e:
        run_grad_values(d[0], d[1], arg, d[4], d[3], m, rc.K, out=out)
    assert e.value.code == _lib.OFX_EUNSUPPORTED and "n=2049" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool(is_sentinel(out).all()), "the refused call wrote to out"
    assert LIB.ofx_device_error_check() == _lib.OFX_OK
    # n = 2048 is the last width it takes (test_wide_widths[f32-2048])


# ---- row ranges of the gradient entries, hub chunks in the remaining types ---------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_gradient_row_ranges(device, dt):
    rc.check_gradient_row_ranges(device, DTYPES[dt])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_hub_row_ranges(device, dt):
    rc.check_hub_ranges(device, DTYPES[dt])


@pytest.mark.parametrize("dt,it", [("f64", torch.int32), ("f16", torch.int32),
                                   ("f32", torch.int64), ("f64", torch.int64)])
def test_hub_tiny_other_types(device, dt, it):
    # f64: partials of an 8-byte winner and an 8-byte arg; int64 indices through the hub kernels
    rc.check_hub_tiny(device, DTYPES[dt], idx_dtype=it)


def test_hub_default_schedule_f64(device):
    rc.check_hub_default(device, torch.float64, 128)


# ---- small ABI edges ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 17])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_null_arg(device, dt, n):
    """arg = NULL: nothing is written for it, out is the out of the call with arg (aligned and
    unaligned width; rows and hub chunks)."""
    rp, ci, vals, b, _ = rc.base_problem(n, DTYPES[dt], seed=14)
    hub = rc.hub_tiny_problem(DTYPES[dt])
    for (p_rp, p_ci, p_vals, p_b, m, k), o in (((rp, ci, vals, b, rc.M, rc.K), None),
                                               ((*hub[:4], *hub[5:]), options(split=8, chunk=4))):
        d = rc.to_dev(device, p_rp, p_ci, p_vals, p_b)
        for red in ("max", "min"):
            want, _ = run_reduce(*d, m, k, red, opts=o)
            out, arg = run_reduce(*d, m, k, red, opts=o, want_arg=False)
            assert arg is None
            assert_same(out, want, f"{red} out without arg")
            assert_bitwise(out, ref_extremum(p_rp, p_ci, p_vals, p_b, k, red)[0], f"{red} out")
    assert_quiet()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_unaligned_base_pointer(device, dt):
    """b, out and arg one element into their buffers, leading dimensions a multiple of 16 bytes
    (n = 16): not a lane's alignment, so the launch must take the element-wise kernels."""
    n = 16
    rp, ci, vals, b, _ = rc.base_problem(n, DTYPES[dt], seed=15)
    d = rc.to_dev(device, rp, ci, vals, b)
    for red in ("max", "min"):
        want, want_arg = run_reduce(*d, rc.M, rc.K, red)
        out, arg = run_reduce(*d, rc.M, rc.K, red, shift=1)
        assert out.data_ptr() % 16 and arg.data_ptr() % 16 and want.data_ptr() % 16 == 0
        assert_same(out, want, f"{red} out, shifted")
        assert_same(arg, want_arg, f"{red} arg, shifted")
        ref_out, ref_arg = ref_extremum(rp, ci, vals, b, rc.K, red)
        assert_bitwise(out, ref_out, f"{red} out")
        assert np.array_equal(to_oracle(arg).astype(np.int64), ref_arg), f"{red} arg"
        # the element in front of each view is not the kernel's
        assert bool(is_sentinel(out._base[:1]).all()) and int(arg._base[0]) == -7
    assert_quiet()


@pytest.mark.parametrize("it", [torch.int32, torch.int64])
@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_row_scale_out_of_place_range(device, dt, it):
    rc.check_row_scale(device, DTYPES[dt], it)


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

"""Multi-head SpMM / SDDMM (ops "spmm_csr_heads", "sddmm_csr_heads") on host tensors: the kCPU
kernels against the per-head loop of the single-head ops and the oracle bit for bit, the contract
pin of the per-head schedule, row ranges, the op layer, autograd, the multi-head attention layer,
and the kCPU kernels under the host sanitizers (heads_cases.py)."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest
import torch

import heads_cases as hc
from helpers import DTYPES, assert_bitwise, oracle_spmm, random_csr, random_dense
from oneflow_spmm import _C, _lib, ops
from oneflow_spmm._lib import LIB
from reduce_helpers import assert_same, options
from sanitize_helpers import CLANG, build_and_run


@pytest.mark.parametrize("it", ["i32", "i64"])
@pytest.mark.parametrize("h,d,dt", hc.HD_DT)
def test_spmm_matches_per_head_loop(h, d, dt, it):
    """Default schedule, split = chunk = 8 (many hubs at these sizes), split 8 / chunk 4 and
    ordered; inexact and exact data."""
    for exact in (False, True):
        hc.check_spmm("cpu", h, d, dt, it, exact)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_spmm_matches_oracle_per_head(dt):
    h, d = 4, 16
    rp, ci, vals, b, _ = hc.problem(h, d, dt)
    out = ops.spmm_csr_heads(rp, ci, vals, b, hc.M, hc.K, h)
    for i in range(h):
        ref = oracle_spmm(rp, ci, vals[:, i].contiguous(), hc.head(b, i, d).contiguous())
        assert_bitwise(hc.head(out, i, d).contiguous(), ref, f"head {i} vs oracle")


def test_schedule_is_a_function_of_d_not_of_n():
    """H = 8, D = 64, f32, inexact data, a 300-nonzero row.  default_split(64) = 512 leaves the row
    whole, so the default run equals the per-head op under default options; default_split(512) =
    128 would cut it, and a run forced to split = chunk = 128 differs in at least one bit."""
    h, d = 8, 64
    assert ops.default_split(d) == 512 and ops.default_split(h * d) == 128
    rng = np.random.default_rng(21)
    rp, ci, _ = random_csr(3, hc.K, [300, 5, 0], rng)
    vals = random_dense(ci.numel(), h, rng)
    b = random_dense(hc.K, h * d, rng)
    out = ops.spmm_csr_heads(rp, ci, vals, b, 3, hc.K, h)
    assert_same(out, hc.spmm_loop(rp, ci, vals, b, 3, hc.K, h), "default = per-head default")
    forced = ops.spmm_csr_heads(rp, ci, vals, b, 3, hc.K, h, options=options(split=128, chunk=128))
    assert_same(forced, hc.spmm_loop(rp, ci, vals, b, 3, hc.K, h, options(split=128, chunk=128)),
                "forced split = per-head forced split")
    assert not torch.equal(out[0].view(torch.int32), forced[0].view(torch.int32)), \
        "split = chunk = 128 changed no bit of the 300-nonzero row"
    assert_same(out[1:], forced[1:], "short rows")


@pytest.mark.parametrize("it", ["i32", "i64"])
@pytest.mark.parametrize("h,d,dt", hc.HD_DT)
def test_sddmm_matches_per_head(h, d, dt, it):
    for exact in (False, True):
        hc.check_sddmm("cpu", h, d, dt, it, exact)


@pytest.mark.parametrize("h,d,dt", [(3, 5, "f32"), (4, 16, "bf16"), (2, 4, "f64")])
def test_row_ranges(h, d, dt):
    hc.check_row_ranges("cpu", h, d, dt)


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_single_head_is_the_single_head_op(dt):
    hc.check_single_head("cpu", dt)


def test_op_layer():
    hc.check_op_layer("cpu")


def test_sbp_signatures():
    for op in ("spmm_csr_heads", "sddmm_csr_heads"):
        text = _C.sbp_signatures(op)
        assert "a_csr_row_ptr" in text and "S(" not in text, text  # all-broadcast only


def test_gradcheck():
    hc.check_gradcheck("cpu")


def test_gradients_match_per_head_loop():
    hc.check_grads_match_loop("cpu")


def test_attention_layer_heads_f32():
    hc.check_attention_heads_f32("cpu")


def test_edge_softmax_heads_is_the_per_column_op():
    import oneflow_spmm as flow_spmm
    rp, ci, vals, _, _ = hc.problem(3, 5, "f32")
    y = flow_spmm.edge_softmax(rp, ci, vals)
    assert tuple(y.shape) == tuple(vals.shape)
    for i in range(3):
        assert_same(y[:, i], _C.edge_softmax_csr(rp, ci, vals[:, i].contiguous()), f"head {i}")


def test_argument_checks():
    rp = torch.tensor([0, 2, 3], dtype=torch.int32)
    ci = torch.tensor([0, 1, 1], dtype=torch.int32)
    v = torch.ones(3, 2)
    b = torch.ones(2, 8)
    c = torch.empty(2, 8)
    I, F = _lib.DT_INT32, _lib.DT_FLOAT
    p = (rp.data_ptr(), ci.data_ptr(), v.data_ptr(), b.data_ptr(), 8, c.data_ptr(), 8)
    call = lambda *a, o=None: LIB.ofx_spmm_csr_heads_cpu(0, *a, o)  # noqa: E731
    assert call(I, F, 2, 2, 2, 4, 3, *p, 0, 2) == _lib.OFX_OK
    assert torch.equal(c, torch.tensor([[2.0] * 8, [1.0] * 8]))
    assert call(I, F, 2, 2, 2, 4, 3, *p, 1, 3) == _lib.OFX_EINVAL          # row range
    assert call(I, F, 2, 2, 2, 5, 3, *p, 0, 2) == _lib.OFX_EINVAL          # ldb < heads * d
    assert call(I, F, 2, 2, -1, 4, 3, *p, 0, 2) == _lib.OFX_EINVAL         # negative heads
    assert call(I, _lib.DT_INT64, 2, 2, 2, 4, 3, *p, 0, 2) == _lib.OFX_EUNSUPPORTED
    assert call(F, F, 2, 2, 2, 4, 3, *p, 0, 2) == _lib.OFX_EUNSUPPORTED
    for bad in (options(planned=True), ops.make_options(variant=1)):
        assert call(I, F, 2, 2, 2, 4, 3, *p, 0, 2, o=ctypes.byref(bad)) == _lib.OFX_EINVAL
        size = ctypes.c_size_t(0)
        assert LIB.ofx_spmm_csr_heads_workspace_size(I, F, 2, 2, 2, 4, 3, ctypes.byref(bad),
                                                     ctypes.byref(size)) == _lib.OFX_EINVAL
    out = torch.empty(3, 2)
    sd = lambda d, ld: LIB.ofx_sddmm_csr_heads_cpu(  # noqa: E731
        0, I, F, 2, 2, 2, d, 3, rp.data_ptr(), ci.data_ptr(), b.data_ptr(), ld, b.data_ptr(), ld,
        out.data_ptr(), 0, 2)
    assert sd(4, 8) == _lib.OFX_OK
    assert torch.equal(out, torch.full((3, 2), 4.0))
    assert sd(4, 7) == _lib.OFX_EINVAL
    assert sd(2049, 2 * 2049) == _lib.OFX_EUNSUPPORTED                     # the narrow range
    size = ctypes.c_size_t(7)
    assert LIB.ofx_sddmm_csr_heads_workspace_size(I, F, 2, 2, 4, 3, ctypes.byref(size)) == 0
    assert LIB.ofx_sddmm_csr_heads_workspace_size(I, F, 2, 2, 4, 3, None) == _lib.OFX_EINVAL


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not found")
def test_cpu_kernels_under_sanitizers(tmp_path):
    """The two kCPU kernels (spmm_heads_cpu.cpp with errors.cpp) built from source with
    AddressSanitizer + UndefinedBehaviorSanitizer and driven by tests/native/heads_sanitize.cpp,
    which also checks them against a naive loop.  Host code only: nothing is loaded into Python
    and nothing runs on the GPU."""
    build_and_run(tmp_path, "heads_sanitize", ["spmm_heads_cpu.cpp", "errors.cpp"])

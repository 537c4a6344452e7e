"""Multi-head SpMM / SDDMM (ops "spmm_csr_heads", "sddmm_csr_heads") on the MI355X: the HIP
kernels against the kCPU heads kernels and against the per-head loop of the single-head HIP
kernels, bit for bit (heads_cases.py): aligned and unaligned operands, default-schedule hubs, wide
rows, the binned work list, the SDDMM's fast and general paths, the workspace check and graph
capture."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import heads_cases as hc
import oneflow_spmm as flow_spmm
from helpers import DTYPES, power_law_degrees, random_csr, random_dense
from oneflow_spmm import _lib, ops
from reduce_helpers import PAD, assert_same, is_sentinel, sentinel

pytestmark = pytest.mark.gpu

HUB_LENGTHS = (3, 600, 0, 17, 1100, 64, 1700, 9)  # one, two and three chunks at split 512


@pytest.mark.parametrize("h,d,dt", hc.HD_DT)
def test_spmm_matrix(device, h, d, dt):
    """Every (H, D) and dtype under the four schedules, aligned; then a base shifted by one
    element and a padded leading dimension (the scalar path)."""
    hc.check_spmm(device, h, d, dt)
    hc.check_spmm(device, h, d, dt, exact=True, schedules=("default", "split8"), pad=PAD, shift=1)


@pytest.mark.parametrize("h,d,dt", [(3, 5, "f32"), (8, 16, "bf16"), (4, 16, "f64")])
def test_spmm_int64_indices(device, h, d, dt):
    hc.check_spmm(device, h, d, dt, "i64")
    hc.check_sddmm(device, h, d, dt, "i64")


@pytest.mark.parametrize("h,d,dt", [(8, 16, "f32"), (8, 32, "bf16")])
def test_spmm_default_schedule_hubs(device, h, d, dt):
    hc.check_spmm(device, h, d, dt, schedules=("default",), lengths=HUB_LENGTHS)
    hc.check_spmm(device, h, d, dt, schedules=("default",), lengths=HUB_LENGTHS, pad=PAD, shift=1)


@pytest.mark.parametrize("h,d,dt", [(8, 64, "f32"), (16, 64, "bf16")])
def test_spmm_wide(device, h, d, dt):
    """N = 512 in f32: two column tiles of the 64-lane group."""
    hc.check_spmm(device, h, d, dt, schedules=("default", "split8"), lengths=HUB_LENGTHS)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_spmm_many_rows(device, dt):
    """16,500 rows with power-law degrees of mean 3 and two long rows: the binned work list."""
    rng = np.random.default_rng(41)
    m, k, h, d = 16500, 4096, 4, 8
    deg = power_law_degrees(m, 3 * m, k, rng)
    deg[7], deg[9001] = 1300, 700
    rp, ci, _ = random_csr(m, k, deg, rng)
    vals = random_dense(ci.numel(), h, rng, DTYPES[dt])
    b = random_dense(k, h * d, rng, DTYPES[dt])
    a = random_dense(m, h * d, rng, DTYPES[dt])
    d_rp, d_ci, d_vals, d_b, d_a = hc.to_dev(device, rp, ci, vals, b, a)
    assert_same(ops.spmm_csr_heads(d_rp, d_ci, d_vals, d_b, m, k, h),
                ops.spmm_csr_heads(rp, ci, vals, b, m, k, h), "binned spmm heads vs kCPU")
    assert_same(ops.sddmm_csr_heads(d_rp, d_ci, d_a, d_b, m, k, h),
                ops.sddmm_csr_heads(rp, ci, a, b, m, k, h), "binned sddmm heads vs kCPU")


@pytest.mark.parametrize("h,d,dt", hc.HD_DT)
def test_sddmm_matrix(device, h, d, dt):
    """Fast path for (4,16), (8,16), (8,64), (16,64); general path for (3,5), (5,1), (2,4) and
    for every unaligned operand."""
    hc.check_sddmm(device, h, d, dt)
    hc.check_sddmm(device, h, d, dt, exact=True, pad=PAD, shift=1)


@pytest.mark.parametrize("h,d,dt", [(8, 16, "f32"), (3, 5, "f32"), (8, 32, "bf16")])
def test_sddmm_hub_row(device, h, d, dt):
    """A 1700-nonzero row: the hub chunks' per-nonzero outputs."""
    hc.check_sddmm(device, h, d, dt, lengths=HUB_LENGTHS)


@pytest.mark.parametrize("h,d,dt", [(3, 5, "f32"), (4, 16, "bf16")])
def test_row_ranges(device, h, d, dt):
    hc.check_row_ranges(device, h, d, dt)


def test_single_head(device):
    hc.check_single_head(device, "f32")
    hc.check_single_head(device, "bf16")


def test_op_layer(device):
    hc.check_op_layer(device)


def test_workspace_one_byte_short(device):
    """OFX_EWORKSPACE, and nothing is launched: the output keeps its sentinel."""
    import ctypes
    h, d = 8, 16
    rp, ci, vals, b, a = hc.problem(h, d, "f32", lengths=HUB_LENGTHS)
    m = rp.numel() - 1
    d_rp, d_ci, d_vals, d_b, d_a = hc.to_dev(device, rp, ci, vals, b, a)
    size = ctypes.c_size_t(0)
    I, F = _lib.DT_INT32, _lib.DT_FLOAT
    _lib.check(_lib.LIB.ofx_spmm_csr_heads_workspace_size(I, F, m, hc.K, h, d, ci.numel(), None,
                                                         ctypes.byref(size)), "ws")
    assert size.value > 0
    out = sentinel((m, h * d), torch.float32, device)
    with pytest.raises(flow_spmm.OfxError, match="workspace") as e:
        ops.spmm_csr_heads(d_rp, d_ci, d_vals, d_b, m, hc.K, h, out=out,
                           workspace_bytes=size.value - 1)
    assert e.value.code == _lib.OFX_EWORKSPACE
    _lib.check(_lib.LIB.ofx_sddmm_csr_heads_workspace_size(I, F, m, h, d, ci.numel(),
                                                          ctypes.byref(size)), "ws")
    assert size.value > 0
    sd = sentinel((ci.numel(), h), torch.float32, device)
    with pytest.raises(flow_spmm.OfxError, match="workspace") as e:
        ops.sddmm_csr_heads(d_rp, d_ci, d_a, d_b, m, hc.K, h, out=sd,
                            workspace_bytes=size.value - 1)
    assert e.value.code == _lib.OFX_EWORKSPACE
    torch.cuda.synchronize()
    assert bool(is_sentinel(out).all()) and bool(is_sentinel(sd).all())


def test_attention_layer_heads_f32(device):
    hc.check_attention_heads_f32(device)


def test_gradients_match_per_head_loop(device):
    hc.check_grads_match_loop(device)


@pytest.mark.graph_capture
def test_graph_capture_forward_and_gradients(device):
    """Forward and both gradients of both functions captured once, replayed on new values: the
    eager result."""
    h, d = 4, 16
    rp, ci, vals, b, _ = hc.problem(h, d, "f32", lengths=HUB_LENGTHS)
    m = rp.numel() - 1
    d_rp, d_ci = hc.to_dev(device, rp, ci)
    v = vals.to(device).requires_grad_(True)
    bb = b.to(device).view(hc.K, h, d).clone().requires_grad_(True)
    w = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, size=(m, h, d))).float().to(device)

    def step():
        out = flow_spmm.spmm(d_rp, d_ci, v, m, hc.K, bb)
        gv, gb = torch.autograd.grad((out * w).sum(), (v, bb))
        return out.detach(), gv, gb

    s = torch.cuda.Stream(device)
    s.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(s):
        step()  # warm (outside capture): the transpose cache, the allocator
    torch.cuda.current_stream(device).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = step()
    rng = np.random.default_rng(4)
    with torch.no_grad():
        v.copy_(random_dense(ci.numel(), h, rng).to(device))
        bb.copy_(random_dense(hc.K, h * d, rng).to(device).view(hc.K, h, d))
    g.replay()
    torch.cuda.synchronize()
    want = step()
    for name, x, y in zip(("out", "d(values)", "d(b)"), got, want):
        assert_same(x, y, f"graph replay {name}")

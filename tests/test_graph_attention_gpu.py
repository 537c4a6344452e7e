"""Fused multi-head graph attention (op "graph_attention_csr_heads", `oneflow_spmm.graph_attention`)
on the MI355X: the HIP kernel against the composition of the three HIP entries and against the kCPU
kernel, bit for bit (graph_attention_cases.py): every boundary length of the three phases, every
lane-group width of the launch rule, the fast and the general path, hub chunking, row ranges,
special values, the public API, autograd, graph capture and many short rows."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import graph_attention_cases as gc
import oneflow_spmm as flow_spmm
from helpers import DTYPES, power_law_degrees, random_csr, random_dense
from oneflow_spmm import ops
from reduce_helpers import assert_same

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("h,d,dt", gc.HD_DT)
def test_matrix(device, h, d, dt):
    """Every (H, D) and dtype over every boundary length, under the default schedule and the two
    that chunk short rows.  Fast path: (4,16), (8,16), (8,64), (16,64); general path: the others
    ((1,16) too: H is no multiple of the softmax's head vector).  Lane groups of 1 (bf16 / f16 with H*D <= 8), 4, 16, 32 and 64 lanes, and
    two leaves a lane at (16,64)."""
    gc.check_forward(device, h, d, dt, schedules=("default", "split8", "split8_chunk4"))


@pytest.mark.parametrize("h,d,dt", gc.HD_DT)
def test_general_path_of_unaligned_operands(device, h, d, dt):
    """A base shifted by one element and a padded leading dimension: the general path with the
    same bits."""
    gc.check_forward(device, h, d, dt, exact=True, schedules=("default", "split8"), pad=gc.PAD,
                     shift=1)


@pytest.mark.parametrize("h,d,dt", [(3, 5, "f32"), (8, 16, "bf16"), (4, 16, "f64"), (8, 16, "f32")])
def test_int64_indices(device, h, d, dt):
    gc.check_forward(device, h, d, dt, "i64", schedules=("default", "split8"))


def test_hub_schedule_comes_from_d(device):
    """H = 8, D = 64: a 300-nonzero row stays whole (the split of D = 64 is 512; that of
    H*D = 512 would be 128), next to rows that are cut."""
    gc.check_forward(device, 8, 64, "f32", lengths=(300, 3, 0, 513, 1100), k=1200)


@pytest.mark.parametrize("h,d,dt,k", [(8, 256, "f16", 320), (1, 520, "f32", 320),
                                      (2, 264, "bf16", 320)])
def test_four_leaves_a_lane(device, h, d, dt, k):
    """H*D = 2048 on the fast path and D = 520 / 264 (D/8 no power of two) on the general one: the
    64-lane group with four leaves a lane in phase 1 and column tiles in phase 3."""
    gc.check_forward(device, h, d, dt, schedules=("default", "split8"),
                     lengths=(0, 1, 9, 65, 130, 300), k=k)


@pytest.mark.parametrize("h,d,dt", [(3, 5, "f32"), (4, 16, "bf16"), (8, 16, "f32")])
def test_row_ranges(device, h, d, dt):
    gc.check_row_ranges(device, h, d, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_columns_out_of_range(device, dt):
    gc.check_columns_out_of_range(device, dt)


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_special_values_stay_in_their_head(device, dt):
    gc.check_special_confined(device, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_single_head_and_empty(device, dt):
    gc.check_single_head_and_empty(device, dt)


def test_public_api(device):
    gc.check_public_api(device)


def test_op_layer(device):
    gc.check_op_layer(device)


def test_argument_checks(device):
    gc.check_argument_checks(device)


def test_workspace_one_byte_short(device):
    """The workspace query is honoured: a buffer one byte short of it returns OFX_EWORKSPACE, and
    nothing is launched (the outputs keep their sentinels)."""
    import ctypes

    from oneflow_spmm import _lib
    from reduce_helpers import is_sentinel, sentinel
    h, d = 8, 16
    rp, ci, q, kk, v = gc.problem(h, d, "f32")
    m = rp.numel() - 1
    x = gc.to_dev(device, rp, ci, q, kk, v)
    size = ctypes.c_size_t(0)
    _lib.check(_lib.LIB.ofx_graph_attention_csr_heads_workspace_size(
        _lib.DT_INT32, _lib.DT_FLOAT, m, gc.K, h, d, ci.numel(), None, ctypes.byref(size)), "ws")
    assert size.value > 0  # hub rows: the planner's work list and the chunks' partials
    out = sentinel((m, h * d), torch.float32, device)
    attn = sentinel((ci.numel(), h), torch.float32, device)
    with pytest.raises(flow_spmm.OfxError, match="workspace") as e:
        ops.graph_attention_csr_heads(*x, m, gc.K, h, out=out, attn=attn,
                                      workspace_bytes=size.value - 1)
    assert e.value.code == _lib.OFX_EWORKSPACE
    torch.cuda.synchronize()
    assert bool(is_sentinel(out).all()) and bool(is_sentinel(attn).all())


@pytest.mark.parametrize("with_attn", [False, True])
@pytest.mark.parametrize("h,d", [(3, 5), (8, 16)])
def test_gradients_match_composed_layer(device, h, d, with_attn):
    gc.check_grads_match_composition(device, h, d, with_attn)


def test_only_requested_gradients(device):
    gc.check_needs_input_grad(device)


def test_gradcheck_f64(device):
    gc.check_gradcheck(device)


def test_dense_reference_f32(device):
    gc.check_dense_reference_f32(device)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_many_rows(device, dt):
    """6,000 rows with power-law degrees of mean 4 and two long rows at H = 8, D = 16: several
    workgroups on every CU, against the HIP composition and the kCPU kernel."""
    rng = np.random.default_rng(43)
    m, k, h, d = 6000, 4096, 8, 16
    deg = power_law_degrees(m, 4 * m, k, rng)
    deg[7], deg[4001] = 1300, 700
    rp, ci, _ = random_csr(m, k, deg, rng)
    q, kk, v = (random_dense(r, h * d, rng, DTYPES[dt]) for r in (m, k, k))
    x = gc.to_dev(device, rp, ci, q, kk, v)
    out, attn = ops.graph_attention_csr_heads(*x, m, k, h)
    want_out, want_attn = gc.compose(*x, m, k, h)
    assert_same(attn, want_attn, "many rows: attn vs composition")
    assert_same(out, want_out, "many rows: out vs composition")
    c_out, c_attn = ops.graph_attention_csr_heads(rp, ci, q, kk, v, m, k, h)
    assert_same(attn, c_attn, "many rows: attn vs kCPU")
    assert_same(out, c_out, "many rows: out vs kCPU")


@pytest.mark.graph_capture
def test_graph_capture_forward_and_backward(device):
    """Forward and backward captured once, replayed on new q, k, v: the bits of a fresh eager call
    and of the kCPU kernel."""
    h, d = 8, 16
    rp, ci, q, kk, v = gc.grad_graph(h, d)
    m = rp.numel() - 1
    d_rp, d_ci = gc.to_dev(device, rp, ci)
    x = tuple(t.clone().to(device).requires_grad_(True) for t in (q, kk, v))
    rng = np.random.default_rng(3)
    w = torch.from_numpy(rng.uniform(-1, 1, size=(m, h, d))).float()
    d_w = w.to(device)

    def step(rp_, ci_, ts, w_):
        out, attn = flow_spmm.graph_attention(rp_, ci_, *ts, return_attention=True)
        grads = torch.autograd.grad((out * w_).sum(), ts)
        return (out.detach(), attn.detach()) + tuple(grads)

    s = torch.cuda.Stream(device)
    s.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(s):
        step(d_rp, d_ci, x, d_w)  # warm (outside capture): the transpose cache, the allocator
    torch.cuda.current_stream(device).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = step(d_rp, d_ci, x, d_w)
    new = tuple(torch.from_numpy(rng.uniform(-1, 1, size=tuple(t.shape))).float() for t in x)
    with torch.no_grad():
        for t, n in zip(x, new):
            t.copy_(n.to(device))
    g.replay()
    torch.cuda.synchronize()
    want = step(d_rp, d_ci, x, d_w)
    cpu = step(rp, ci, tuple(n.clone().requires_grad_(True) for n in new), w)
    for name, a, b, c in zip(("out", "attn", "d(q)", "d(k)", "d(v)"), got, want, cpu):
        assert_same(a, b, f"graph replay {name} vs eager")
        assert_same(a, c, f"graph replay {name} vs kCPU")

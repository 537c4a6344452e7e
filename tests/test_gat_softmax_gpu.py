"""GAT attention weights (ops "gat_softmax_csr_heads" and its gradient) on the MI355X: the HIP
kernels of csrc/gat_softmax_heads.hip against the numpy restatement of the scores fed to the
existing multi-head edge softmax and against the kCPU entry, bit for bit (gat_softmax_cases.py):
every boundary row length, head counts of the packed and the general path, every lane-group width,
repeated columns, columns outside [0, K), unaligned bases, row ranges, the activation's edges,
special values, the public API, autograd, the op layer, the argument checks and graph capture."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import edge_softmax_heads_cases as hc
import gat_softmax_cases as gc
import oneflow_spmm as flow_spmm
from edge_softmax_cases import scores
from helpers import DTYPES
from oneflow_spmm import _C
from reduce_helpers import assert_same

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("it", [torch.int32, torch.int64])
@pytest.mark.parametrize("h,dt", hc.HEADS_DT)
def test_boundary_lengths_and_head_counts(device, h, dt, it):
    """LG = 64: rows in the wave's registers and rows swept in tiles; H % V == 0 takes the packed
    path, every other H the general one."""
    gc.check_boundaries(device, h, DTYPES[dt], it)


@pytest.mark.parametrize("h,dt", [(3, "f32"), (8, "f32"), (8, "bf16"), (5, "f16"), (2, "f64"),
                                  (3, "f64")])
@pytest.mark.parametrize("mix", list(hc.LG_MIXES))
def test_lane_group_mixes(device, mix, h, dt):
    """The launches whose mean degree picks 1, 4 and 16 lanes per (row, head group): most rows in
    their group's registers, the longer ones taken over by the wave."""
    gc.check_lane_groups(device, mix, h, DTYPES[dt])


@pytest.mark.parametrize("h,dt", [(4, "f32"), (3, "f32"), (8, "bf16")])
def test_many_rows(device, h, dt):
    gc.check_many_rows(device, h, DTYPES[dt])


@pytest.mark.parametrize("h,dt", [(4, "f32"), (3, "f32"), (8, "bf16"), (4, "f16"), (2, "f64")])
def test_unaligned_base_and_row_ranges(device, h, dt):
    gc.check_unaligned_and_ranges(device, h, DTYPES[dt])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_columns_out_of_range(device, dt):
    gc.check_columns_out_of_range(device, DTYPES[dt])


@pytest.mark.parametrize("slope", gc.SLOPES)
@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_activation_edges(device, dt, slope):
    gc.check_activation_edges(device, DTYPES[dt], slope)


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_special_values_stay_in_their_head_and_row(device, dt):
    gc.check_special_confined(device, DTYPES[dt])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_single_head_and_empty(device, dt):
    gc.check_degenerate(device, DTYPES[dt])


def test_argument_checks(device):
    gc.check_argument_checks(device)


def test_op_layer(device):
    gc.check_op_layer(device)


def test_public_api(device):
    gc.check_public_api(device)


@pytest.mark.parametrize("h,dt", [(3, "f32"), (8, "f32"), (4, "bf16"), (2, "f64"), (1, "f16")])
def test_gradients_match_the_reference_chain(device, h, dt):
    gc.check_grads(device, h, DTYPES[dt])


def test_needs_input_grad(device):
    gc.check_needs_input_grad(device)


def test_gradcheck(device):
    gc.check_gradcheck(device)


def test_gat_attention_dense_reference_f32(device):
    gc.check_dense_reference_f32(device)


@pytest.mark.graph_capture
def test_graph_capture(device):
    """Forward and gradient captured into one graph (no allocation, no host synchronisation in
    the launches) and replayed on new s_row and s_col: the same bits as a fresh eager call and as
    the kCPU entry.  H = 8 takes the packed path, H = 3 the general one."""
    for heads in (8, 3):
        rp, ci, s_row, s_col, g = gc.problem([0, 1, 7, 8, 9, 63, 64, 65, 513], heads,
                                             torch.float32, m=27, seed=9)
        d_rp, d_ci, d_sr, d_sc, d_g = gc.to_dev(device, rp, ci, s_row, s_col, g)
        attn = torch.empty_like(d_g)
        ds = torch.empty_like(d_g)
        d_row = torch.empty_like(d_sr)

        def step():
            _C.gat_softmax_csr_heads(d_rp, d_ci, d_sr, d_sc, 0.2, out=attn)
            x, y = _C.gat_softmax_csr_heads_grad(d_rp, d_ci, d_sr, d_sc, attn, d_g, 0.2)
            ds.copy_(x)
            d_row.copy_(y)

        s = torch.cuda.Stream(device)
        s.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(s):  # warm-up outside the capture
            step()
        torch.cuda.current_stream(device).wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
        rng = np.random.default_rng(10)
        d_sr.copy_(scores(s_row.numel(), torch.float32, rng, False).view(s_row.shape))
        d_sc.copy_(scores(s_col.numel(), torch.float32, rng, False).view(s_col.shape))
        graph.replay()
        torch.cuda.synchronize(device)
        assert_same(attn, gc.run_forward(d_rp, d_ci, d_sr, d_sc, 0.2), f"replayed forward H={heads}")
        e_ds, e_d_row = gc.run_backward(d_rp, d_ci, d_sr, d_sc, 0.2, attn, d_g)
        assert_same(ds, e_ds, f"replayed ds H={heads}")
        assert_same(d_row, e_d_row, f"replayed d_row H={heads}")
        k_attn = flow_spmm.gat_softmax(rp, ci, d_sr.cpu(), d_sc.cpu())
        assert_same(attn, k_attn, f"replayed forward vs kCPU H={heads}")
        k_ds, k_d_row = gc.run_backward(rp, ci, d_sr.cpu(), d_sc.cpu(), 0.2, k_attn, g)
        assert_same(ds, k_ds, f"replayed ds vs kCPU H={heads}")
        assert_same(d_row, k_d_row, f"replayed d_row vs kCPU H={heads}")

"""Multi-head edge softmax (ops "edge_softmax_csr_heads" and its gradient) on the MI355X: the HIP
kernels of csrc/edge_softmax_heads.hip against the numpy restatement of the single-head contract
per column, against the single-head HIP op on every contiguous column and against the kCPU
kernels, bit for bit (edge_softmax_heads_cases.py): every boundary row length, head counts of the
packed and the general path, every lane-group width, an unaligned base, row ranges, special values
confined to one head, the public API, the op layer, the argument checks and graph capture."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import edge_softmax_heads_cases as hc
import heads_cases
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
    hc.check_boundaries(device, h, DTYPES[dt], it)


@pytest.mark.parametrize("h,dt", [(3, "f32"), (8, "f32"), (8, "bf16"), (5, "f16"), (2, "f64"),
                                  (3, "f64")])
@pytest.mark.parametrize("mix", list(hc.LG_MIXES))
def test_lane_group_mixes(device, mix, h, dt):
    """The launches whose mean degree picks 1, 4 and 16 lanes per (row, head group): most rows in
    their group's registers, the longer ones taken over by the wave."""
    hc.check_lane_groups(device, mix, h, DTYPES[dt])


@pytest.mark.parametrize("h,dt", [(4, "f32"), (3, "f32"), (4, "bf16"), (2, "f64")])
def test_many_tiles(device, h, dt):
    hc.check_many_tiles(device, h, DTYPES[dt])


@pytest.mark.parametrize("h,dt", [(8, "f32"), (3, "f32"), (8, "bf16")])
def test_many_rows(device, h, dt):
    hc.check_many_rows(device, h, DTYPES[dt])


@pytest.mark.parametrize("h,dt", [(4, "f32"), (3, "f32"), (8, "bf16"), (4, "f16"), (2, "f64")])
def test_unaligned_base_and_row_ranges(device, h, dt):
    hc.check_unaligned_and_ranges(device, h, DTYPES[dt])


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_special_values_stay_in_their_head(device, dt):
    hc.check_special_confined(device, DTYPES[dt])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_single_head_and_empty(device, dt):
    hc.check_single_head_bits(device, DTYPES[dt])


def test_public_api(device, monkeypatch):
    hc.check_public_api(device, monkeypatch)


def test_attention_layer_heads_f32(device):
    heads_cases.check_attention_heads_f32(device)


def test_op_layer(device):
    hc.check_op_layer(device)


def test_argument_checks(device):
    hc.check_argument_checks(device)


@pytest.mark.graph_capture
def test_graph_capture(device):
    """Forward and gradient captured into one graph (no allocation, no host synchronisation in
    the launches) and replayed on new scores: the same bits as a fresh eager call.  H = 8 takes
    the packed path, H = 3 the general one."""
    for heads in (8, 3):
        rp, ci, e, g = hc.problem([0, 1, 7, 8, 9, 63, 64, 65, 513], heads, torch.float32, m=27,
                                  seed=9)
        d_rp, d_ci, d_e, d_g = hc.to_dev(device, rp, ci, e, g)
        y = torch.empty_like(d_e)
        de = torch.empty_like(d_e)
        s = torch.cuda.Stream(device)
        s.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(s):  # warm-up outside the capture
            _C.edge_softmax_csr_heads(d_rp, d_ci, d_e, out=y)
        torch.cuda.current_stream(device).wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _C.edge_softmax_csr_heads(d_rp, d_ci, d_e, out=y)
            de.copy_(_C.edge_softmax_csr_heads_grad(d_rp, d_ci, y, d_g))
        d_e.copy_(scores(e.numel(), torch.float32, np.random.default_rng(10), False).view(e.shape))
        graph.replay()
        torch.cuda.synchronize(device)
        m = rp.numel() - 1
        assert_same(y, hc.run_forward(d_rp, d_e, m), f"replayed forward H={heads}")
        assert_same(de, _C.edge_softmax_csr_heads_grad(d_rp, d_ci, y, d_g),
                    f"replayed backward H={heads}")
        assert_same(y, flow_spmm.edge_softmax(rp, ci, d_e.cpu()),
                    f"replayed forward vs kCPU H={heads}")

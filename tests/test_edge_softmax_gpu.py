"""Edge softmax over CSR rows (op "edge_softmax_csr" and its gradient) on the GPU: the HIP kernels
of csrc/edge_softmax.hip against the numpy restatement of the contract and, bit for bit, against
the kCPU kernels (edge_softmax_cases.py); every lane-group width, rows held in registers and rows
swept in tiles, row ranges, an unaligned base pointer, graph capture."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import edge_softmax_cases as ec
import oneflow_spmm as flow_spmm
from edge_softmax_helpers import run_forward
from helpers import DTYPES
from oneflow_spmm import _C
from reduce_helpers import assert_same

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("it", [torch.int32, torch.int64])
@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
@pytest.mark.parametrize("mix", ["lg16", "lg64"])
def test_bit_identity(device, mix, dt, it, exact):
    ec.check_bit_identity(device, mix, DTYPES[dt], it, exact)


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
@pytest.mark.parametrize("mix", ["lg1", "lg4"])
def test_narrow_groups(device, mix, dt):
    """The launches whose mean degree picks one lane or four per row: most rows in their group's
    registers, the longer ones taken over by the wave."""
    ec.check_bit_identity(device, mix, DTYPES[dt], torch.int32, False)


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16"])
def test_many_tiles(device, dt):
    """Rows of 6 to 38 tiles: the binary-counter stack past its first two levels."""
    ec.check_bit_identity(device, "tiles", DTYPES[dt], torch.int32, False)


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_schedule_and_ranges(device, dt):
    ec.check_schedule_and_ranges(device, DTYPES[dt])


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_special_values(device, dt):
    ec.check_special(device, DTYPES[dt])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_many_rows(device, dt):
    ec.check_many_rows(device, DTYPES[dt])


def test_softmax_accuracy(device):
    ec.check_softmax_accuracy(device)


def test_gradcheck(device):
    ec.check_gradcheck(device)


def test_attention_layer_f32(device):
    ec.check_attention_f32(device)


def test_op_layer(device):
    ec.check_op_layer(device)


@pytest.mark.graph_capture
def test_graph_capture(device):
    """Forward and backward captured into one graph (no allocation, no host synchronisation in
    the launches) and replayed on new scores: the same bits as the eager calls."""
    rp, ci, e, g = ec.problem(ec.SHORT + [ec.T + 1], torch.float32, seed=9)
    d_rp, d_ci, d_e, d_g = ec.to_dev(device, rp, ci, e, g)
    y = torch.empty_like(d_e)
    de = torch.empty_like(d_e)
    s = torch.cuda.Stream(device)
    s.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(s):  # warm-up outside the capture
        _C.edge_softmax_csr(d_rp, d_ci, d_e, out=y)
    torch.cuda.current_stream(device).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _C.edge_softmax_csr(d_rp, d_ci, d_e, out=y)
        de.copy_(_C.edge_softmax_csr_grad(d_rp, d_ci, y, d_g))
    d_e.copy_(ec.scores(e.numel(), torch.float32, np.random.default_rng(10), False))
    graph.replay()
    torch.cuda.synchronize(device)
    m = rp.numel() - 1
    assert_same(y, run_forward(d_rp, d_e, m), "replayed forward")
    assert_same(de, _C.edge_softmax_csr_grad(d_rp, d_ci, y, d_g), "replayed backward")
    assert_same(y, flow_spmm.edge_softmax(rp, ci, d_e.cpu()), "replayed forward vs kCPU")

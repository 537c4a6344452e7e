"""The SpMM over per-edge feature vectors on the MI355X (`spmm_edge`): the HIP kernels of
csrc/spmm_edge.hip and csrc/spmm_edge_grad.hip against the float64 reference, bit for bit
(spmm_edge_cases.py): every lane group and a second column tile, the general path, the boundary
row lengths under the default and a forced schedule, repeated columns, columns outside [0, K), an
unaligned leading dimension, a row range, relu's edges; against the kCPU kernels on
order-sensitive inputs; the `spmm` identity, autograd, the argument errors and graph capture."""
from __future__ import annotations

import pytest
import torch

import oneflow_spmm as flow_spmm
import spmm_edge_cases as ec

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("op,act", ec.PAIRS)
@pytest.mark.parametrize("name", ec.CASES)
def test_case_table(device, name, op, act):
    ec.check_case(device, name, op, act)


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_same_bits_as_kcpu_on_normal_inputs(device, dt):
    host, dev = ec.random_problem(dt, "cpu"), ec.random_problem(dt, device)
    for op, act in ec.PAIRS:
        for split in (0, 8):
            for a, b, what in zip(ec.run_random(dev, op, act, split),
                                  ec.run_random(host, op, act, split), ("out", "de", "db")):
                ec.bits_equal(a, b, f"{what} {dt} {op} {act} split={split}: HIP vs kCPU")


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_mul_on_expanded_values_has_spmm_bits(device, dt):
    ec.check_spmm_identity(device, dt)


def test_autograd(device, monkeypatch):
    ec.check_autograd(device, monkeypatch)


def test_argument_errors(device):
    ec.check_errors(device)


@pytest.mark.graph_capture
def test_graph_capture_replays_on_new_values(device):
    """One capture of the forward and both gradients (a hub row: planner, chunks, hub sum), replayed
    on new values: every replay equals the eager result."""
    rp, ci, e, b, dy = ec.random_problem("f32", device)
    m = rp.numel() - 1
    e, b = e.requires_grad_(), b.requires_grad_()

    def step():
        out = flow_spmm.spmm_edge(rp, ci, e, m, ec.K, b, "add", "relu")
        return (out,) + torch.autograd.grad(out, (e, b), dy)

    step()  # warm-up: the transpose is cached before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for seed in (1, 2, 3):
        _, _, e2, b2, _ = ec.random_problem("f32", device, seed=seed)
        with torch.no_grad():
            e.copy_(e2)
            b.copy_(b2)
        graph.replay()
        torch.cuda.synchronize()
        for got, want, what in zip(captured, step(), ("out", "de", "db")):
            ec.bits_equal(got, want, f"replay {seed}: {what}")

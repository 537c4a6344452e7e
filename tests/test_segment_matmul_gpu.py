"""`segment_matmul` on the MI355X: the MFMA kernels of csrc/segment_matmul.hip and
csrc/segment_matmul_grad_w.hip through the op layer and autograd against the float64 torch loop
(segment_matmul_cases.py): the exact case table (any permutation of an operand or result layout,
any tail or mask error shows as a wrong bit), the contract's bound on normal inputs with
repeatability, the argument errors and graph capture."""
from __future__ import annotations

import pytest
import torch

import oneflow_spmm as flow_spmm
import segment_matmul_cases as sc
from oneflow_spmm import _C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("trans_w", [False, True])
@pytest.mark.parametrize("it", sc.INDEX)
@pytest.mark.parametrize("dt", sc.DTYPES)
@pytest.mark.parametrize("name", sc.CASES)
def test_case_table(device, name, dt, it, trans_w):
    sc.check_exact(device, name, dt, it, trans_w)


@pytest.mark.parametrize("with_idx", [False, True])
@pytest.mark.parametrize("dt", sc.DTYPES)
def test_bound_and_repeatability(device, dt, with_idx):
    sc.check_bound(device, dt, with_idx)


def test_argument_errors(device):
    sc.check_errors(device)


@pytest.mark.graph_capture
def test_graph_capture_replays_on_new_values(device):
    """The forward and dw with idx, and dx without idx, captured once and replayed on three new
    seeded inputs: every replay equals the eager result bit for bit."""
    x, w, seg_ptr, idx, dy, _ = sc.make_case("table_idx", torch.float32, torch.int32, device)

    def step():
        return (flow_spmm.segment_matmul(x, w, seg_ptr, idx),
                _C.segment_matmul_grad_w(x, dy, seg_ptr, idx),
                flow_spmm.segment_matmul(dy, w, seg_ptr, None, trans_w=True))

    step()  # warm-up: code objects are loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for seed in (1, 2, 3):
        x2, w2, _, _, dy3, _ = sc.make_case("table_idx", torch.float32, torch.int32, device,
                                            seed=seed)
        x.copy_(x2), w.copy_(w2), dy.copy_(dy3)
        graph.replay()
        torch.cuda.synchronize()
        for got, want, what in zip(captured, step(), ("out", "dw", "dx")):
            assert torch.equal(got, want), f"replay {seed}: {what}"

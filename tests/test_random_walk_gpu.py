"""Random walks on the GPU (csrc/random_walk.hip): both HIP kernels against the
Python restatement and the kCPU kernel, bit for bit; bad inputs; a GraphSAINT-RW batch in `spmm`."""
import numpy as np
import pytest
import torch

import oneflow_spmm as fs
from oracle import oracle
from tests import node_subgraph_cases
from tests import random_walk_cases as cases
from tests.random_walk_cases import IDX
from tests.test_random_walk_cpu import assert_reference_is_sharp, walk

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("length", [1, 7, 8, 9, 33])
@pytest.mark.parametrize("pq", cases.PQ)
@pytest.mark.parametrize("idx", list(IDX))
def test_gpu_equals_restatement_and_cpu(device, idx, pq, length):
    it = IDX[idx]
    rp, ci, starts, walks, eids, stats = cases.case(3000, 2500, pq)
    assert_reference_is_sharp(stats, pq)
    got = walk((rp, ci, starts), it, length, pq, dev=device)
    cases.assert_walks(got, walks, eids, it, "cuda", length)
    host = walk((rp, ci, starts), it, length, pq)
    assert torch.equal(got[0].cpu(), host[0]) and torch.equal(got[1].cpu(), host[1])
    if length == 9:
        got = walk((rp, ci, starts), it, length, pq, dev=device, return_edge_ids=False)
        assert got[1] is None
        cases.assert_walks(got, walks, eids, it, "cuda", length)


@pytest.mark.parametrize("length", [3, 17])
@pytest.mark.parametrize("s", [0, 1, 63, 64, 65])
@pytest.mark.parametrize("pq", [(1.0, 1.0), (1.0, 2.0)])
def test_partial_waves(device, pq, s, length):
    rp, ci, starts, walks, eids, _ = cases.case(3000, 65, pq, 17)
    for it in IDX.values():
        got = walk((rp, ci, starts[:s]), it, length, pq, dev=device)
        cases.assert_walks(got, walks[:s], eids[:s], it, "cuda", length)


def test_attempt_cap(device):
    rp, ci, starts, length, pq, seed, walks, eids, stats = cases.ring_case()
    assert 1 <= stats["capped"] < stats["biased"]
    for it in IDX.values():
        got = walk((rp, ci, starts), it, length, pq, seed, dev=device)
        cases.assert_walks(got, walks, eids, it, "cuda")


@pytest.mark.parametrize("idx", list(IDX))
def test_bad_inputs_raise_and_the_next_call_is_right(device, idx):
    it = IDX[idx]
    rp, ci, starts, walks, eids, _ = cases.case(3000, 2500, (1.0, 2.0))
    for pq in ((1.0, 1.0), (1.0, 2.0)):
        for bad in (len(rp) - 1, -1, 2 ** 31 - 1):
            spoiled = starts.copy()
            spoiled[17] = bad
            with pytest.raises(RuntimeError, match="outside"):
                walk((rp, ci, spoiled), it, 3, pq, dev=device)
        broken = rp.copy()
        broken[cases.HUB + 1] = len(ci) + 5  # the hub, a start, ends past nnz
        with pytest.raises(RuntimeError, match="outside"):
            walk((broken, ci, starts), it, 3, pq, dev=device)
    torch.cuda.synchronize()
    got = walk((rp, ci, starts), it, 9, (1.0, 2.0), dev=device)
    cases.assert_walks(got, walks, eids, it, "cuda", 9)


@pytest.mark.parametrize("idx", list(IDX))
def test_a_walk_batch_through_spmm(device, idx):
    """`node_subgraph` of the reference walks' nodes, and `spmm` on it gives the oracle's bits."""
    it = IDX[idx]
    rp, ci = cases.graph(3000, wide=False)
    starts = cases.starts_of(3000, 200)
    walks = cases.reference(rp, ci, starts, 2, 1.0, 1.0, 5)[0]
    host = [cases.tensor(a, it) for a in (rp, ci, starts)]
    want = fs.node_subgraph(host[0], host[1], cases.tensor(walks[walks >= 0], it))
    got = fs.random_walk_subgraph(*(a.to(device) for a in host), 2, seed=5)
    node_subgraph_cases.assert_subgraph(got, want, it, "cuda")
    src, rp_s, col_local, eid, _ = got
    gen = np.random.default_rng(4)
    values = gen.uniform(-1, 1, len(ci)).astype(np.float32)[eid.cpu().numpy()]
    h = gen.uniform(-1, 1, (src.numel(), 8)).astype(np.float32)
    out = fs.spmm(rp_s, col_local, torch.from_numpy(values).to(device), src.numel(), src.numel(),
                  torch.from_numpy(h).to(device))
    ref = oracle.spmm(rp_s.cpu().numpy(), col_local.cpu().numpy(), values, h)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32))

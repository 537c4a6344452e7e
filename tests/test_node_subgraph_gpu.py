"""Induced-subgraph extraction on the GPU (csrc/node_subgraph.hip): the HIP kernels
against the numpy restatement and the kCPU kernel over the case table of
tests/node_subgraph_cases.py, bad inputs, and one mean `spmm` layer on the subgraph."""
import numpy as np
import pytest
import torch

import oneflow_spmm as fs
from tests import node_subgraph_cases as cases

pytestmark = pytest.mark.gpu

IDX = cases.IDX


@pytest.mark.parametrize("idx", list(IDX))
@pytest.mark.parametrize("name", cases.CASES + ["wide"])
def test_gpu_equals_numpy_and_cpu(device, name, idx):
    it = IDX[idx]
    rp, ci, nodes, ref = cases.case(name)
    host = [cases.tensor(a, it) for a in (rp, ci, nodes)]
    got = fs.node_subgraph(*(a.to(device) for a in host))
    cases.assert_subgraph(got, ref, it, "cuda")
    cases.assert_subgraph(got, fs.node_subgraph(*host), it, "cuda")
    if name == "all":  # the graph itself
        cases.assert_subgraph(got[1:4], (rp, ci, np.arange(len(ci))), it, "cuda")
    if name == "shuffled":
        again = fs.node_subgraph(*(a.to(device) for a in host), return_edge_ids=False)
        assert again[3] is None
        cases.assert_subgraph(again[:3] + (got[3], again[4]), ref, it, "cuda")


@pytest.mark.parametrize("idx", list(IDX))
def test_bad_inputs_raise_and_the_next_call_is_right(device, idx):
    it = IDX[idx]
    rp, ci, nodes, ref = cases.case("shuffled")
    good = [cases.tensor(a, it, device) for a in (rp, ci, nodes)]
    for bad in cases.bad_node_ids(it, len(rp) - 1):
        spoiled = nodes.copy()
        spoiled[17] = bad
        with pytest.raises(RuntimeError, match="outside"):
            fs.node_subgraph(good[0], good[1], cases.tensor(spoiled, it, device))
    v = int(nodes[5])
    broken = rp.copy()
    broken[v + 1] = broken[v] - 1  # row v, which is selected, has degree -1
    with pytest.raises(RuntimeError, match="outside"):
        fs.node_subgraph(cases.tensor(broken, it, device), good[1], good[2])
    torch.cuda.synchronize()
    cases.assert_subgraph(fs.node_subgraph(*good), ref, it, "cuda")


def test_a_mean_layer_on_the_subgraph(device):
    """`spmm(..., reduce="mean")` on the GPU's subgraph of 200 nodes: the bits of the same call on
    the kCPU kernel's subgraph, and a dense float64 restatement within the error of a float32 sum
    of d products and its division: (d + 2) * 2^-24 * sum |v h| / d per element."""
    rp, ci = cases.graph()
    gen = np.random.default_rng(3)
    nodes = np.concatenate([[cases.HUB], gen.choice(len(rp) - 1, 199, replace=False)])
    host = [cases.tensor(a, torch.int32) for a in (rp, ci, nodes)]
    values = torch.from_numpy(gen.uniform(0.5, 1.5, len(ci)).astype(np.float32))
    h = torch.from_numpy(gen.uniform(-1, 1, (len(rp) - 1, 8)).astype(np.float32))

    def layer(sub):
        src, rp_s, col_local, eid, _ = (x.to(device) for x in sub)
        c = src.numel()
        return fs.spmm(rp_s, col_local, values.to(device)[eid.long()], c, c, h.to(device)[src.long()],
                       reduce="mean")

    out = layer(fs.node_subgraph(*(a.to(device) for a in host)))
    assert torch.equal(out.view(torch.int32), layer(fs.node_subgraph(*host)).view(torch.int32))
    src = np.unique(nodes)
    a, kept = np.zeros((len(src), len(src))), np.zeros((len(src), 1))
    for r, v in enumerate(src):  # the values are positive: |a| is a
        js = np.arange(rp[v], rp[v + 1])
        js = js[np.isin(ci[js], src)]
        np.add.at(a[r], np.searchsorted(src, ci[js]), values.numpy()[js].astype(np.float64))
        kept[r] = len(js)
    hs = h.numpy().astype(np.float64)[src]
    want = a @ hs / np.maximum(kept, 1)
    tol = (kept + 2) * 2.0 ** -24 * (a @ np.abs(hs)) / np.maximum(kept, 1)
    assert np.all(np.abs(out.cpu().numpy().astype(np.float64) - want) <= tol)

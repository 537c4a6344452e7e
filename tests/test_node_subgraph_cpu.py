"""Induced-subgraph extraction: the kCPU kernel behind `node_subgraph` against the
numpy restatement over the case table of tests/node_subgraph_cases.py, its errors, and the size
checks of the device entries (which launch nothing)."""
import ctypes

import pytest
import torch

import oneflow_spmm as fs
from oneflow_spmm import _lib
from tests import node_subgraph_cases as cases

IDX = cases.IDX


def run(name, it, dev="cpu", **kw):
    rp, ci, nodes, ref = cases.case(name)
    return fs.node_subgraph(*(cases.tensor(a, it, dev) for a in (rp, ci, nodes)), **kw), ref


@pytest.mark.parametrize("idx", list(IDX))
@pytest.mark.parametrize("name", cases.CASES + ["wide"])
def test_cpu_equals_numpy(name, idx):
    got, ref = run(name, IDX[idx])
    cases.assert_subgraph(got, ref, IDX[idx], "cpu")
    if name == "all":  # the graph itself
        rp, ci = cases.graph()
        cases.assert_subgraph(got[1:4], (rp, ci, torch.arange(len(ci))), IDX[idx], "cpu")
    if name == "shuffled":
        src, rp_s, col_local, none, node_pos = run(name, IDX[idx], return_edge_ids=False)[0]
        assert none is None
        cases.assert_subgraph((src, rp_s, col_local, got[3], node_pos), ref, IDX[idx], "cpu")


@pytest.mark.parametrize("idx", list(IDX))
@pytest.mark.parametrize("name", ["all", "hub", "shuffled"])
def test_thread_count_does_not_change_the_arrays(name, idx):
    for nt in (1, 16):
        got, ref = run(name, IDX[idx], num_threads=nt)
        cases.assert_subgraph(got, ref, IDX[idx], "cpu")


@pytest.mark.parametrize("idx", list(IDX))
def test_bad_inputs_are_refused_and_the_next_call_is_right(idx):
    it = IDX[idx]
    rp, ci, nodes, ref = cases.case("shuffled")
    good = [cases.tensor(a, it) for a in (rp, ci, nodes)]
    for bad in cases.bad_node_ids(it, len(rp) - 1):
        spoiled = nodes.copy()
        spoiled[17] = bad
        with pytest.raises(fs.OfxError, match="outside") as e:
            fs.node_subgraph(good[0], good[1], cases.tensor(spoiled, it))
        assert e.value.code == _lib.OFX_EINVAL
    v = int(nodes[5])
    broken = rp.copy()
    broken[v + 1] = broken[v] - 1  # row v, which is selected, has degree -1
    with pytest.raises(fs.OfxError, match="outside") as e:
        fs.node_subgraph(cases.tensor(broken, it), good[1], good[2])
    assert e.value.code == _lib.OFX_EINVAL
    cases.assert_subgraph(fs.node_subgraph(*good), ref, it, "cpu")


@pytest.mark.parametrize("m, nnz, s", [(2 ** 31, 8, 3), (5, 2 ** 31, 3), (-1, 8, 3), (5, 8, 2 ** 31)])
def test_bad_sizes_are_refused_before_any_launch(m, nnz, s):
    # every entry checks the sizes first: no pointer is read, no GPU is needed
    size = ctypes.c_size_t(0)
    lib, dt = _lib.LIB, _lib.DT_INT64
    assert lib.ofx_node_subgraph_workspace_size(dt, m, nnz, s, ctypes.byref(size)) == _lib.OFX_EINVAL
    assert lib.ofx_node_subgraph_count(None, dt, m, nnz, s, None, None, None, None, None, None, None,
                                       None, 0) == _lib.OFX_EINVAL
    assert lib.ofx_node_subgraph_fill(None, dt, m, nnz, s, 0, 0, None, None, None, None, None, None,
                                      None, 0) == _lib.OFX_EINVAL


def test_arguments_and_exports():
    ids = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(TypeError):
        fs.node_subgraph(ids, ids, ids.to(torch.int32))
    with pytest.raises(RuntimeError, match="1-D"):
        fs.node_subgraph(ids, ids, ids.view(3, 1))
    assert fs.node_subgraph is fs.sampling.node_subgraph and "node_subgraph" in fs.__all__
    assert {"ofx_node_subgraph_workspace_size", "ofx_node_subgraph_count", "ofx_node_subgraph_fill",
            "ofx_node_subgraph_count_cpu", "ofx_node_subgraph_fill_cpu"} <= set(_lib.EXPORTED)

"""Random walks over CSR: the kCPU kernel against the Python restatement, the
restatement against known walks, the attempt cap, node2vec's class frequencies, the errors."""
import ctypes

import numpy as np
import pytest
import torch

import oneflow_spmm as fs
from oneflow_spmm import _lib
from tests import node_subgraph_cases
from tests import random_walk_cases as cases
from tests.random_walk_cases import IDX


def walk(arrays, it, length, pq, seed=cases.SEED, dev="cpu", **kw):
    kw.setdefault("return_edge_ids", True)
    return fs.random_walk(*(cases.tensor(a, it, dev) for a in arrays), length, p=pq[0], q=pq[1],
                          seed=seed, **kw)


def assert_reference_is_sharp(stats, pq):
    """The case meets every class, ends walks early and, when biased, needs a second round."""
    assert min(stats["met"]) >= 50 and stats["ended"] >= 1
    assert pq == (1.0, 1.0) or stats["max_attempt"] >= 8


def test_known_walks():
    *_, walks, eids, _ = cases.case(300, 400, (0.25, 4.0))
    for i, (nodes, entries) in cases.KNOWN_WALKS.items():
        assert walks[i, :10].tolist() == nodes and eids[i, :9].tolist() == entries


@pytest.mark.parametrize("length", [1, 7, 8, 9, 33])
@pytest.mark.parametrize("pq", cases.PQ)
@pytest.mark.parametrize("idx", list(IDX))
def test_cpu_equals_restatement(idx, pq, length):
    rp, ci, starts, walks, eids, stats = cases.case(300, 400, pq)
    assert_reference_is_sharp(stats, pq)
    for nt in (1, 16) if length == 33 else (0,):  # the thread count does not change the arrays
        got = walk((rp, ci, starts), IDX[idx], length, pq, num_threads=nt)
        cases.assert_walks(got, walks, eids, IDX[idx], "cpu", length)
    if length == 9:
        got = walk((rp, ci, starts), IDX[idx], length, pq, return_edge_ids=False)
        assert got[1] is None
        cases.assert_walks(got, walks, eids, IDX[idx], "cpu", length)


def test_attempt_cap():
    rp, ci, starts, length, pq, seed, walks, eids, stats = cases.ring_case()
    assert stats["met"][cases.COMMON] == 0
    assert 1 <= stats["capped"] < stats["biased"]  # the cap was needed, and not by every step
    for it in IDX.values():
        cases.assert_walks(walk((rp, ci, starts), it, length, pq, seed), walks, eids, it, "cpu")


@pytest.mark.parametrize("pq", [(1.0, 1.0), (0.5, 2.0), (4.0, 0.25)])
def test_class_frequencies_are_node2vecs(pq):
    """The circulant graph C12(1, 2), degree 4: of the neighbours of 1 seen from 0, 0 is the return,
    2 and 11 are common, 3 is out.  8e5 two-step walks from 0: the first step is uniform, the second
    of the about 2e5 through 1 has node2vec's weights, each within 5 binomial standard deviations."""
    n, s = 12, 800_000
    ci = np.sort((np.arange(n).reshape(-1, 1) + np.array([-2, -1, 1, 2])) % n, 1).reshape(-1)
    rp = np.arange(n + 1) * 4
    walks, _ = walk((rp, ci, np.zeros(s, dtype=np.int64)), torch.int64, 2, pq, seed=7)
    walks = walks.numpy()

    def check(got, want, count):
        assert abs(got - want) <= 5 * np.sqrt(want * (1 - want) / count), (got, want, count)

    for x in (1, 2, 10, 11):
        check(np.mean(walks[:, 1] == x), 0.25, s)
    second = walks[walks[:, 1] == 1, 2]
    weight = {0: 1 / pq[0], 2: 1.0, 11: 1.0, 3: 1 / pq[1]}
    assert set(np.unique(second)) == set(weight) and len(second) > 190_000
    for x, w in weight.items():
        check(np.mean(second == x), w / sum(weight.values()), len(second))


@pytest.mark.parametrize("idx", list(IDX))
def test_bad_inputs_are_refused_and_the_next_call_is_right(idx):
    it = IDX[idx]
    rp, ci, starts, walks, eids, _ = cases.case(300, 400, (1.0, 2.0))
    for pq in ((1.0, 1.0), (1.0, 2.0)):
        for bad in (len(rp) - 1, -1, 2 ** 31 - 1):
            spoiled = starts.copy()
            spoiled[17] = bad
            with pytest.raises(fs.OfxError, match="outside") as e:
                walk((rp, ci, spoiled), it, 3, pq)
            assert e.value.code == _lib.OFX_EINVAL
        broken = rp.copy()
        broken[cases.HUB + 1] = len(ci) + 5  # the hub, a start, ends past nnz
        with pytest.raises(fs.OfxError, match="outside") as e:
            walk((broken, ci, starts), it, 3, pq)
        assert e.value.code == _lib.OFX_EINVAL
    cases.assert_walks(walk((rp, ci, starts), it, 9, (1.0, 2.0)), walks, eids, it, "cpu", 9)


@pytest.mark.parametrize("m, nnz, s, length, p, q", [
    (2, 3, 3, 0, 1, 1), (2, 3, 3, 65536, 1, 1), (2, 3, 3, 3, 0, 1), (2, 3, 3, 3, 1, -2),
    (2, 3, 3, 3, float("nan"), 1), (2, 3, 3, 3, 1, float("inf")),
    (2 ** 31, 8, 3, 3, 1, 1), (5, 2 ** 31, 3, 3, 1, 1), (5, 8, 2 ** 31, 3, 1, 1), (-1, 8, 3, 3, 1, 1)])
def test_bad_arguments_are_refused_before_any_launch(m, nnz, s, length, p, q):
    # both entries check before they read a pointer: no GPU is needed
    tail = (length, ctypes.c_double(p), ctypes.c_double(q), 0, None, None)
    lib, dt = _lib.LIB, _lib.DT_INT64
    assert lib.ofx_random_walk(None, dt, m, nnz, s, None, None, None, *tail, None) == _lib.OFX_EINVAL
    assert lib.ofx_random_walk_cpu(1, dt, m, nnz, s, None, None, None, *tail) == _lib.OFX_EINVAL


def test_walk_subgraph_is_the_subgraph_of_the_walks_nodes():
    rp, ci = cases.graph(300, wide=False)
    starts = cases.starts_of(300, 120)
    walks = cases.reference(rp, ci, starts, 2, 1.0, 1.0, 5)[0]
    host = [cases.tensor(a, torch.int32) for a in (rp, ci, starts)]
    want = fs.node_subgraph(host[0], host[1], cases.tensor(walks[walks >= 0], torch.int32))
    node_subgraph_cases.assert_subgraph(fs.random_walk_subgraph(*host, 2, seed=5), want, torch.int32, "cpu")


def test_arguments_and_exports():
    ids = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(TypeError):
        fs.random_walk(ids, ids, ids.to(torch.int32), 2)
    with pytest.raises(RuntimeError, match="1-D"):
        fs.random_walk(ids, ids, ids.view(3, 1), 2)
    assert fs.random_walk is fs.sampling.random_walk and "random_walk_subgraph" in fs.__all__
    assert {"ofx_random_walk", "ofx_random_walk_cpu"} <= set(_lib.EXPORTED)

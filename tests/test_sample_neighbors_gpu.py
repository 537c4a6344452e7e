"""Neighbour sampling over CSR on the GPU (csrc/sample_neighbors.hip): the HIP
kernels against the numpy restatement and the kCPU kernel, bit for bit; partial waves; bad seeds;
and the sampled CSR through the ops."""
import numpy as np
import pytest
import torch

import oneflow_spmm as fs
from oracle import oracle
from tests import sample_neighbors_cases as cases

pytestmark = pytest.mark.gpu

IDX = {"i32": torch.int32, "i64": torch.int64}
SEED = 11


def _t(a, it, dev="cpu"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(it).to(dev)


def _assert_equal(got, ref, it):
    for g, r, name in zip(got, ref, ("row_ptr_s", "col_idx_s", "edge_ids")):
        assert g.dtype == it and g.dim() == 1, name
        r = r.numpy() if isinstance(r, torch.Tensor) else r
        np.testing.assert_array_equal(g.cpu().numpy().astype(np.int64), r.astype(np.int64), err_msg=name)


# every group width (4, 8, 16, 32, 64 lanes) and both sides of each power of two
@pytest.mark.parametrize("idx", list(IDX))
@pytest.mark.parametrize("fanout", [1, 5, 16, 17, 33, 64])
def test_gpu_equals_restatement_and_cpu(device, fanout, idx):
    it = IDX[idx]
    rp, ci, seeds, ref = cases.gpu_case(fanout, SEED)
    deg = np.diff(rp)
    assert {0, fanout - 1, fanout, fanout + 1, 65} <= set(deg[seeds]) and (deg[seeds] == 20000).sum() >= 3
    assert len(seeds) == 2500 and len(np.unique(seeds)) < len(seeds)
    got = fs.sample_neighbors(_t(rp, it, device), _t(ci, it, device), _t(seeds, it, device), fanout,
                              seed=SEED)
    assert all(g.device.type == "cuda" for g in got)
    _assert_equal(got, ref, it)
    cpu = fs.sample_neighbors(_t(rp, it), _t(ci, it), _t(seeds, it), fanout, seed=SEED)
    _assert_equal(got, cpu, it)


@pytest.mark.parametrize("fanout", [4, 64])
@pytest.mark.parametrize("num_seeds", [0, 1, 63, 64, 65])
def test_partial_last_wave(device, num_seeds, fanout):
    rp, ci, seeds, _ = cases.gpu_case(fanout, SEED)
    # the degree edge cases and the hubs first, so that one seed already samples
    seeds = np.concatenate([[8, 5, 3], seeds])[:num_seeds]
    ref = cases.reference(rp, ci, seeds, fanout, 3)
    for it in IDX.values():
        got = fs.sample_neighbors(_t(rp, it, device), _t(ci, it, device), _t(seeds, it, device),
                                  fanout, seed=3)
        _assert_equal(got, ref, it)


@pytest.mark.parametrize("idx", list(IDX))
def test_bad_seed_raises_and_does_not_fault(device, idx):
    it = IDX[idx]
    rp, ci, seeds, ref = cases.gpu_case(5, SEED)
    m = len(rp) - 1
    d = [_t(a, it, device) for a in (rp, ci)]
    for bad in (m, -1, 2 ** 31 - 1):
        s = seeds[:200].copy()
        s[17] = bad
        with pytest.raises(RuntimeError, match="outside"):
            fs.sample_neighbors(*d, _t(s, it, device), 5, seed=SEED)
    torch.cuda.synchronize()
    # and the device is as it was: the next call gives the right arrays
    _assert_equal(fs.sample_neighbors(*d, _t(seeds, it, device), 5, seed=SEED), ref, it)
    rp_s, ci_s, none = fs.sample_neighbors(*d, _t(seeds, it, device), 5, seed=SEED,
                                           return_edge_ids=False)
    assert none is None
    _assert_equal((rp_s, ci_s), ref[:2], it)


@pytest.mark.parametrize("idx", list(IDX))
def test_sampled_csr_feeds_the_ops(device, idx):
    it = IDX[idx]
    rp, ci, seeds, _ = cases.gpu_case(5, SEED)
    k, n, s = len(rp) - 1, 16, len(seeds)
    rng = np.random.default_rng(4)
    values = rng.uniform(-1, 1, len(ci)).astype(np.float32)
    b = rng.uniform(-1, 1, (k, n)).astype(np.float32)
    rp_s, ci_s, eid = fs.sample_neighbors(_t(rp, it, device), _t(ci, it, device),
                                          _t(seeds, it, device), 5, seed=SEED)
    vals = torch.from_numpy(values).to(device)[eid.long()]
    out = fs.spmm(rp_s, ci_s, vals, s, k, torch.from_numpy(b).to(device))
    ref = oracle.spmm(rp_s.cpu().numpy(), ci_s.cpu().numpy(), vals.cpu().numpy(), b)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    # one GAT layer on the mini-batch: scores of the seeds and of all nodes, features of all nodes
    s_row = torch.from_numpy(rng.uniform(-1, 1, (s, 2)).astype(np.float32)).to(device)
    s_col = torch.from_numpy(rng.uniform(-1, 1, (k, 2)).astype(np.float32)).to(device)
    v = torch.from_numpy(rng.uniform(-1, 1, (k, 2, 8)).astype(np.float32)).to(device)
    h = fs.gat_attention(rp_s, ci_s, s_row, s_col, v)
    assert h.shape == (s, 2, 8) and bool(torch.isfinite(h).all())
    empty = (rp_s[1:] == rp_s[:-1])
    assert bool((h[empty] == 0).all()) and bool((h[~empty].abs().sum(dim=(1, 2)) > 0).all())

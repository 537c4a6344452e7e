"""Neighbour sampling over CSR: the kCPU kernel behind `sample_neighbors` against
the pure numpy restatement of tests/sample_neighbors_cases.py, the contract's structure, its
uniformity as a condition, its errors, and `sample_blocks` feeding the ops."""
import ctypes

import numpy as np
import pytest
import torch

import oneflow_spmm as fs
from oneflow_spmm import _lib
from tests import sample_neighbors_cases as cases

IDX = {"i32": torch.int32, "i64": torch.int64}
FANOUTS = [1, 4, 5, 16, 17, 64]
SEEDS = [0, 2 ** 63 + 5]


def _t(a, it=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(it)


def _sample(rp, ci, seeds, fanout, it=torch.int64, **kw):
    return fs.sample_neighbors(_t(rp, it), _t(ci, it), _t(seeds, it), fanout, **kw)


def _assert_equal(got, ref, it):
    for g, r, name in zip(got, ref, ("row_ptr_s", "col_idx_s", "edge_ids")):
        assert g.dtype == it and g.dim() == 1, name
        np.testing.assert_array_equal(g.cpu().numpy().astype(np.int64), r, err_msg=name)


# ---- the checker itself ------------------------------------------------------------------------
def test_restatement_passes_random123_vectors_and_known_rows():
    for counter, key, out in cases.PHILOX_VECTORS:
        assert tuple(int(x) for x in cases.philox4x32_10(counter, key)) == out
    for seed, v, deg, fanout, want in cases.KNOWN_ROWS:
        got = cases.row_positions(v, deg, fanout, seed)
        assert len(got) == min(deg, fanout) and got[:len(want)] == want, (seed, v)


# ---- 1. known answers --------------------------------------------------------------------------
def _positions_of_row(v, deg, fanout, seed):
    """The positions `ofx_sample_neighbors_cpu` gives row v of degree deg: col_idx = position."""
    ci = np.arange(deg, dtype=np.int64)
    if v < 2 ** 24:  # a row_ptr just long enough: rows 0..v-1 empty
        rp = np.zeros(v + 2, dtype=np.int64)
        rp[v + 1] = deg
        rp_s, ci_s, eid = _sample(rp, ci, [v], fanout, seed=seed)
        assert rp_s.tolist() == [0, min(deg, fanout)] and torch.equal(ci_s, eid)
        return ci_s.tolist()
    # A node id no row_ptr in memory reaches: the C entry is given the address at which row_ptr[0]
    # would stand if the two entries of row v stood where they do.  It reads row_ptr[v] and
    # row_ptr[v + 1] only.
    rp = np.array([0, deg], dtype=np.int64)
    seeds = np.array([v], dtype=np.int64)
    out_rp, out_ci, out_eid = (np.zeros(n, dtype=np.int64) for n in (2, fanout, fanout))
    cnt = ctypes.c_int64(0)
    base = (rp.ctypes.data - 8 * v) % 2 ** 64
    rc = _lib.LIB.ofx_sample_neighbors_cpu(1, _lib.DT_INT64, v + 1, 1, base,
                                           ci.ctypes.data, seeds.ctypes.data, fanout,
                                           seed % 2 ** 64, out_rp.ctypes.data, out_ci.ctypes.data,
                                           out_eid.ctypes.data, ctypes.byref(cnt))
    assert rc == _lib.OFX_OK, _lib.last_error()
    assert cnt.value == min(deg, fanout) and np.array_equal(out_ci, out_eid)
    return out_ci[:cnt.value].tolist()


@pytest.mark.parametrize("row", cases.KNOWN_ROWS, ids=lambda r: f"v{r[1]}")
def test_known_answers(row):
    seed, v, deg, fanout, want = row
    got = _positions_of_row(v, deg, fanout, seed)
    assert len(got) == min(deg, fanout)
    assert got[:len(want)] == want
    assert got == cases.row_positions(v, deg, fanout, seed)


# ---- 2. against the restatement ----------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("idx", list(IDX))
@pytest.mark.parametrize("fanout", FANOUTS)
def test_cpu_equals_restatement(fanout, idx, seed):
    rp, ci, seeds, ref = cases.cpu_case(fanout, seed)
    deg = np.diff(rp)
    assert {0, fanout - 1, fanout, fanout + 1, 65} <= set(deg[seeds]) and deg[seeds].max() > 5000
    assert len(seeds) == 400 and len(np.unique(seeds)) < len(seeds)
    _assert_equal(_sample(rp, ci, seeds, fanout, IDX[idx], seed=seed), ref, IDX[idx])


# ---- 3. structure ------------------------------------------------------------------------------
@pytest.mark.parametrize("fanout", [4, 17])
def test_structure(fanout):
    rp, ci, seeds, _ = cases.cpu_case(fanout, 0)
    deg = np.diff(rp)
    rp_s, ci_s, eid = (x.numpy() for x in _sample(rp, ci, seeds, fanout, seed=0))
    np.testing.assert_array_equal(rp_s, np.concatenate([[0], np.cumsum(np.minimum(deg[seeds], fanout))]))
    np.testing.assert_array_equal(ci_s, ci[eid])
    for i, v in enumerate(seeds):
        row = eid[rp_s[i]:rp_s[i + 1]]
        assert (np.diff(row) > 0).all() and (len(row) == 0 or (rp[v] <= row[0] and row[-1] < rp[v + 1]))
    # permuting the seeds permutes the rows
    perm = np.random.default_rng(5).permutation(len(seeds))
    rp_p, ci_p, eid_p = (x.numpy() for x in _sample(rp, ci, seeds[perm], fanout, seed=0))
    for new, old in enumerate(perm):
        np.testing.assert_array_equal(eid_p[rp_p[new]:rp_p[new + 1]], eid[rp_s[old]:rp_s[old + 1]])
        np.testing.assert_array_equal(ci_p[rp_p[new]:rp_p[new + 1]], ci_s[rp_s[old]:rp_s[old + 1]])
    # another seed: the same lengths, another subset of at least one long row
    rp_o, _, eid_o = (x.numpy() for x in _sample(rp, ci, seeds, fanout, seed=1))
    np.testing.assert_array_equal(rp_o, rp_s)
    changed = [i for i in range(len(seeds))
               if not np.array_equal(eid_o[rp_s[i]:rp_s[i + 1]], eid[rp_s[i]:rp_s[i + 1]])]
    assert changed and all(deg[seeds[i]] > fanout for i in changed)


@pytest.mark.parametrize("idx", list(IDX))
def test_thread_count_does_not_change_the_bits(idx):
    rp, ci, seeds, ref = cases.cpu_case(16, 0)
    for nt in (1, 16):
        _assert_equal(_sample(rp, ci, seeds, 16, IDX[idx], seed=0, num_threads=nt), ref, IDX[idx])


# ---- 4. uniformity: a condition ----------------------------------------------------------------
def test_every_position_is_drawn_equally_often():
    rows, deg, fanout = 20000, 37, 10
    rp, ci = cases.regular_graph(rows, deg)
    rp_s, ci_s, _ = _sample(rp, ci, np.arange(rows), fanout, seed=12345)
    assert rp_s[-1].item() == rows * fanout
    p = fanout / deg
    z = (np.bincount(ci_s.numpy(), minlength=deg) - rows * p) / np.sqrt(rows * p * (1 - p))
    print("max |z| over the 37 positions:", np.abs(z).max())
    assert len(z) == deg and np.abs(z).max() < 5.0


def test_every_subset_is_drawn_equally_often():
    rows, deg, fanout = 6000, 6, 5
    rp, ci = cases.regular_graph(rows, deg)
    _, ci_s, _ = _sample(rp, ci, np.arange(rows), fanout, seed=3)
    left_out = sum(range(deg)) - ci_s.numpy().reshape(rows, fanout).sum(axis=1)  # names the subset
    counts = np.bincount(left_out, minlength=deg)
    print("occurrences of the 6 subsets:", counts.tolist())
    assert len(counts) == deg and counts.min() >= 800 and counts.max() <= 1200


# ---- 5. errors and empties ---------------------------------------------------------------------
@pytest.mark.parametrize("idx", list(IDX))
def test_errors_and_empties(idx):
    it = IDX[idx]
    rp, ci, seeds, _ = cases.cpu_case(4, 0)
    m = len(rp) - 1
    for fanout in (0, 65):
        with pytest.raises(fs.OfxError) as e:
            _sample(rp, ci, seeds, fanout, it)
        assert e.value.code == _lib.OFX_EINVAL
    for bad in (m, -1):
        with pytest.raises(RuntimeError, match="outside"):
            _sample(rp, ci, np.array([3, bad, 5]), 4, it)
    # no seeds
    rp_s, ci_s, eid = _sample(rp, ci, np.zeros(0, np.int64), 4, it)
    assert rp_s.tolist() == [0] and ci_s.numel() == 0 and eid.numel() == 0
    assert rp_s.dtype == ci_s.dtype == eid.dtype == it
    # a graph without edges
    rp_s, ci_s, eid = _sample(np.zeros(8, np.int64), np.zeros(0, np.int64), np.array([6, 0, 6]), 4, it)
    assert rp_s.tolist() == [0, 0, 0, 0] and ci_s.numel() == 0 and eid.numel() == 0
    # without edge ids: the same two arrays
    full = _sample(rp, ci, seeds, 4, it, seed=9)
    rp_s, ci_s, none = _sample(rp, ci, seeds, 4, it, seed=9, return_edge_ids=False)
    assert none is None and torch.equal(rp_s, full[0]) and torch.equal(ci_s, full[1])


def test_a_degree_of_2_to_the_31_is_refused():
    rp = np.array([0, 2 ** 31], dtype=np.int64)  # never dereferenced: the row is refused first
    with pytest.raises(RuntimeError, match="outside"):
        _sample(rp, np.zeros(1, np.int64), np.array([0]), 4)


# ---- 6. sample_blocks --------------------------------------------------------------------------
def _small_graph(it):
    rng = np.random.default_rng(2)
    deg = rng.integers(1, 9, 50)
    rp = np.concatenate([[0], np.cumsum(deg)])
    ci = np.concatenate([np.sort(rng.choice(50, d, replace=False)) for d in deg])
    return _t(rp, it), _t(ci, it), rng


def _dense_mean(rp_s, col_local, vals, h):
    """The mean aggregation of one block from its sampled edges, in float64."""
    out = np.zeros((len(rp_s) - 1, h.shape[1]))
    for i in range(len(rp_s) - 1):
        js = range(rp_s[i], rp_s[i + 1])
        if len(js):
            out[i] = sum(vals[j] * h[col_local[j]] for j in js) / len(js)
    return out


@pytest.mark.parametrize("idx", list(IDX))
def test_sample_blocks_run_two_mean_layers(idx):
    rp, ci, rng = _small_graph(IDX[idx])
    seeds = _t(rng.choice(50, 12, replace=False), IDX[idx])
    values = torch.from_numpy(rng.uniform(0.5, 1.5, ci.numel()).astype(np.float32)).requires_grad_()
    x = torch.from_numpy(rng.uniform(-1, 1, (50, 8)).astype(np.float32)).requires_grad_()
    blocks = fs.sample_blocks(rp, ci, seeds, (3, 2), seed=5)
    assert len(blocks) == 2
    deg = np.diff(rp.numpy())
    # the output layer's block: fanout 2 from the seeds, seed 5 + 1; the input layer's from its src
    inner, outer = blocks
    assert torch.equal(outer[3][outer[4]], seeds) and torch.equal(inner[3][inner[4]], outer[3])
    for (rp_s, col_local, eid, src, seed_pos), fanout, cur in ((outer, 2, seeds), (inner, 3, outer[3])):
        assert torch.equal(src, torch.unique(src)) and rp_s.numel() == cur.numel() + 1
        np.testing.assert_array_equal(np.diff(rp_s.numpy()), np.minimum(deg[cur.numpy()], fanout))
        assert torch.equal(src[col_local.long()], ci[eid.long()])
    want = fs.sample_neighbors(rp, ci, seeds, 2, seed=6)
    assert torch.equal(outer[0], want[0]) and torch.equal(outer[2], want[2])

    h = x[inner[3].long()]
    ref = x.detach().numpy().astype(np.float64)[inner[3].numpy()]
    for rp_s, col_local, eid, src, seed_pos in blocks:
        assert h.shape[0] == src.numel()
        h = fs.spmm(rp_s, col_local, values[eid.long()], seed_pos.numel(), src.numel(), h, reduce="mean")
        ref = _dense_mean(rp_s.numpy(), col_local.numpy(),
                          values.detach().numpy().astype(np.float64)[eid.numpy()], ref)
    assert h.shape == (seeds.numel(), 8)
    assert np.abs(h.detach().numpy() - ref).max() <= 1e-6
    h.sum().backward()
    used = torch.zeros(ci.numel(), dtype=torch.bool)
    for b in blocks:
        used[b[2].long()] = True
    assert (values.grad[used] != 0).any() and (values.grad[~used] == 0).all()
    touched = torch.zeros(50, dtype=torch.bool)
    touched[inner[3][inner[1].long()].long()] = True
    # (a row of the input block that the output block did not sample gets no gradient either)
    assert (x.grad[touched] != 0).any() and (x.grad[~touched] == 0).all()

    # an FP8 feature table takes a block as it is
    rp_s, col_local, eid, src, seed_pos = inner
    feats = x.detach()[src.long()]
    b_q, b_scale = fs.quantize_rows_fp8(feats)
    vals = values.detach()[eid.long()]
    out = fs.spmm_fp8(rp_s, col_local, vals, seed_pos.numel(), src.numel(), b_q, b_scale)
    same = fs.spmm(rp_s, col_local, vals * b_scale[col_local.long()], seed_pos.numel(), src.numel(),
                   b_q.to(torch.float32))
    assert out.shape == (seed_pos.numel(), 8) and torch.equal(out, same)


def test_the_package_exports_the_sampler():
    assert fs.sample_neighbors is fs.sampling.sample_neighbors
    assert fs.sample_blocks is fs.sampling.sample_blocks
    assert {"sample_neighbors", "sample_blocks"} <= set(fs.__all__)
    assert {"ofx_sample_neighbors_workspace_size", "ofx_sample_neighbors",
            "ofx_sample_neighbors_cpu"} <= set(_lib.EXPORTED)

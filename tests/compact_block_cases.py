"""The inputs the block-compaction tests share (CPU and GPU run the same table), their numpy
reference (`np.unique` and `np.searchsorted` on int64) and the torch route `sample_blocks` took
before `compact_block`.  The bitmap has 32-bit words, 128-bit granules and tiles of
32,768 bits: the boundary cases stand on both sides of each."""
import functools

import numpy as np
import torch

import oneflow_spmm as fs

IDX = {"i32": torch.int32, "i64": torch.int64}
WORD, GRANULE, TILE = 32, 128, 32768
BOUNDARY_NODES = [1, 31, 32, 33, 127, 128, 129, 32767, 32768, 32769, 2 * 32768 + 5]
SIZES = [1, 63, 64, 65, 257]


def _boundary_ids(n):
    """0, n - 1 and both neighbours of every word, granule and tile boundary inside [0, n)."""
    ids = {0, n - 1}
    for step in (WORD, GRANULE, TILE):
        for b in range(step, n + 1, step):
            ids |= {b - 1, b}
    return np.array(sorted(i for i in ids if 0 <= i < n), dtype=np.int64)


def _build(name):
    """(num_nodes, seeds, cols) of a case, int64."""
    rng = np.random.default_rng(len(name) + sum(map(ord, name)))
    kind, _, arg = name.partition("-")
    if kind == "boundary":  # seeds: every third id; cols: all of them, some twice, shuffled
        n = int(arg)
        ids = _boundary_ids(n)
        return n, rng.permutation(ids[::3]), rng.permutation(np.concatenate([ids, ids[::2]]))
    if kind == "full":  # every node present
        n = int(arg)
        return n, rng.integers(0, n, 40), rng.permutation(n)
    if kind == "hub":  # one id 100,000 times among 50 others
        others = rng.choice(np.delete(np.arange(1000), 777), 50, replace=False)
        return 1000, others[:7], rng.permutation(np.concatenate([np.full(100_000, 777), others]))
    if kind == "sparse":  # many empty tiles, a scan over 153 tile counts
        n = 5_000_000
        ids = np.concatenate([rng.choice(n - 1, 999, replace=False), [n - 1]])
        return n, rng.permutation(ids)[:300], rng.permutation(ids)
    if kind == "sizes":  # S and E given: empty inputs, partial last waves and blocks
        s, e = (int(x) for x in arg.split("x"))
        return 300, rng.integers(0, 300, s), rng.integers(0, 300, e)
    pool = rng.permutation(2000)  # seeds with repeats, against the columns
    cols = np.repeat(pool[:400], 2)
    seeds = {"contained": pool[:100], "overlapping": pool[350:450], "disjoint": pool[400:500]}[arg]
    return 2000, rng.permutation(np.concatenate([seeds, seeds[:30]])), rng.permutation(cols)


CASES = ([f"boundary-{n}" for n in BOUNDARY_NODES] + ["full-129", "full-32769", "hub", "sparse"]
         + ["sizes-0x65", "sizes-65x0", "sizes-0x0"] + [f"sizes-{k}x{k}" for k in SIZES]
         + ["seeds-contained", "seeds-overlapping", "seeds-disjoint"])


@functools.lru_cache(maxsize=None)
def case(name):
    """(num_nodes, seeds, cols, (src, col_local, seed_pos)): the inputs and the reference."""
    n, seeds, cols = _build(name)
    seeds, cols = seeds.astype(np.int64), cols.astype(np.int64)
    src = np.unique(np.concatenate((seeds, cols)))
    return n, seeds, cols, (src, np.searchsorted(src, cols), np.searchsorted(src, seeds))


def tensor(a, it, dev="cpu"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(it).to(dev)


def assert_block(got, ref, it, dev):
    """(src, col_local, seed_pos) equal to the reference, with the contract's dtypes and device."""
    for g, r, dt, name in zip(got, ref, (it, it, torch.int64), ("src", "col_local", "seed_pos")):
        assert g.dtype == dt and g.dim() == 1 and g.device.type == dev, name
        r = r.cpu().numpy() if isinstance(r, torch.Tensor) else r
        np.testing.assert_array_equal(g.cpu().numpy().astype(np.int64), r.astype(np.int64), err_msg=name)


def torch_route_blocks(row_ptr, col_idx, seeds, fanouts, seed=0):
    """`sample_blocks` as it was before `compact_block`: unique and two searchsorted per layer."""
    blocks, cur = [], seeds
    for layer in reversed(range(len(fanouts))):
        rp_s, ci_s, eid = fs.sample_neighbors(row_ptr, col_idx, cur, fanouts[layer], seed=seed + layer)
        src = torch.unique(torch.cat((cur, ci_s)))
        blocks.append((rp_s, torch.searchsorted(src, ci_s).to(ci_s.dtype), eid, src,
                       torch.searchsorted(src, cur)))
        cur = src
    return blocks[::-1]


def assert_blocks_equal(got, want):
    assert len(got) == len(want)
    for b, w in zip(got, want):
        for x, y, name in zip(b, w, ("row_ptr_s", "col_local", "edge_ids", "src", "seed_pos")):
            assert x.dtype == y.dtype and x.shape == y.shape, name
            assert torch.equal(x.cpu(), y.cpu()), name


# a CSR of 4 rows whose columns reach 9: past its row count
WIDE = (np.array([0, 3, 5, 5, 8]), np.array([1, 6, 9, 0, 3, 2, 8, 9]), np.array([3, 0, 3]))

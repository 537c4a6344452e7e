"""The graph, the node sets and the numpy reference the induced-subgraph tests share (CPU and GPU run
the same table).  The edge bitmap has 32-bit words, 128-bit granules and tiles of
32,768 bits: the boundary graph's rows start and end on both sides of each."""
import functools

import numpy as np
import torch

IDX = {"i32": torch.int32, "i64": torch.int64}
HUB, LOOP, NO_LOOP, DUPES = 8, 3, 1, 6  # rows of the boundary graph
EMPTY_ROWS = 70


@functools.lru_cache(maxsize=None)
def graph():
    """(row_ptr, col_idx), int64: rows cut at 31|32|33, 127|128|129, 65535|65536|65537, a hub of
    40,000 entries across the tile boundary at 32,768, 70 consecutive empty rows, a self-loop (row
    3), rows 1 and 2 whose only columns are far away, a row of 21 equal columns (row 6)."""
    rng = np.random.default_rng(12)
    cuts = [0, 31, 32, 33, 127, 128, 129, 150, 200, 40200]
    while cuts[-1] < 65535 - 60:
        cuts.append(cuts[-1] + int(rng.integers(1, 61)))
    cuts += [65535, 65536, 65537] + [65537] * EMPTY_ROWS
    while len(cuts) < 3001:
        cuts.append(cuts[-1] + int(rng.integers(0, 51)))
    rp = np.array(cuts, dtype=np.int64)
    m = len(rp) - 1
    ci = np.concatenate([np.sort(rng.integers(0, m, d)) for d in np.diff(rp)])
    ci[rp[LOOP]] = LOOP  # row 3: 94 entries, its first the self-loop (still sorted: 3 is small)
    ci[rp[LOOP] + 1:rp[LOOP + 1]] = np.sort(rng.integers(LOOP, m, rp[LOOP + 1] - rp[LOOP] - 1))
    ci[rp[1]], ci[rp[2]] = 2000, 2001
    ci[rp[DUPES]:rp[DUPES + 1]] = 77
    assert m == 3000 and rp[-1] < 150_000 and rp[HUB + 1] - rp[HUB] == 40_000
    return rp, ci


def _nodes(name):
    rp, ci = graph()
    m = len(rp) - 1
    rng = np.random.default_rng(sum(map(ord, name)))
    kind, _, arg = name.partition("-")
    if kind == "all":
        return np.arange(m)
    if kind == "one":
        return np.array([LOOP if arg == "loop" else NO_LOOP])
    if kind == "nothing":  # rows 1 and 2 point at 2000 and 2001
        return np.array([2, 1])
    if kind == "hub":  # the hub alone plus 50 of its neighbours
        return np.concatenate([[HUB], rng.permutation(np.setdiff1d(ci[rp[HUB]:rp[HUB + 1]], [HUB]))[:50]])
    if kind == "shuffled":  # with repeats, the empty rows among them
        return rng.permutation(np.concatenate([rng.integers(0, m, 700), rng.integers(0, m, 300)]))
    return rng.integers(0, m, int(arg))  # sizes-S


CASES = (["all", "one-loop", "one-noloop", "nothing", "hub", "shuffled"]
         + [f"sizes-{s}" for s in (0, 1, 63, 64, 65)])

# a CSR of 4 rows whose columns reach 9: the columns >= 4 are dropped
WIDE = (np.array([0, 3, 5, 5, 8]), np.array([1, 6, 9, 0, 3, 2, 8, 9]), np.array([3, 0, 3, 1]))


def reference(rp, ci, nodes):
    """(src, row_ptr_s, col_local, edge_ids, node_pos), int64: the contract restated in numpy."""
    nodes = np.asarray(nodes, dtype=np.int64)
    src = np.unique(nodes)
    eids = [lo + np.flatnonzero(np.isin(ci[lo:hi], src)) for lo, hi in zip(rp[src], rp[src + 1])]
    eid = np.concatenate(eids + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    rp_s = np.concatenate([[0], np.cumsum([len(e) for e in eids], dtype=np.int64)]).astype(np.int64)
    return src, rp_s, np.searchsorted(src, ci[eid]), eid, np.searchsorted(src, nodes)


@functools.lru_cache(maxsize=None)
def case(name):
    """(row_ptr, col_idx, nodes, reference) of a case of the table, or of "wide"."""
    rp, ci, nodes = WIDE if name == "wide" else (*graph(), _nodes(name))
    return rp, ci, nodes, reference(rp, ci, nodes)


def tensor(a, it, dev="cpu"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(it).to(dev)


def assert_subgraph(got, ref, it, dev):
    """The five arrays equal to the reference, with the contract's dtypes and device."""
    names = ("src", "row_ptr_s", "col_local", "edge_ids", "node_pos")
    for g, r, dt, name in zip(got, ref, (it, it, it, it, torch.int64), names):
        assert g.dtype == dt and g.dim() == 1 and g.device.type == dev, name
        r = r.cpu().numpy() if isinstance(r, torch.Tensor) else r
        np.testing.assert_array_equal(g.cpu().numpy().astype(np.int64), r.astype(np.int64), err_msg=name)


def bad_node_ids(it, m):
    return (-1, m, 2 ** 31 - 1) + ((2 ** 40,) if it == torch.int64 else ())

"""The random walks' contract (include/ofx_spmm.h) restated as a loop over Python
ints, on the sampler's philox4x32-10 restatement (held to Random123's vectors), and the tests'
graphs.  Step t does not depend on the length: a reference serves every shorter one as a prefix."""
import functools
import math

import numpy as np

from tests.node_subgraph_cases import IDX, tensor  # noqa: F401
from tests.sample_neighbors_cases import philox4x32_10

MAX_ATTEMPTS = 256
RETURN, COMMON, OUT = 0, 1, 2
PQ = [(1.0, 1.0), (0.25, 4.0), (4.0, 0.25), (1.0, 2.0)]
SEED = 0x5EED0000000B


def thresholds(p, q):
    w = (1.0 / p, 1.0, 1.0 / q)
    mx = max(w)
    return [2 ** 32 if x == mx else math.floor((x / mx) * 4294967296.0) for x in w]


def words(i, t, a, seed):
    i = np.asarray(i, dtype=np.uint64)
    w = philox4x32_10((i & np.uint64(0xFFFFFFFF), i >> np.uint64(32), t, a),
                      (seed & 0xFFFFFFFF, seed >> 32))
    return w[0], w[1]


def row_has(ci, lo, hi, x):
    end = hi
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if ci[mid] < x:
            lo = mid + 1
        else:
            hi = mid
    return lo < end and ci[lo] == x


def reference(rp, ci, starts, length, p, q, seed):
    """(walks [S, length + 1], edge_ids [S, length], stats): int64 arrays, and what the tests
    assert on the reference itself: classes met, walks ended early, the largest accepted attempt,
    steps accepted at attempt 255, steps t >= 2, attempts."""
    rp, ci = (memoryview(np.ascontiguousarray(a, dtype=np.int64)) for a in (rp, ci))  # Python ints
    m, thr = len(rp) - 1, thresholds(p, q)
    s = len(starts)
    walks = np.full((s, length + 1), -1, dtype=np.int64)
    eids = np.full((s, length), -1, dtype=np.int64)
    met, ended, max_a, capped, biased, attempts = [0, 0, 0], 0, 0, 0, 0, 0
    first = 8  # the attempts whose words come from one table; later ones walk by walk and step
    tab = words(np.arange(s).reshape(-1, 1, 1), np.arange(1, length + 1).reshape(1, -1, 1),
                np.arange(first).reshape(1, 1, -1), seed)
    tab0, tab1 = tab[0].tolist(), tab[1].tolist()
    for i, v in enumerate(int(x) for x in starts):
        assert 0 <= v < m
        walks[i, 0] = v
        u = -1
        for t in range(1, length + 1):
            if not 0 <= v < m or rp[v + 1] == rp[v]:
                ended += 1
                break
            begin, deg = rp[v], rp[v + 1] - rp[v]
            w0s, w1s = tab0[i][t - 1], tab1[i][t - 1]
            for a in range(MAX_ATTEMPTS):
                if a == first:
                    rest = words(i, t, np.arange(first, MAX_ATTEMPTS), seed)
                    w0s, w1s = w0s + rest[0].tolist(), w1s + rest[1].tolist()
                e = begin + ((w0s[a] * deg) >> 32)
                x = ci[e]
                if t == 1 or a == MAX_ATTEMPTS - 1:
                    break
                c = RETURN if x == u else COMMON if row_has(ci, rp[u], rp[u + 1], x) else OUT
                met[c] += 1
                if w1s[a] < thr[c]:
                    break
            max_a, capped = max(max_a, a), capped + (a == MAX_ATTEMPTS - 1)
            biased, attempts = biased + (t >= 2), attempts + a + 1
            walks[i, t], eids[i, t - 1] = x, e
            u, v = v, x
    return walks, eids, dict(met=met, ended=ended, max_attempt=max_a, capped=capped,
                              biased=biased, attempts=attempts)


HUB, LOOP, EMPTY = 5, 2, (0, 1)


@functools.lru_cache(maxsize=None)
def graph(m, wide=True):
    """A canonical CSR of m rows: rows 0 and 1 empty, row 2 with a self-loop, row 5 a hub of 5003
    entries, rows [m/3, 2m/3) a ring j±1, j±2, j±3 (triangles, every edge with its reverse) plus two
    random columns, the others random (duplicates) with every 10th pointing at the hub and the
    empty rows.  `wide`: every 7th random row ends in a column >= m (a non-square CSR)."""
    rng = np.random.default_rng(m)
    lo, hi = m // 3, 2 * m // 3
    n = hi - lo
    rows = []
    for j in range(m):
        if j in EMPTY:
            cols = []
        elif j == HUB:
            cols = rng.integers(0, m, 5003)
        elif lo <= j < hi:
            ring = lo + (j - lo + np.array([-3, -2, -1, 1, 2, 3])) % n
            cols = np.concatenate([ring, rng.integers(0, m, 2)])
        else:
            cols = rng.integers(0, m, min(int(rng.pareto(1.1) * 4) + 1, 300))
            if j % 10 == 0:
                cols = np.concatenate([cols, [HUB, 0, 1]])
            if j == LOOP:
                cols = np.concatenate([cols, [LOOP]])
            if wide and j % 7 == 0:
                cols = np.concatenate([cols, [m + 3]])
        rows.append(np.sort(np.asarray(cols, dtype=np.int64)))
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return rp, np.concatenate(rows)


def starts_of(m, s, rng_seed=0):
    rng = np.random.default_rng(rng_seed)
    return np.concatenate([[HUB, LOOP, EMPTY[0], HUB], rng.integers(0, m, max(s - 4, 0))])[:s]


@functools.lru_cache(maxsize=None)
def case(m, s, pq, length=33):
    """(row_ptr, col_idx, starts, walks, edge_ids, stats) of the wide graph of m rows."""
    rp, ci = graph(m)
    starts = starts_of(m, s)
    return (rp, ci, starts) + reference(rp, ci, starts, length, *pq, SEED)


@functools.lru_cache(maxsize=None)
def ring_case(n=16, s=64, length=121, pq=(1e6, 1e6), seed=1):
    """An even ring: bipartite, so no candidate is common; with p = q = 1e6 a step is accepted
    before attempt 255 with probability 2.6e-4 only."""
    rp = np.arange(n + 1, dtype=np.int64) * 2
    ci = np.stack([(np.arange(n) - 1) % n, (np.arange(n) + 1) % n], 1)
    ci = np.sort(ci, 1).reshape(-1).astype(np.int64)
    starts = np.arange(s, dtype=np.int64) % n
    return (rp, ci, starts, length, pq, seed) + reference(rp, ci, starts, length, *pq, seed)


# walks of case(300, 400, (0.25, 4.0)), written down once: i -> (ten nodes, nine entries).  Walk 0
# leaves the hub and ends on a column >= m, 1 takes the self-loop, 399 turns inside the ring.
KNOWN_WALKS = {
    0: ([5, 289, 265, 70, 303, -1, -1, -1, -1, -1], [4838, 8039, 7757, 5728, -1, -1, -1, -1, -1]),
    1: ([2, 2, 225, 267, 112, 110, 109, 112, 110, 111],
        [0, 4, 7097, 7786, 6017, 6001, 5996, 6017, 6002]),
    399: ([231, 132, 134, 132, 130, 132, 133, 130, 133, 136],
          [7267, 6180, 6194, 6177, 6165, 6179, 6185, 6166, 6190]),
}


def assert_walks(got, walks, eids, it, dev, length=None):
    length = walks.shape[1] - 1 if length is None else length
    for g, r, name in ((got[0], walks[:, :length + 1], "walks"), (got[1], eids[:, :length], "edge_ids")):
        if g is None:
            continue
        assert g.dtype == it and g.device.type == dev and g.is_contiguous(), name
        assert tuple(g.shape) == r.shape, name
        np.testing.assert_array_equal(g.cpu().numpy().astype(np.int64), r, err_msg=name)

"""The checker of the neighbour sampler and the graphs its tests share.

The checker restates the contract of include/ofx_spmm.h ("neighbour sampling over CSR") in numpy
and plain Python, independently of the C++: philox4x32-10 on uint64 arrays, Floyd's algorithm as a
loop over a Python set.  test_sample_neighbors_cpu.py holds it to Random123's known-answer vectors
and to a table of known rows before any kernel is compared with it."""
import functools

import numpy as np

U32 = np.uint64(0xFFFFFFFF)
SH32 = np.uint64(32)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)

# Random123's kat_vectors for philox4x32 with 10 rounds: (counter, key, output)
PHILOX_VECTORS = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
]

# (seed, v, deg, fanout, positions or their beginning)
KNOWN_ROWS = [
    (7, 3, 20, 5, [3, 4, 6, 7, 17]),
    (7, 4, 20, 5, [2, 4, 7, 11, 18]),
    (0, 0, 100, 8, [2, 37, 41, 48, 78, 82, 90, 91]),
    (0x123456789ABCDEF0, 5000000000, 1000, 10, [110, 187, 330, 349, 581, 608, 690, 744, 904, 948]),
    (1, 9, 6, 5, [0, 2, 3, 4, 5]),
    (2 ** 64 - 1, 2449028, 17492, 64, [8, 37, 194, 412, 555, 791, 1128, 1930]),
]


def philox4x32_10(counter, key):
    """The four output words for four counter words and two key words, each a uint64 array (or a
    number) holding 32-bit values; the arrays broadcast."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in counter)
    k0, k1 = (np.asarray(k, dtype=np.uint64) for k in key)
    for _ in range(10):
        p0 = PHILOX_M0 * c0  # 32 x 32 bits: fits 64
        p1 = PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> SH32) ^ c1 ^ k0, p1 & U32, (p0 >> SH32) ^ c3 ^ k1, p0 & U32
        k0, k1 = (k0 + PHILOX_W0) & U32, (k1 + PHILOX_W1) & U32
    return c0, c1, c2, c3


def draws(nodes, fanout, seed):
    """u [len(nodes), fanout]: the first philox word of counter (v lo, v hi, t, 0) under the seed."""
    seed = int(seed) % 2 ** 64
    v = np.asarray(nodes, dtype=np.uint64).reshape(-1, 1)
    t = np.arange(fanout, dtype=np.uint64).reshape(1, -1)
    return philox4x32_10((v & U32, v >> SH32, t, 0), (seed & 0xFFFFFFFF, seed >> 32))[0]


def floyd(u, deg, fanout):
    """The ascending positions of a row of `deg` > fanout entries from its draws u [fanout]."""
    kept = set()
    for t in range(fanout):
        j = deg - fanout + t
        r = (int(u[t]) * (j + 1)) >> 32
        kept.add(j if r in kept else r)
    return sorted(kept)


def row_positions(v, deg, fanout, seed):
    if deg <= fanout:
        return list(range(deg))
    return floyd(draws([v], fanout, seed)[0], deg, fanout)


def reference(row_ptr, col_idx, seeds, fanout, seed):
    """(row_ptr_s, col_idx_s, edge_ids) as int64 arrays."""
    row_ptr, seeds = np.asarray(row_ptr, dtype=np.int64), np.asarray(seeds, dtype=np.int64)
    assert 1 <= fanout <= 64 and ((0 <= seeds) & (seeds < len(row_ptr) - 1)).all()
    u = draws(seeds, fanout, seed)
    rows = []
    for i, v in enumerate(seeds):
        begin, deg = row_ptr[v], int(row_ptr[v + 1] - row_ptr[v])
        pos = list(range(deg)) if deg <= fanout else floyd(u[i], deg, fanout)
        rows.append(begin + np.asarray(pos, dtype=np.int64))
    rp_s = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    eid = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    return rp_s, np.asarray(col_idx, dtype=np.int64)[eid], eid


# ---- graphs -------------------------------------------------------------------------------------
def graph(m, fanout, num_seeds, hubs=(), rng_seed=0):
    """A power-law CSR of m rows (sorted columns, duplicates possible) and num_seeds seeds in
    shuffled order with repeats.  Rows 0..5: empty, degree fanout-1, fanout, fanout+1, 65, about
    5000; the rows after them have the degrees of `hubs`.  Every one of them is among the seeds."""
    rng = np.random.default_rng(rng_seed + 1000 * fanout)
    deg = np.minimum((rng.pareto(1.1, m) * 4).astype(np.int64), 300)
    special = [0, fanout - 1, fanout, fanout + 1, 65, 5003] + list(hubs)
    deg[:len(special)] = special
    row_ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col_idx = np.concatenate([np.sort(rng.integers(0, m, d)) for d in deg]).astype(np.int64)
    seeds = np.concatenate([np.arange(len(special)), np.arange(len(special)),
                            rng.integers(0, m, num_seeds - 2 * len(special))])
    rng.shuffle(seeds)
    return row_ptr, col_idx, seeds.astype(np.int64)


@functools.lru_cache(maxsize=None)
def cpu_case(fanout, seed):
    """The 300-row graph of the CPU tests with about 400 seeds, and its reference."""
    rp, ci, seeds = graph(300, fanout, 400)
    return rp, ci, seeds, reference(rp, ci, seeds, fanout, seed)


@functools.lru_cache(maxsize=None)
def gpu_case(fanout, seed=11):
    """The 3000-row graph of the GPU tests (three hub rows of degree 20000) with 2500 seeds."""
    rp, ci, seeds = graph(3000, fanout, 2500, hubs=(20000, 20000, 20000), rng_seed=1)
    return rp, ci, seeds, reference(rp, ci, seeds, fanout, seed)


def regular_graph(rows, deg):
    """`rows` rows of degree `deg` whose columns are the positions 0..deg-1."""
    row_ptr = np.arange(rows + 1, dtype=np.int64) * deg
    return row_ptr, np.tile(np.arange(deg, dtype=np.int64), rows)

"""The checks of the max / min / mean aggregation, written once for both devices
(test_reduce_cpu.py runs them on host tensors, test_reduce_gpu.py on the GPU, where every result
is also compared with the kCPU kernel's bits).  References: reduce_helpers.py."""
from __future__ import annotations

import functools

import numpy as np
import torch

from helpers import (assert_bitwise, from_f32, power_law_degrees, random_csr, random_dense,
                     to_oracle)
from oracle import oracle
from reduce_helpers import (PAD, acc, assert_same, is_sentinel, options, padding_of, ref_extremum,
                            ref_grad_b, ref_grad_values, ref_mean, ref_row_scale, run_grad_b,
                            run_grad_values, run_reduce, run_row_scale, transpose_t)

WIDTHS = [1, 3, 4, 16, 17, 33, 47, 64, 128, 255, 256, 300]
# Beyond one column tile of the forward and d(b) (64 * VEC columns: 256 f32, 512 16-bit, 128 f64)
# and in the widest layout of the masked SDDMM (n in 513..2048: four leaves per lane), aligned (520,
# 2048) and not (513, 1030); 1030 is three f32 tiles and three 16-bit ones.
WIDE_WIDTHS = [("f32", 513), ("f32", 520), ("f32", 1030), ("f32", 2048), ("bf16", 513),
               ("bf16", 520), ("bf16", 1030), ("f16", 513), ("f16", 520), ("f16", 1030),
               ("f64", 520)]
ROW_LENGTHS = [0, 1, 2, 7, 63, 64, 65]
M, K = 40, 70  # k >= the longest row


def to_dev(dev, *ts):
    return tuple(t.to(dev) for t in ts)


def base_problem(n, dtype, idx_dtype=torch.int32, seed=0, exact=True, m=M, k=K, lengths=None):
    rng = np.random.default_rng(seed + 1000 * n)
    lengths = ROW_LENGTHS if lengths is None else lengths
    deg = np.array([lengths[i % len(lengths)] for i in range(m)])
    rng.shuffle(deg)
    rp, ci, vals = random_csr(m, k, deg, rng, idx_dtype=idx_dtype, val_dtype=dtype, exact=exact)
    b = random_dense(k, n, rng, dtype, exact=exact)
    g = random_dense(m, n, rng, dtype, exact=exact)
    return rp, ci, vals, b, g


def check_all(dev, rp, ci, vals, b, g, m, k, *, pad=0, opts=None, split=0, chunk=0, what="",
              cpu_too=None):
    """Forward max / min (out, arg), mean, d(b) and d(values) of one problem against the numpy
    references, bit for bit; on the GPU also against the kCPU kernel."""
    cpu_too = dev != "cpu" if cpu_too is None else cpu_too
    d = to_dev(dev, rp, ci, vals, b, g)
    rp_t, ci_t, perm = transpose_t(rp, ci, k)
    dt = to_dev(dev, rp_t, ci_t, perm)
    for red in ("max", "min"):
        out, arg = run_reduce(*d[:4], m, k, red, pad=pad, opts=opts)
        ref_out, ref_arg = ref_extremum(rp, ci, vals, b, k, red)
        assert_bitwise(out, ref_out, f"{what} {red} out")
        assert np.array_equal(to_oracle(arg).astype(np.int64), ref_arg), f"{what} {red} arg"
        db = run_grad_b(*dt, d[2], arg, d[4], m, k, pad=pad, opts=opts)
        assert_bitwise(db, ref_grad_b(rp, ci, vals, arg, g, k, split=split, chunk=chunk),
                       f"{what} {red} d(b)")
        dv = run_grad_values(d[0], d[1], arg, d[4], d[3], m, k, pad=pad)
        assert_bitwise(dv, ref_grad_values(rp, ci, arg, g, b), f"{what} {red} d(values)")
        if cpu_too:
            c_out, c_arg = run_reduce(rp, ci, vals, b, m, k, red, pad=pad, opts=opts)
            assert_same(out, c_out, f"{what} {red} out vs kCPU")
            assert_same(arg, c_arg, f"{what} {red} arg vs kCPU")
            assert_same(db, run_grad_b(rp_t, ci_t, perm, vals, c_arg, g, m, k, opts=opts),
                        f"{what} {red} d(b) vs kCPU")
            assert_same(dv, run_grad_values(rp, ci, c_arg, g, b, m, k),
                        f"{what} {red} d(values) vs kCPU")
    mean, _ = run_reduce(*d[:4], m, k, "mean", pad=pad, opts=opts)
    assert_bitwise(mean, ref_mean(rp, ci, vals, b, split=split, chunk=chunk), f"{what} mean")
    if cpu_too:
        assert_same(mean, run_reduce(rp, ci, vals, b, m, k, "mean", opts=opts)[0],
                    f"{what} mean vs kCPU")


def special_problem(dtype):
    """Rows with an all-negative row, +0 / -0 ties, a NaN and +-inf in values and in b, and one
    column index >= K."""
    k, n = 6, 5
    inf, nan = np.inf, np.nan
    b = np.array([[1, -1, 0.0, 2, -2],
                  [-0.0, 0.0, -0.0, 0.0, -0.0],
                  [inf, -inf, 1, nan, -3],
                  [-1, -2, -3, -4, -5],
                  [3, 3, 3, 3, 3],
                  [nan, 1, inf, -inf, 0.0]], dtype=np.float32)
    rows = [([3, 3], [1.0, 2.0]),                    # all negative products
            ([1, 1, 0], [1.0, -1.0, 0.0]),           # +0 / -0 ties: the lowest j wins
            ([2, 4], [1.0, 1.0]),                    # inf and NaN in b
            ([4, 5, 2], [nan, 1.0, 1.0]),            # NaN in values: wins at once, stays
            ([0, 4], [inf, -inf]),                   # inf in values (inf * 0 = NaN in column 2)
            ([9, 3], [1.0, 1.0]),                    # column 9 >= K: a zero row
            ([], []),
            ([5, 2, 0], [-0.0, 1.0, -1.0])]
    rp = np.zeros(len(rows) + 1, dtype=np.int32)
    rp[1:] = np.cumsum([len(c) for c, _ in rows])
    ci = np.array([c for cs, _ in rows for c in cs], dtype=np.int32)
    vals = np.array([v for _, vs in rows for v in vs], dtype=np.float32)
    return (torch.from_numpy(rp), torch.from_numpy(ci), from_f32(vals, dtype), from_f32(b, dtype),
            len(rows), k, n)


def check_special(dev, dtype):
    rp, ci, vals, b, m, k, n = special_problem(dtype)
    g = from_f32(np.arange(1, m * n + 1, dtype=np.float32).reshape(m, n), dtype)
    rp_t, ci_t, perm = transpose_t(rp, ci, k)
    for red in ("max", "min"):
        out, arg = run_reduce(*to_dev(dev, rp, ci, vals, b), m, k, red)
        ref_out, ref_arg = ref_extremum(rp, ci, vals, b, k, red)
        assert_bitwise(out, ref_out, f"special {red} out")
        assert np.array_equal(to_oracle(arg).astype(np.int64), ref_arg), f"special {red} arg"
        assert int(arg[6].max()) == -1 and not out[6].any()  # the empty row
        # the gradients of non-finite inputs: the two kernels agree bit for bit
        c_out, c_arg = run_reduce(rp, ci, vals, b, m, k, red)
        assert_same(out, c_out, f"special {red} out vs kCPU")
        assert_same(arg, c_arg, f"special {red} arg vs kCPU")
        if dev != "cpu":
            d = to_dev(dev, rp, ci, vals, b, g, rp_t, ci_t, perm)
            db = run_grad_b(d[5], d[6], d[7], d[2], arg, d[4], m, k)
            assert_same(db, run_grad_b(rp_t, ci_t, perm, vals, c_arg, g, m, k), "special d(b)")
            dv = run_grad_values(d[0], d[1], arg, d[4], d[3], m, k)
            assert_same(dv, run_grad_values(rp, ci, c_arg, g, b, m, k), "special d(values)")
    # a nonzero that won no column gets +0 whatever b holds: row 3's nonzeros after the NaN
    _, arg = run_reduce(rp, ci, vals, b, m, k, "max")
    dv = run_grad_values(rp, ci, arg, g, b, m, k)
    lost = [j for j in range(len(ci)) if not (to_oracle(arg) == j).any()]
    assert lost and not to_oracle(dv)[lost].view(np.uint8).any()


def hub_tiny_problem(dtype, n=5, idx_dtype=torch.int32):
    """Rows of 8..37 nonzeros for split_threshold=8, chunk=4: the maximum in the first chunk, in
    the last chunk and tied across chunks; and columns as long (hub rows of A^T)."""
    lengths = [8, 9, 11, 12, 16, 37, 9, 12, 37]
    m, k = len(lengths), 40
    rng = np.random.default_rng(7)
    rp, ci, vals = random_csr(m, k, lengths, rng, idx_dtype=idx_dtype, val_dtype=dtype, exact=True)
    v = np.ones(int(rp[-1]), dtype=np.float32)
    rpn = rp.numpy()
    v[rpn[0]] = 2          # first chunk
    v[rpn[2] - 1] = 2      # last chunk (the remainder chunk)
    v[[rpn[2] + 1, rpn[2] + 5, rpn[3] - 1]] = 2  # tied across chunks: the lowest j wins
    v[rpn[5] + 20] = 2
    v[rpn[6]:rpn[7]] = -1  # all equal: tie across every chunk
    b = from_f32(np.ones((k, n), dtype=np.float32) * np.array([1, -1, 2, -2, 1])[None, :n], dtype)
    g = random_dense(m, n, rng, dtype, exact=True)
    return rp, ci, from_f32(v, dtype), b, g, m, k


def transposed_problem(rp, ci, vals, m, k):
    """The CSR of A^T with its values (so that A's long rows become long rows of the gradient's
    transpose)."""
    rp_t, rows_t, perm = oracle.transpose(to_oracle(rp), to_oracle(ci), k)
    np_idx = np.int32 if rp.dtype == torch.int32 else np.int64
    return (torch.from_numpy(rp_t.astype(np_idx)), torch.from_numpy(rows_t.astype(np_idx)),
            vals[torch.from_numpy(perm)], k, m)


def check_hub_tiny(dev, dtype, idx_dtype=torch.int32):
    rp, ci, vals, b, g, m, k = hub_tiny_problem(dtype, idx_dtype=idx_dtype)
    o = options(split=8, chunk=4)
    check_all(dev, rp, ci, vals, b, g, m, k, opts=o, split=8, chunk=4, what="hub tiny")
    # the transposed problem: its d(b) walks hub rows of A (37 entries -> 9 chunks)
    rp2, ci2, v2, m2, k2 = transposed_problem(rp, ci, vals, m, k)
    rng = np.random.default_rng(8)
    b2 = random_dense(k2, b.shape[1], rng, dtype, exact=True)
    g2 = random_dense(m2, b.shape[1], rng, dtype, exact=True)
    check_all(dev, rp2, ci2, v2, b2, g2, m2, k2, opts=o, split=8, chunk=4, what="hub tiny ^T")
    # out and arg do not depend on the schedule
    d = to_dev(dev, rp, ci, vals, b)
    base = run_reduce(*d, m, k, "max", opts=options(ordered=True))
    for oo in (None, o):
        got = run_reduce(*d, m, k, "max", opts=oo)
        assert_same(got[0], base[0], "schedule independence: out")
        assert_same(got[1], base[1], "schedule independence: arg")


def check_hub_default(dev, dtype, n):
    """The default schedule: one row of default_split(n) + 1 and one of 3 * default_split(n) + 5
    nonzeros, and the transposed problem for d(b)."""
    s = oracle.default_split(n)
    lengths = [3, s + 1, 0, 3 * s + 5, s]
    m, k = len(lengths), 3 * s + 40
    rng = np.random.default_rng(n)
    rp, ci, vals = random_csr(m, k, lengths, rng, val_dtype=dtype, exact=True)
    b = random_dense(k, n, rng, dtype, exact=True)
    g = random_dense(m, n, rng, dtype, exact=True)
    check_all(dev, rp, ci, vals, b, g, m, k, what=f"hub default n={n}")
    rp2, ci2, v2, m2, k2 = transposed_problem(rp, ci, vals, m, k)
    b2 = random_dense(k2, n, rng, dtype, exact=True)
    g2 = random_dense(m2, n, rng, dtype, exact=True)
    check_all(dev, rp2, ci2, v2, b2, g2, m2, k2, what=f"hub default ^T n={n}")


def binned_problem(dtype):
    """m >= the planner's kMinBinRows (16384): a binned work list; mean degree 3, two hub rows and
    two hub columns (hub rows of A^T), n = 32."""
    m, k, n = 16400, 2000, 32
    rng = np.random.default_rng(11)
    deg = power_law_degrees(m, 3 * m, k, rng)
    deg[[100, 9000]] = [600, 1100]
    rp, ci, vals = random_csr(m, k, deg, rng, val_dtype=dtype, exact=True)
    rpn, cin = rp.numpy(), ci.numpy()
    rows = np.flatnonzero(np.diff(rpn) > 0)
    for col, cnt in ((0, 700), (1, 1300)):
        for r in rng.choice(rows, size=cnt, replace=False):
            if col not in cin[rpn[r]:rpn[r + 1]] and cin[rpn[r]] > col:
                cin[rpn[r]] = col
    b = random_dense(k, n, rng, dtype, exact=True)
    g = random_dense(m, n, rng, dtype, exact=True)
    return rp, torch.from_numpy(cin), vals, b, g, m, k


def check_row_ranges(dev, dtype):
    rp, ci, vals, b, _ = base_problem(17, dtype)
    d = to_dev(dev, rp, ci, vals, b)
    for red in ("max", "min", "mean"):
        full, full_arg = run_reduce(*d, M, K, red)
        for lo, hi in ((0, 0), (5, 5), (M, M), (0, 13), (3, 17), (17, M)):
            out, arg = run_reduce(*d, M, K, red, pad=PAD, row_begin=lo, row_end=hi)
            assert_same(out, full[lo:hi], f"{red} rows [{lo}, {hi})")
            if red != "mean":  # global nonzero indices: no rebasing to the range
                assert_same(arg, full_arg[lo:hi], f"{red} arg rows [{lo}, {hi})")


def row_ranges(rows):
    """Empty ranges at both ends and inside, a prefix, an inner range and a suffix of `rows`."""
    return (0, 0), (5, 5), (rows, rows), (0, 13), (3, 17), (17, rows)


def assert_values_range(dv, full_dv, rpn, lo, hi, what):
    """d(values) of a launch over rows [lo, hi): the full result on the range's nonzeros, and
    every other entry still the sentinel run_grad_values filled in (never written)."""
    j0, j1 = int(rpn[lo]), int(rpn[hi])
    assert_same(dv[j0:j1], full_dv[j0:j1], f"{what} d(values) rows [{lo}, {hi})")
    kept = is_sentinel(dv)
    assert bool(kept[:j0].all()) and bool(kept[j1:].all()), \
        f"{what} d(values) rows [{lo}, {hi}): wrote outside [{j0}, {j1})"


def check_gradient_row_ranges(dev, dtype):
    """The row ranges of both gradient entries: d(b) over rows [lo, hi) of A^T is that slice of
    the full d(b) (db rebased to the range, arg and g over all rows); d(values) over rows [lo, hi)
    of A writes exactly the range's nonzeros (arg and g rebased to the range, out[j] global)."""
    rp, ci, vals, b, g = base_problem(17, dtype)
    d = to_dev(dev, rp, ci, vals, b, g)
    dt = to_dev(dev, *transpose_t(rp, ci, K))
    rpn = to_oracle(rp).astype(np.int64)
    for red in ("max", "min"):
        _, arg = run_reduce(*d[:4], M, K, red)
        full_db = run_grad_b(*dt, d[2], arg, d[4], M, K)
        full_dv = run_grad_values(d[0], d[1], arg, d[4], d[3], M, K)
        assert_bitwise(full_db, ref_grad_b(rp, ci, vals, arg, g, K), f"{red} d(b)")
        assert_bitwise(full_dv, ref_grad_values(rp, ci, arg, g, b), f"{red} d(values)")
        for lo, hi in row_ranges(K):
            db = run_grad_b(*dt, d[2], arg, d[4], M, K, pad=PAD, row_begin=lo, row_end=hi)
            assert_same(db, full_db[lo:hi], f"{red} d(b) rows [{lo}, {hi})")
        for lo, hi in row_ranges(M):
            dv = run_grad_values(d[0], d[1], arg, d[4], d[3], M, K, pad=PAD, row_begin=lo,
                                 row_end=hi)
            assert_values_range(dv, full_dv, rpn, lo, hi, red)


def hub_ranges(lens, split):
    """Row ranges around the hub rows (len > split) of a problem: one that begins at the longest
    hub row, one that ends just after it, and the longest run of rows that holds no hub."""
    lens = np.asarray(lens)
    rows, out = len(lens), []
    if (lens > split).any():
        h = int(np.argmax(lens))
        out += [(h, rows), (0, h + 1)]
    best, start = (0, 0), 0
    for r in range(rows + 1):
        if r == rows or lens[r] > split:
            if r - start > best[1] - best[0]:
                best = (start, r)
            start = r + 1
    if best[1] > best[0]:
        out.append(best)
    return out


def check_ranges_of(dev, rp, ci, vals, b, g, m, k, opts, split, what):
    """Forward out / arg and d(values) over ranges of A's rows, d(b) over ranges of A^T's rows,
    against the slices of the full-range results (check_all compares those with the references);
    on the GPU also against the kCPU kernels over the same range.  Returns the ranges used."""
    cpu_too = dev != "cpu"
    d = to_dev(dev, rp, ci, vals, b, g)
    t_cpu = transpose_t(rp, ci, k)
    dt = to_dev(dev, *t_cpu)
    rpn = to_oracle(rp).astype(np.int64)
    rows = hub_ranges(np.diff(rpn), split) + [(3, min(17, m))]
    rows_t = hub_ranges(np.diff(to_oracle(t_cpu[0]).astype(np.int64)[:k + 1]), split) + \
        [(3, min(17, k))]
    for red in ("max", "min", "mean"):
        full, full_arg = run_reduce(*d[:4], m, k, red, opts=opts)
        for lo, hi in rows:
            out, arg = run_reduce(*d[:4], m, k, red, pad=PAD, row_begin=lo, row_end=hi, opts=opts)
            assert_same(out, full[lo:hi], f"{what} {red} rows [{lo}, {hi})")
            if cpu_too:
                c_out, c_arg = run_reduce(rp, ci, vals, b, m, k, red, row_begin=lo, row_end=hi,
                                          opts=opts)
                assert_same(out, c_out, f"{what} {red} rows [{lo}, {hi}) vs kCPU")
            if red != "mean":
                assert_same(arg, full_arg[lo:hi], f"{what} {red} arg rows [{lo}, {hi})")
                if cpu_too:
                    assert_same(arg, c_arg, f"{what} {red} arg rows [{lo}, {hi}) vs kCPU")
        if red == "mean":
            continue
        h_arg = full_arg.cpu()
        full_dv = run_grad_values(d[0], d[1], full_arg, d[4], d[3], m, k)
        for lo, hi in rows:
            dv = run_grad_values(d[0], d[1], full_arg, d[4], d[3], m, k, pad=PAD, row_begin=lo,
                                 row_end=hi)
            assert_values_range(dv, full_dv, rpn, lo, hi, f"{what} {red}")
            if cpu_too:
                assert_same(dv, run_grad_values(rp, ci, h_arg, g, b, m, k, row_begin=lo,
                                                row_end=hi),
                            f"{what} {red} d(values) rows [{lo}, {hi}) vs kCPU")
        full_db = run_grad_b(*dt, d[2], full_arg, d[4], m, k, opts=opts)
        for lo, hi in rows_t:
            db = run_grad_b(*dt, d[2], full_arg, d[4], m, k, pad=PAD, opts=opts, row_begin=lo,
                            row_end=hi)
            assert_same(db, full_db[lo:hi], f"{what} {red} d(b) rows [{lo}, {hi})")
            if cpu_too:
                assert_same(db, run_grad_b(*t_cpu, vals, h_arg, g, m, k, opts=opts, row_begin=lo,
                                           row_end=hi),
                            f"{what} {red} d(b) rows [{lo}, {hi}) vs kCPU")
    return rows, rows_t


def check_hub_ranges(dev, dtype):
    """Row ranges over hub rows (split_threshold=8, chunk=4): the planner's hub tables hold rows
    local to a range that starts after row 0.  hub_tiny_problem's rows 1..8 are hubs of the
    forward; the transposed problem makes them the hub rows that d(b) walks."""
    o = options(split=8, chunk=4)
    rp, ci, vals, b, g, m, k = hub_tiny_problem(dtype)
    rows, _ = check_ranges_of(dev, rp, ci, vals, b, g, m, k, o, 8, "hub tiny")
    assert rows[:3] == [(5, 9), (0, 6), (0, 1)]  # begins at a hub, ends after one, holds none
    rp2, ci2, v2, m2, k2 = transposed_problem(rp, ci, vals, m, k)
    rng = np.random.default_rng(8)
    b2 = random_dense(k2, b.shape[1], rng, dtype, exact=True)
    g2 = random_dense(m2, b.shape[1], rng, dtype, exact=True)
    _, rows_t = check_ranges_of(dev, rp2, ci2, v2, b2, g2, m2, k2, o, 8, "hub tiny ^T")
    assert rows_t[:3] == [(5, 9), (0, 6), (0, 1)]


# ---- problems of the planned path ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planned_problem(name):
    """Two f32 problems with exact data and int32 indices that the sum op does not run in its small
    form, so that ofx_spmm_csr_plan plans them and opts->planned is honoured (built once):
    "mid": m = k = 3000, power-law degrees of mean 12, rows 100 / 1000 of 300 / 700 nonzeros (above
      default_split(256) = 256), n = 256: nnz * n > 2^23, the sum's form is mid;
    "many-rows": m = 33000 > 32768 rows, k = 2000, mean degree 2, rows 100 / 20000 of 600 / 1100
      nonzeros, n = 16: a planned form (form=narrow) with a binned work list (m >= 16384), 33
      planner blocks.
    Returns (rp, ci, vals, b, g, m, k); shared, never written."""
    if name == "mid":
        m, k, n, mean, hubs, seed = 3000, 3000, 256, 12, ((100, 300), (1000, 700)), 21
    else:
        m, k, n, mean, hubs, seed = 33000, 2000, 16, 2, ((100, 600), (20000, 1100)), 22
    rng = np.random.default_rng(seed)
    deg = power_law_degrees(m, mean * m, k, rng)
    for r, length in hubs:
        deg[r] = length
    rp, ci, vals = random_csr(m, k, deg, rng, exact=True)
    b = random_dense(k, n, rng, exact=True)
    g = random_dense(m, n, rng, exact=True)
    return rp, ci, vals, b, g, m, k


@functools.lru_cache(maxsize=None)
def planned_reference(name, red):
    """ref_extremum of planned_problem(name): (out, arg int64), computed once."""
    rp, ci, vals, b, _, _, k = planned_problem(name)
    return ref_extremum(rp, ci, vals, b, k, red)


@functools.lru_cache(maxsize=None)
def planned_reference_grad_b(name):
    """ref_grad_b of planned_problem(name) for the arg of max, computed once."""
    rp, ci, vals, _, g, _, k = planned_problem(name)
    arg = torch.from_numpy(planned_reference(name, "max")[1].astype(np.int32))
    return ref_grad_b(rp, ci, vals, arg, g, k)


def check_row_scale(dev, dtype, idx_dtype):
    """ofx_row_scale_by_degree out of place, ldsrc != lddst, over the row range (3, 17) of rows
    whose degrees include 0, 1, 3, 7 and 65: numpy's division in the accumulation type with one
    rounding (ref_row_scale), the kCPU kernel, and dst's padding columns untouched."""
    deg = np.array([2, 0, 5, 0, 1, 3, 7, 65, 2, 4, 0, 1, 3, 7, 65, 6, 9, 1, 1, 1])
    m, n, lo, hi = len(deg), 19, 3, 17
    np_idx = np.int32 if idx_dtype == torch.int32 else np.int64
    rp = torch.from_numpy(np.concatenate([[0], np.cumsum(deg)]).astype(np_idx))
    src = random_dense(hi - lo, n, np.random.default_rng(31), dtype)
    want = ref_row_scale(acc(src), deg[lo:hi], dtype)
    dst = run_row_scale(rp.to(dev), src.to(dev), m, row_begin=lo, row_end=hi, pad_src=3,
                        pad_dst=PAD)
    assert_bitwise(dst, want, "row scale")
    assert bool(is_sentinel(padding_of(dst, PAD)).all()), "row scale wrote dst's padding"
    assert not to_oracle(dst)[deg[lo:hi] == 0].view(np.uint8).any()  # degree 0: +0
    if dev != "cpu":
        assert_same(dst, run_row_scale(rp, src, m, row_begin=lo, row_end=hi, pad_src=1),
                    "row scale vs kCPU")


def check_degenerate(dev, dtype):
    it = torch.int32
    z = lambda *s: torch.zeros(s, dtype=dtype, device=dev)  # noqa: E731
    zi = lambda *s: torch.zeros(s, dtype=it, device=dev)  # noqa: E731
    for red in ("max", "min", "mean"):
        out, arg = run_reduce(zi(1), zi(0), z(0), z(4, 3), 0, 4, red)  # m = 0
        assert out.shape == (0, 3)
        out, arg = run_reduce(zi(6), zi(0), z(0), z(4, 3), 5, 4, red)  # nnz = 0
        assert not to_oracle(out).view(np.uint8).any()
        if red != "mean":
            assert (arg == -1).all()
        rp = torch.tensor([0, 1, 2], dtype=it, device=dev)
        out, arg = run_reduce(rp, zi(2), z(2), z(4, 0), 2, 4, red)  # n = 0
        assert out.shape == (2, 0)
    rp_t = zi(5)
    db = run_grad_b(rp_t, zi(0), zi(0), z(0), torch.full((5, 3), -1, dtype=it, device=dev),
                    z(5, 3), 5, 4)
    assert db.shape == (4, 3) and not to_oracle(db).view(np.uint8).any()

"""The checks of the max / min / mean aggregation, written once for both devices
(test_reduce_cpu.py runs them on host tensors, test_reduce_gpu.py on the GPU, where every result
is also compared with the kCPU kernel's bits).  References: reduce_helpers.py."""
from __future__ import annotations

import numpy as np
import torch

from helpers import (assert_bitwise, from_f32, power_law_degrees, random_csr, random_dense,
                     to_oracle)
from oracle import oracle
from reduce_helpers import (PAD, assert_same, options, ref_extremum, ref_grad_b, ref_grad_values,
                            ref_mean, run_grad_b, run_grad_values, run_reduce, transpose_t)

WIDTHS = [1, 3, 4, 16, 17, 33, 47, 64, 128, 255, 256, 300]
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


def hub_tiny_problem(dtype, n=5):
    """Rows of 8..37 nonzeros for split_threshold=8, chunk=4: the maximum in the first chunk, in
    the last chunk and tied across chunks; and columns as long (hub rows of A^T)."""
    lengths = [8, 9, 11, 12, 16, 37, 9, 12, 37]
    m, k = len(lengths), 40
    rng = np.random.default_rng(7)
    rp, ci, vals = random_csr(m, k, lengths, rng, val_dtype=dtype, exact=True)
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


def check_hub_tiny(dev, dtype):
    rp, ci, vals, b, g, m, k = hub_tiny_problem(dtype)
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

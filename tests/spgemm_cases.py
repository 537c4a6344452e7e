"""The case table and the dense float64 reference the CSR x CSR tests share (CPU and GPU run the
same table).  The device path classes a row of A by ub, the sum of the lengths of
the rows of B it selects: up to 32 (eight lanes a row), up to 512 (a wave), up to 2048 (a block),
above (the block over column ranges).  Values come from a small dyadic set, so every product and
every partial sum is exact in the value dtype and the comparison is for equality."""
import functools

import numpy as np
import pytest
import torch

from tests import row_topk_cases

IDX = {"i32": torch.int32, "i64": torch.int64}
VAL = {"f32": torch.float32, "f64": torch.float64, "f16": torch.float16, "bf16": torch.bfloat16}
PRECISION = {"f32": 24, "f64": 53, "f16": 11, "bf16": 8}
UBS = (1, 32, 33, 512, 513, 2048, 2049)  # each class's bound and the one above it
tensor = row_topk_cases.tensor


def csr(rows):
    """(row_ptr, col_idx) int64 of a list of rows, each a sequence of columns."""
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return rp, np.concatenate([np.asarray(r, dtype=np.int64) for r in rows] + [np.zeros(0, np.int64)])


def classes_case(rng):
    """Every class at ub = 0, 1, its bound and its bound + 1, once with every product on its own
    column and once with most of them colliding in a window of 64 columns; two hub rows of more
    than 2048 distinct columns; empty rows in A and B; a column of A at and above K."""
    n, b_rows, a_rows = 5000, [], []
    pool = range(len(UBS), len(UBS) + 16)  # B rows of 16 columns inside [100, 164)
    single, empty = len(UBS) + 16, len(UBS) + 17
    for u in UBS:
        b_rows.append(np.sort(rng.choice(n, u, replace=False)))
    b_rows += [100 + np.sort(rng.choice(64, 16, replace=False)) for _ in pool]
    b_rows += [[131], []]
    k = len(b_rows)
    for i, u in enumerate(UBS):
        a_rows.append([i])                                                   # distinct = ub
        a_rows.append([pool[j % 16] for j in range(u // 16)] + [single] * (u % 16))  # << ub
    a_rows += [[], [empty], [k, k + 7], [6, 5, k, 3, 6], [5, 6, 4, 3, 2]]  # ub = 0 three times; hubs
    return csr(a_rows), csr(b_rows), n


def crowd_case(_rng):
    """A hub row whose 3300 columns stand inside [70000, 73300) of 100000: the first ranges
    overflow and are halved five times, the ranges on either side are empty."""
    b_rows = [70000 + 3 * np.arange(1100) + r for r in range(3)]
    return csr([[0, 1, 2], [2, 2, 0]]), csr(b_rows), 100000


def small_case(m):
    """m rows of four entries (A's columns repeat), K = 6, n = 11: partial narrow groups."""
    def build(rng):
        b_rows = [np.sort(rng.choice(11, d, replace=False)) for d in (3, 0, 5, 1, 4, 2)]
        return csr([list(rng.integers(0, 6, 2)) * 2 for _ in range(m)]), csr(b_rows), 11
    return build


CASES = {"classes": classes_case, "crowd": crowd_case, "no_b": lambda _: (csr([[0, 2], [1]]), csr([[], [], []]), 4),
         "cancel": lambda _: (csr([[0, 1]]), csr([[2], [2]]), 3),
         **{f"m{m}": small_case(m) for m in (0, 1, 7, 8, 9)}}
LARGE = ("classes", "crowd")  # +-1 alone in the 16-bit dtypes


def dense(mat, vals, shape, absolute=False):
    """The float64 matrix of a CSR: duplicates summed, columns at or above shape[1] dropped."""
    rp, ci = mat
    out = np.zeros(shape)
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    keep = ci < shape[1]
    np.add.at(out, (rows[keep], ci[keep]), np.abs(vals[keep]) if absolute else vals[keep])
    return out


@functools.lru_cache(maxsize=None)
def case(name, val):
    """(A, va, B, vb, n, (row_ptr_c, col_idx_c, values_c)): CSR pairs int64, values float64."""
    rng = np.random.default_rng(11)
    a, b, n = CASES[name](rng)
    levels = [-1.0, 1.0] if name in LARGE and val in ("f16", "bf16") else [-2.0, -1.0, -0.5, 0.5, 1.0, 2.0]
    va, vb = rng.choice(levels, len(a[1])), rng.choice(levels, len(b[1]))
    if name == "cancel":
        va, vb = np.array([1.0, 1.0]), np.array([1.0, -1.0])
    m, k = len(a[0]) - 1, len(b[0]) - 1
    # the premise of the exact comparison: no chain leaves the dtype's integers of the smallest product
    bound = dense(a, va, (m, k), True) @ dense(b, vb, (k, n), True) / min(abs(x) for x in levels) ** 2
    assert bound.max(initial=0.0) < 2.0 ** PRECISION[val], (name, val, bound.max())
    product = dense(a, va, (m, k)) @ dense(b, vb, (k, n))
    pattern = dense(a, np.ones(len(a[1])), (m, k)) @ dense(b, np.ones(len(b[1])), (k, n)) > 0
    rp_c = np.concatenate([[0], np.cumsum(pattern.sum(axis=1))]).astype(np.int64)
    return a, va, b, vb, n, (rp_c, np.nonzero(pattern)[1], product[pattern])


def operands(name, val, it, dev="cpu"):
    """The seven arguments of fs.spgemm for a case."""
    a, va, b, vb, n, _ = case(name, val)
    vt = VAL[val]
    return (tensor(a[0], it, dev), tensor(a[1], it, dev), tensor(va, vt, dev), tensor(b[0], it, dev),
            tensor(b[1], it, dev), tensor(vb, vt, dev), n)


def assert_csr(got, ref, it, vt, dev):
    """(row_ptr_c, col_idx_c, values_c) equal to the reference's; a zero is +0."""
    ref = [r.cpu().double().numpy() if isinstance(r, torch.Tensor) else r for r in ref]
    for g, r, name, dt in zip(got, ref, ("row_ptr_c", "col_idx_c", "values_c"), (it, it, vt)):
        assert g.dtype == dt and g.dim() == 1 and g.device.type == dev, name
        np.testing.assert_array_equal(g.cpu().double().numpy(), r.astype(np.float64), err_msg=name)
    assert not torch.signbit(got[2][got[2] == 0]).any()


def check_case(fs, name, val, idx, dev):
    """The valued call against the reference, pattern only against the valued call."""
    it, vt = IDX[idx], VAL[val]
    args = operands(name, val, it, dev)
    got = fs.spgemm(*args)
    assert_csr(got, case(name, val)[5], it, vt, dev.type)
    rp_p, ci_p, none = fs.spgemm(args[0], args[1], None, args[3], args[4], None, args[6])
    assert none is None and torch.equal(rp_p, got[0]) and torch.equal(ci_p, got[1])
    return got


ORDER = (csr([[0, 1, 0, 1]]), np.array([1e8, 1.0, -1e8, 1.0], np.float32),
         csr([[0, 2], [0, 2]]), np.array([1.0, 1e8, 1.0, 1.0], np.float32), 3)


def order_reference():
    """Column -> float32 sum of the order-sensitive case, in the contract's order: any other order
    of the terms 1e8, 1, -1e8, 1 of column 0 gives another float32."""
    (_, ci_a), va, (rp_b, ci_b), vb, _ = ORDER
    acc = {}
    for p, ca in enumerate(ci_a):
        for q in range(rp_b[ca], rp_b[ca + 1]):
            acc[ci_b[q]] = np.float32(acc.get(ci_b[q], np.float32(0)) + np.float32(va[p] * vb[q]))
    return acc


def check_order(fs, dev):
    (rp_a, ci_a), va, (rp_b, ci_b), vb, n = ORDER
    i32 = torch.int32
    got = fs.spgemm(tensor(rp_a, i32, dev), tensor(ci_a, i32, dev), torch.from_numpy(va).to(dev),
                    tensor(rp_b, i32, dev), tensor(ci_b, i32, dev), torch.from_numpy(vb).to(dev), n)
    acc = order_reference()
    assert acc[0] == 1.0 and got[1].tolist() == sorted(acc)
    assert got[2].cpu().numpy().view(np.uint32).tolist() == [acc[c].view(np.uint32) for c in sorted(acc)]


def check_chain(fs, dev):
    """spgemm takes its own output as B, and spmm takes it as a CSR."""
    rng = np.random.default_rng(3)
    mask = rng.random((40, 40)) < 0.08
    a = csr([np.nonzero(r)[0] for r in mask])
    va = rng.choice([-1.0, 0.5, 1.0], len(a[1]))
    d = dense(a, va, (40, 40))
    t = [tensor(a[0], torch.int32, dev), tensor(a[1], torch.int32, dev), tensor(va, torch.float32, dev)]
    sq = fs.spgemm(*t, *t, 40)
    cube = fs.spgemm(*t, *sq, 40)
    ref, pattern = d @ d @ d, (mask.astype(float) @ mask @ mask) > 0
    assert_csr(cube, (np.concatenate([[0], np.cumsum(pattern.sum(axis=1))]), np.nonzero(pattern)[1],
                      ref[pattern]), torch.int32, torch.float32, dev.type)
    x = rng.choice([-1.0, 1.0, 2.0], (40, 5))
    out = fs.spmm(*sq, 40, 40, tensor(x, torch.float32, dev))
    np.testing.assert_array_equal(out.cpu().double().numpy(), d @ (d @ x))


def bad_inputs():
    """A good (A, B, n) whose row_ptr the broken ones of row_topk_cases fit, and the bad variants
    as (which of the four index arrays, its replacement)."""
    rp, ci, _ = row_topk_cases.graph()
    two = int(np.nonzero(np.diff(rp) >= 2)[0][0])  # a row of B with a pair of entries
    j = rp[two]
    bad = [(w, r) for w in (0, 2) for r in row_topk_cases.bad_row_ptrs(rp)]
    for which, at, value in ((1, 3, -1), (3, j + 1, 4000), (3, j + 1, ci[j]), (3, j, ci[j + 1] + 1)):
        broken = ci.copy()
        broken[at] = value
        bad.append((which, broken))
    return (rp, ci), 4000, bad


def check_bad_inputs(fs, idx, dev):
    it = IDX[idx]
    (rp, ci), n, bad = bad_inputs()
    good = [tensor(rp, it, dev), tensor(ci, it, dev), tensor(rp, it, dev), tensor(ci, it, dev)]
    ones = np.ones(len(ci))
    pattern = dense((rp, ci), ones, (len(rp) - 1,) * 2) @ dense((rp, ci), ones, (len(rp) - 1, n)) > 0
    for which, broken in bad:
        args = list(good)
        args[which] = tensor(broken, it, dev)
        with pytest.raises(RuntimeError, match="outside|ascending"):
            fs.spgemm(args[0], args[1], None, args[2], args[3], None, n)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    got = fs.spgemm(good[0], good[1], None, good[2], good[3], None, n)
    assert got[2] is None and got[0].tolist() == [0] + np.cumsum(pattern.sum(axis=1)).tolist()
    assert got[1].tolist() == np.nonzero(pattern)[1].tolist()

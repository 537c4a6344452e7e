"""The graph, the value patterns and the numpy reference the per-row top-k tests share (CPU and GPU
run the same table).  The device path has three row classes: up to 64 entries (eight
lanes a row), up to 512 (a wave a row) and hub rows (a block a row, emission in chunks of 1024
entries); the degrees stand on both sides of each bound and of every parametrised k."""
import functools

import numpy as np
import torch

import oneflow_spmm as fs

IDX = {"i32": torch.int32, "i64": torch.int64}
VAL = {"f32": torch.float32, "f64": torch.float64, "f16": torch.float16, "bf16": torch.bfloat16}
BITS = {torch.float32: np.uint32, torch.float64: np.uint64, torch.float16: np.uint16,
        torch.bfloat16: np.uint16}
MANTISSA = {torch.float32: 23, torch.float64: 52, torch.float16: 10, torch.bfloat16: 7}
KS = (1, 3, 64, 200, 600)
# (degree, pattern): 0 distinct, 1 four levels, 2 all equal, 3 specials.  Every k has k-1, k, k+1;
# 1300 and 2600 cross one and two emission chunks; the last row is empty.
ROWS = ((0, 0), (1, 3), (2, 0), (3, 1), (4, 2), (5, 3), (7, 0), (8, 1), (9, 3), (63, 0), (64, 1),
        (65, 2), (66, 3), (0, 0), (128, 1), (129, 0), (199, 1), (200, 2), (201, 3), (300, 1),
        (511, 0), (512, 1), (512, 2), (513, 3), (513, 2), (599, 0), (600, 1), (601, 2), (700, 3),
        (1024, 1), (1025, 0), (1300, 1), (1300, 3), (2600, 2), (2600, 0), (2048, 3), (40, 2),
        (10, 1), (0, 0))
WAVE_MAX = 512


@functools.lru_cache(maxsize=None)
def graph():
    """(row_ptr, col_idx, values), int64 and float64: rows sorted by column."""
    rng = np.random.default_rng(7)
    deg = np.array([d for d, _ in ROWS])
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    ci = np.concatenate([np.sort(rng.choice(4000, d, replace=False)) for d in deg]).astype(np.int64)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1e-40, -1e-40, 5e-324, 1.0, -1.0])
    vals = []
    for d, pattern in ROWS:
        if pattern == 0:
            vals.append(rng.permutation(d) - d / 3.0)
        elif pattern == 1:
            vals.append(rng.choice([-2.0, 0.5, 0.75, 3.0], d))
        elif pattern == 2:
            vals.append(np.full(d, -1.5))
        else:
            vals.append(rng.choice(special, d))
    return rp, ci, np.concatenate(vals)


def key_of(bits, largest):
    """The contract's key of a value's bit pattern (an unsigned numpy array)."""
    sign = bits.dtype.type(1) << bits.dtype.type(8 * bits.dtype.itemsize - 1)
    key = np.where(bits & sign != 0, ~bits, bits ^ sign)
    return key if largest else ~key


def bits_of(values):
    """The bit patterns of a CPU tensor of values, unsigned."""
    raw = values.view(torch.int16) if values.dtype == torch.bfloat16 else values
    return raw.numpy().view(BITS[values.dtype])


def reference(rp, values, k, largest):
    """(row_ptr_s, edge_ids), int64, plus per row whether the k-th and (k+1)-th keys are equal and
    whether a NaN is kept: a few lines of numpy per row."""
    bits = bits_of(values)
    nan = torch.isnan(values).numpy()
    eids, ties, nans = [], [], []
    for lo, hi in zip(rp[:-1], rp[1:]):
        key = key_of(bits[lo:hi], largest)
        order = np.argsort(~key, kind="stable")
        keep = np.sort(order[:k]) + lo
        eids.append(keep)
        ties.append(hi - lo > k and key[order[k - 1]] == key[order[k]])
        nans.append(bool(nan[keep].any()))
    rp_s = np.concatenate([[0], np.cumsum([len(e) for e in eids])]).astype(np.int64)
    return rp_s, np.concatenate(eids + [np.zeros(0, dtype=np.int64)]).astype(np.int64), ties, nans


@functools.lru_cache(maxsize=None)
def case(k, largest, val):
    """(row_ptr, col_idx, values tensor of dtype `val`, (row_ptr_s, edge_ids))."""
    rp, ci, v = graph()
    values = torch.from_numpy(v).to(VAL[val])
    # a conversion may give every NaN one sign: both quiet NaNs are written as bits, by v's sign
    bits, nan, neg = bits_of(values), np.isnan(v), np.signbit(v)
    sign = 1 << (8 * bits.dtype.itemsize - 1)
    quiet = (sign - 1) ^ ((1 << (MANTISSA[VAL[val]] - 1)) - 1)
    bits[nan & ~neg], bits[nan & neg] = quiet, quiet | sign
    rp_s, eid, ties, nans = reference(rp, values, k, largest)
    # Sharp for every k: the tie rule decides a hub row and (where a row of at most 512 entries
    # can be longer than k at all) a register-path row, and a NaN is among the kept entries.
    deg = np.diff(rp)
    assert any(t and d > WAVE_MAX for t, d in zip(ties, deg)), (k, largest, val)
    assert k >= WAVE_MAX or any(t and d <= WAVE_MAX for t, d in zip(ties, deg)), (k, largest, val)
    assert any(nans), (k, largest, val)
    return rp, ci, values, (rp_s, eid)


def tensor(a, it, dev="cpu"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(it).to(dev)


def assert_topk(got, ref, ci, it, dev):
    """The three arrays equal to (row_ptr_s, edge_ids) of the reference, dtype and device too."""
    rp_s, eid = (r.cpu().numpy() if isinstance(r, torch.Tensor) else r for r in ref)
    for g, r, name in zip(got, (rp_s, ci[eid], eid), ("row_ptr_s", "col_idx_s", "edge_ids")):
        assert g.dtype == it and g.dim() == 1 and g.device.type == dev, name
        np.testing.assert_array_equal(g.cpu().numpy().astype(np.int64), r.astype(np.int64), err_msg=name)


def uniform_rows(m, deg=9):
    """m rows of `deg` entries with values that repeat: (row_ptr, col_idx, values float32)."""
    rng = np.random.default_rng(m)
    rp = np.arange(m + 1, dtype=np.int64) * deg
    return rp, rng.integers(0, 50, m * deg), torch.from_numpy(rng.integers(0, 4, m * deg).astype(np.float32))


def bad_row_ptrs(rp):
    """row_ptr descending, a row ending past nnz, the end of the hub row of 1300 entries spoiled."""
    hub = [d for d, _ in ROWS].index(1300)
    for at, value in ((5, rp[4] - 1), (len(rp) - 1, rp[-1] + 1), (hub + 1, rp[hub] - 7)):
        broken = rp.copy()
        broken[at] = value
        yield broken


def attention_case():
    """A 300-row graph with features: (row_ptr, col_idx) int32 numpy, q, kf, h float32 tensors.  A
    row holds no entry or at least two: a lone kept entry has softmax 1 and a gradient of zero."""
    rng = np.random.default_rng(5)
    deg = rng.integers(2, 12, 300) * (rng.integers(0, 8, 300) > 0)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    ci = np.concatenate([np.sort(rng.choice(300, d, replace=False)) for d in deg]).astype(np.int32)
    q, kf, h = (torch.from_numpy(rng.uniform(-1, 1, (300, 8)).astype(np.float32)) for _ in range(3))
    return rp, ci, q, kf, h


def check_attention(dev):
    """`sddmm`, `row_topk` with k = 4, `edge_softmax` and `spmm` on the kept entries: the bits of
    the same ops on the CSR the reference selects, and a gradient exactly at the kept scores."""
    rp, ci, q, kf, h = attention_case()
    rp_t, ci_t = torch.from_numpy(rp).to(dev), torch.from_numpy(ci).to(dev)
    s = fs.sddmm(rp_t, ci_t, q.to(dev), kf.to(dev)).detach().requires_grad_(True)
    rp_s, ci_s, eid = fs.row_topk(rp_t, ci_t, s, 4)
    out = fs.spmm(rp_s, ci_s, fs.edge_softmax(rp_s, ci_s, s[eid.long()]), 300, 300, h.to(dev))
    ref_rp, ref_eid = reference(rp.astype(np.int64), s.detach().cpu(), 4, True)[:2]
    assert_topk((rp_s, ci_s, eid), (ref_rp, ref_eid), ci, torch.int32, dev.type)
    r_rp, r_eid = torch.from_numpy(ref_rp).int().to(dev), torch.from_numpy(ref_eid).to(dev)
    want = fs.spmm(r_rp, ci_t[r_eid], fs.edge_softmax(r_rp, ci_t[r_eid], s.detach()[r_eid]), 300, 300,
                   h.to(dev))
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    (out * torch.arange(1.0, 9.0, device=dev)).sum().backward()
    touched = torch.zeros(len(ci), dtype=torch.bool)
    touched[ref_eid] = True
    assert torch.equal(s.grad.cpu() != 0, touched)

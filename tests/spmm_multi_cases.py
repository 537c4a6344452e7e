"""The case table, the references and the checks the multi-aggregator SpMM tests share (op
"spmm_csr_multi"; test_spmm_multi_cpu.py and test_spmm_multi_gpu.py run the same table; contract in
include/ofx_spmm.h).  Inputs come from {+-0.5, +-1, +-2} (+-1 alone for the 16-bit
types on the long rows), so every product p, every p * p and every partial sum of s1 and s2 is
exact: the sum / mean / max / min slices and the args equal a plain float64 numpy loop bit for bit,
and var / std equal the contract restated in numpy in the accumulation type from the exact moments."""
from __future__ import annotations

import functools

import numpy as np
import torch

import oneflow_spmm as flow_spmm
from helpers import DTYPES
from oneflow_spmm import _C, ops
from reduce_helpers import options, padded, run_reduce

AGGRS = tuple(_C.AGGR_BITS)  # sum, mean, max, min, var, std: the stored order
PRECISION = {"f32": 24, "f64": 53, "f16": 11, "bf16": 8}
EPS = 1e-5
K = 97
HUB = ops.default_split(64) + 1  # one more than the default schedule sums in one chain


def lens(lpr):
    """Row lengths 0, 1, the lane group +- 1, one load batch (8) +- 1, 17 (split8: chunks 8 + 9)."""
    return (0, 1, lpr - 1, lpr, lpr + 1, 7, 8, 9, 17, 3)


# name: (dtype, index, N, row lengths, keyword extras).  The lane group of N columns is the power
# of two in {1, 4, 16, 32, 64} that holds ceil(N / VEC) lanes, VEC = 16 bytes of the dtype.
CASES = {
    "f32_n64": ("f32", "i32", 64, lens(16) + (HUB,), {}),
    "f32_n64_split8": ("f32", "i32", 64, lens(16), dict(split=8)),
    "f32_n64_rows": ("f32", "i32", 64, lens(16) + (HUB,), dict(split=8, rows=(2, 9))),
    "f32_n64_ld": ("f32", "i32", 64, lens(16), dict(split=8, pad=1, shift=1)),
    "f32_n64_subset": ("f32", "i32", 64, lens(16), dict(split=8, aggrs=("std", "max"))),
    "f32_n16": ("f32", "i32", 16, lens(4), {}),
    "f32_n1": ("f32", "i32", 1, lens(4), {}),
    "f32_n3": ("f32", "i32", 3, lens(4), dict(split=8)),
    "f32_n4": ("f32", "i32", 4, lens(1), dict(split=8)),
    "f32_n5": ("f32", "i32", 5, lens(4), {}),
    "f32_n260": ("f32", "i32", 260, lens(64), dict(split=8)),
    "f32_n128_i64": ("f32", "i64", 128, lens(32), dict(split=8)),
    "f32_specials": ("f32", "i32", 8, (6, 2, 0), dict(specials=True)),
    "f64_n8": ("f64", "i32", 8, lens(4), dict(split=8)),
    "f64_n64": ("f64", "i32", 64, lens(32) + (HUB,), {}),
    "bf16_n128": ("bf16", "i32", 128, lens(16) + (130,), dict(unit=True, split=8)),
    "bf16_n7": ("bf16", "i32", 7, lens(4), {}),
    "f16_n64": ("f16", "i32", 64, lens(8) + (HUB,), dict(unit=True)),
}


def rounded(x, dt):
    return torch.from_numpy(np.asarray(x, dtype=np.float64)).to(DTYPES[dt]).double().numpy()


@functools.lru_cache(maxsize=None)
def problem(name):
    """(rp, ci, values, b) as host tensors of the case's dtypes.  Every row of three or more
    nonzeros repeats a column; the second and third nonzero of every eighth row lie at and above K."""
    dt, it, n, row_lens, kw = CASES[name]
    rng = np.random.default_rng(len(name) + n)
    rp = np.concatenate([[0], np.cumsum(row_lens)]).astype(np.int64)
    ci = rng.integers(0, K, rp[-1])
    for r, length in enumerate(row_lens):
        if length >= 3:
            ci[rp[r] + 2] = ci[rp[r]]
            if r % 8 == 3:
                ci[rp[r] + 1: rp[r] + 3] = (K, K + 5)
    pool = np.array([-1.0, 1.0]) if kw.get("unit") else np.array([-2, -1, -.5, .5, 1, 2.0])
    vals, b = rng.choice(pool, rp[-1]), rng.choice(pool, (K, n))
    if kw.get("specials"):  # row 0: a NaN, +inf, -inf and a -0 / +0 tie, one column each
        ci[:6] = np.arange(6)
        vals[:6] = 1.0
        b[:6] = rng.choice([1.0, 2.0], (6, n))
        b[2, 0], b[1, 1], b[3, 2] = np.nan, np.inf, -np.inf
        b[:6, 3] = (-0.0, 0.0, 0.0, -0.0, 0.0, 0.0)
    idt = torch.int32 if it == "i32" else torch.int64
    as_t = lambda x: torch.from_numpy(x).to(DTYPES[dt])  # noqa: E731
    return torch.from_numpy(rp).to(idt), torch.from_numpy(ci).to(idt), as_t(vals), as_t(b)


@functools.lru_cache(maxsize=None)
def reference(name):
    """Per stored aggregator the float64 value [M, N] (sum / mean / max / min rounded where the
    contract rounds; var / std unrounded), the args, and var / std by the contract in the
    accumulation type from the exact moments, with the tolerance of each; computed once."""
    dt = CASES[name][0]
    rp, ci, vals, b = (t.double().numpy() if t.is_floating_point() else t.numpy()
                       for t in problem(name))
    m, n = len(rp) - 1, b.shape[1]
    s1, s2, mx, mn = (np.zeros((m, n)) for _ in range(4))
    amax, amin = (np.full((m, n), -1, np.int64) for _ in range(2))
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(m):
            for j in range(rp[r], rp[r + 1]):
                p = rounded(vals[j] * (b[ci[j]] if ci[j] < K else np.zeros(n)), dt)
                s1[r], s2[r] = s1[r] + p, s2[r] + p * p
                first = amax[r] < 0  # the strict walk: the lowest j wins ties, the first NaN stays
                tmax = first | (p > mx[r]) | (np.isnan(p) & ~np.isnan(mx[r]))
                tmin = first | (p < mn[r]) | (np.isnan(p) & ~np.isnan(mn[r]))
                mx[r], amax[r] = np.where(tmax, p, mx[r]), np.where(tmax, j, amax[r])
                mn[r], amin[r] = np.where(tmin, p, mn[r]), np.where(tmin, j, amin[r])
        # the bound that makes equality exact: s1 is a multiple of 1/4 and s2 of 1/16, both exact
        # in the f32 accumulator below 2^24 units
        fin = np.isfinite(s2)
        assert 16 * max(np.abs(s1[fin]).max(), s2[fin].max()) < 2 ** 24
        acc = np.float64 if dt == "f64" else np.float32
        u = 2.0 ** -(53 if dt == "f64" else 24)
        deg = np.diff(rp).astype(np.float64)[:, None]
        safe = np.maximum(deg, 1)
        out = {"sum": rounded(s1, dt), "max": mx, "min": mn}
        out["mean"] = np.where(deg > 0, rounded((out["sum"] / safe).astype(acc), dt), 0.0)
        mu64 = s1 / safe
        out["var"] = np.where(deg > 0, np.maximum(s2 / safe - mu64 * mu64, 0.0), 0.0)
        out["std"] = np.sqrt(out["var"] + EPS)
        # the contract in the accumulation type (numpy's float32 / float64 arithmetic is IEEE's)
        a1, a2, ad = s1.astype(acc), s2.astype(acc), safe.astype(acc)
        mu = a1 / ad
        v = a2 / ad - mu * mu
        var = np.where(deg > 0, np.where(v < 0, acc(0), v), acc(0)).astype(acc)
        bits = {"var": rounded(var, dt), "std": rounded(np.sqrt(var + acc(EPS)), dt)}
        # |var - var64| <= 4u (s2 / deg + mu^2): two divisions, a square and a subtraction, each
        # within u of operands bounded by those two terms; then one rounding to T.  std: the error
        # of var and of the addition through sqrt's slope 1 / (2 sqrt(.)) <= 1 / sqrt(var64 + eps),
        # sqrt's own rounding, one rounding to T.
        ut = 2.0 ** -PRECISION[dt]
        tv = 4 * u * (s2 / safe + mu64 * mu64)
        ts = (tv + u * (out["var"] + EPS)) / out["std"] + u * out["std"]
        tol = {"var": tv + ut * (out["var"] + tv), "std": ts + ut * (out["std"] + ts)}
    return out, {"max": amax, "min": amin}, bits, tol


def same(got, want, what):
    """Bit for bit (the sign of a zero included); a NaN where the reference has one."""
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else got
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions differ"
    bad = np.flatnonzero((got.view(np.int64) != want.view(np.int64)).ravel() & ~nan.ravel())
    assert bad.size == 0, f"{what}: {bad.size} elements differ, first at flat index {bad[0]}: " \
                          f"{got.ravel()[bad[0]]!r} != {want.ravel()[bad[0]]!r}"


def bits_equal(a, b, what):
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    assert torch.equal(a.cpu().contiguous().view(it), b.cpu().contiguous().view(it)), what


def stored(name):
    """The case's aggregators in the stored order."""
    return [a for a in AGGRS if a in CASES[name][4].get("aggrs", AGGRS)]


def run(dev, name, num_threads=0):
    """(out [rows, A, N], arg_max, arg_min) of the C-ABI entry on `dev` for a case: its aggregators,
    schedule, row range, leading dimension and base shift (b, and the output buffer)."""
    kw = CASES[name][4]
    rp, ci, vals, b = (t.to(dev) for t in problem(name))
    m, n = rp.numel() - 1, b.shape[1]
    nt = dict(num_threads=num_threads) if b.device.type == "cpu" else {}
    o = options(split=kw["split"], chunk=kw["split"]) if "split" in kw else None
    lo, hi = kw.get("rows", (0, m))
    pad, shift, slices = kw.get("pad", 0), kw.get("shift", 0), len(stored(name))
    buf = torch.full(((hi - lo) * slices * (n + pad) + shift,), float("nan"), dtype=b.dtype,
                     device=b.device)
    out = buf[shift:].view(hi - lo, slices, n + pad)[:, :, :n]
    mask = _C.aggr_mask(stored(name))
    return ops.spmm_csr_multi(rp, ci, vals, padded(b, pad, shift), m, K, mask, EPS, out=out,
                              row_begin=lo, row_end=hi, options=o, **nt)


def check_case(dev, name):
    """Checks 1-4 of a case on `dev`: the float64 reference, var / std's bits and tolerance, and
    the existing ops on the same inputs and options."""
    dt, _, _, _, kw = CASES[name]
    want, want_arg, bits, tol = reference(name)
    rp, ci, vals, b = (t.to(dev) for t in problem(name))
    m = rp.numel() - 1
    lo, hi = kw.get("rows", (0, m))
    out, arg_max, arg_min = run(dev, name)
    o = options(split=kw["split"], chunk=kw["split"]) if "split" in kw else None
    for i, a in enumerate(stored(name)):
        got, what = out[:, i, :], f"{name} {a} on {dev}"
        if a in ("var", "std"):
            same(got, bits[a][lo:hi], f"{what}: the contract's bits")
            err = np.abs(got.double().cpu().numpy() - want[a][lo:hi])
            fin = np.isfinite(want[a][lo:hi])
            print(f"{what}: max error {err[fin].max(initial=0):.3e}, "
                  f"bound there {tol[a][lo:hi][fin].max(initial=0):.3e}")
            assert (err[fin] <= tol[a][lo:hi][fin]).all(), f"{what}: outside the derived bound"
            continue
        same(got, want[a][lo:hi], f"{what}: float64 reference")
        old, old_arg = run_reduce(rp, ci, vals, b, m, K, a, row_begin=lo, row_end=hi, opts=o)
        bits_equal(got, old, f"{what}: the existing op's bits")
        if a in ("max", "min"):
            arg = arg_max if a == "max" else arg_min
            assert np.array_equal(arg.cpu().numpy(), want_arg[a][lo:hi]), f"{what}: arg"
            assert torch.equal(arg, old_arg), f"{what}: the existing op's arg"


def grad_problem(dev):
    """Continuous float64 inputs, degrees 0, 1 and up to 8: no ties, no variance at the clamp apart
    from the rows of degree 0 and 1."""
    rng = np.random.default_rng(11)
    row_lens = (3, 0, 1, 8, 5, 2, 1, 7, 4, 0, 6, 3)
    rp = torch.from_numpy(np.concatenate([[0], np.cumsum(row_lens)]).astype(np.int32))
    ci = torch.from_numpy(rng.integers(0, 9, int(rp[-1])).astype(np.int32))
    vals, b, w = (torch.from_numpy(rng.standard_normal(s))
                  for s in (int(rp[-1]), (9, 5), (len(row_lens), len(AGGRS), 5)))
    return tuple(t.to(dev) for t in (rp, ci, vals, b, w))


def dense_multi(rp, ci, vals, b, aggrs):
    """The plain torch restatement: per row the messages and their statistics."""
    rows = []
    for r in range(rp.numel() - 1):
        j0, j1 = int(rp[r]), int(rp[r + 1])
        p = vals[j0:j1, None] * b[ci[j0:j1].long()]
        if j0 == j1:
            zero = torch.zeros(b.shape[1], dtype=b.dtype, device=b.device)
            st = {a: zero for a in AGGRS}
            st["std"] = zero + EPS ** 0.5
        else:
            var = ((p * p).mean(0) - p.mean(0) ** 2).clamp(min=0)
            st = {"sum": p.sum(0), "mean": p.mean(0), "max": p.max(0).values,
                  "min": p.min(0).values, "var": var, "std": (var + EPS).sqrt()}
        rows.append(torch.stack([st[a] for a in aggrs]))
    return torch.stack(rows)


def check_gradients(dev, aggrs=AGGRS):
    rp, ci, vals, b, w = grad_problem(dev)
    w = w[:, :len(aggrs)]
    grads = []
    for f in (lambda v, x: flow_spmm.spmm_multi(rp, ci, v, rp.numel() - 1, 9, x, aggrs, EPS),
              lambda v, x: dense_multi(rp, ci, v, x, aggrs)):
        v, x = vals.clone().requires_grad_(), b.clone().requires_grad_()
        out = f(v, x)
        grads.append((out.detach(),) + torch.autograd.grad((out * w).sum(), (v, x)))
    for got, want, what in zip(*grads, ("out", "d(values)", "d(b)")):
        torch.testing.assert_close(got, want, msg=lambda s: f"{aggrs} {what} on {dev}: {s}")  # noqa: B023

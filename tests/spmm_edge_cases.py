"""The case table, the reference and the checks the edge-feature SpMM tests share (ops
"spmm_csr_edge", "_grad_e", "_grad_b"; test_spmm_edge_cpu.py and test_spmm_edge_gpu.py run the same
table; contract in include/ofx_spmm.h).  The reference is a plain float64 numpy
loop over rows and nonzeros.  Inputs come from {+-0.5, +-1, +-2} (+-1 alone for the 16-bit types
on the long rows), so every product, sum and rounding is exact and equality with the reference is
bit for bit: no tolerance.  One table drives the forward and both gradients."""
from __future__ import annotations

import functools

import numpy as np
import torch

import oneflow_spmm as flow_spmm
from helpers import DTYPES
from oneflow_spmm import ops
from reduce_helpers import options, padded

OPS = {"mul": 0, "add": 1}
ACTS = {None: 0, "relu": 1}
PAIRS = [("mul", None), ("mul", "relu"), ("add", None), ("add", "relu")]
PRECISION = {"f32": 24, "f64": 53, "f16": 11, "bf16": 8}
K = 97
HUB = ops.default_split(64) + 1  # one more than the default schedule sums in one chain
assert HUB == ops.default_split(128) + 1


def lens(lpr):
    """Row lengths 0, 1, the lane group +- 1, one load batch (8) +- 1, 17 (split8: chunks 8 + 9)."""
    return (0, 1, lpr - 1, lpr, lpr + 1, 7, 8, 9, 17, 3)


# name: (dtype, index, N, row lengths, keyword extras).  The lane group of N columns is the power
# of two in {1, 4, 16, 32, 64} that holds ceil(N / VEC) lanes, VEC = 16 bytes of the dtype.
CASES = {
    "f32_n64": ("f32", "i32", 64, lens(16) + (HUB,), {}),
    "f32_n64_split8": ("f32", "i32", 64, lens(16), dict(split=8)),
    # rows: the forward's and d(e)'s range of A's rows; trows: d(b)'s range of A^T's rows (under
    # split 8 some of its columns, of 6 entries on average, are hubs)
    "f32_n64_rows": ("f32", "i32", 64, lens(16) + (HUB,), dict(split=8, rows=(2, 9), trows=(10, 61))),
    # pad, shift: the leading dimension and base of b, dy, out and db
    "f32_n64_ld": ("f32", "i32", 64, lens(16), dict(pad=1, shift=1)),
    "f32_n16": ("f32", "i32", 16, lens(4), {}),
    "f64_n8_split8": ("f64", "i32", 8, lens(4), dict(split=8)),
    "f32_n128_i64": ("f32", "i64", 128, lens(32) + (HUB,), {}),
    "f32_n1": ("f32", "i32", 1, lens(4), {}),
    "f32_n3": ("f32", "i32", 3, lens(4), {}),
    "f32_n4": ("f32", "i32", 4, lens(1), {}),
    "f32_n5_split8": ("f32", "i32", 5, lens(4), dict(split=8)),
    "f32_n260": ("f32", "i32", 260, lens(64), {}),
    "f32_specials": ("f32", "i32", 4, (6, 2), dict(specials=True)),
    "f64_n64": ("f64", "i32", 64, lens(32), {}),
    "f64_n1": ("f64", "i32", 1, lens(4), {}),
    "f64_n5": ("f64", "i32", 5, lens(4), dict(split=8)),
    # 8 significand bits hold relu's sum over 513 unit products only half of the time: a forced
    # schedule and 130 nonzeros here; bf16's default-schedule hub is compared with the kCPU kernel
    "bf16_n128": ("bf16", "i32", 128, lens(16) + (130,), dict(unit=True, split=8)),
    "bf16_n7": ("bf16", "i32", 7, lens(4), {}),
    "bf16_n8": ("bf16", "i32", 8, lens(1), dict(split=8)),
    "bf16_n520": ("bf16", "i32", 520, lens(64), dict(unit=True)),
    "f16_n64": ("f16", "i32", 64, lens(16) + (HUB,), dict(unit=True)),
    "f16_n5": ("f16", "i32", 5, lens(4), {}),
}


def rounded(x, dt):
    return torch.from_numpy(x).to(DTYPES[dt]).double().numpy()


@functools.lru_cache(maxsize=None)
def problem(name):
    """(rp, ci, e, b, dy) as host tensors of the case's dtypes, and K.  Every row of three or more
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
    e, b, dy = (rng.choice(pool, s) for s in ((rp[-1], n), (K, n), (len(row_lens), n)))
    if kw.get("specials"):  # relu's edges in row 0, one column each; b = 1 there
        b[ci[:6]] = 1.0
        e[:6] = 1.0
        e[0, 0], e[1, 0], e[2, 1], e[3, 2], e[4, 3] = -0.0, 0.0, np.nan, np.inf, -np.inf
    idt = torch.int32 if it == "i32" else torch.int64
    as_t = lambda x: torch.from_numpy(x).to(DTYPES[dt])  # noqa: E731
    return torch.from_numpy(rp).to(idt), torch.from_numpy(ci).to(idt), as_t(e), as_t(b), as_t(dy)


@functools.lru_cache(maxsize=None)
def reference(name, op, act):
    """(out [M, N], de [nnz, N], db [K, N]) in float64 by the contract's steps; computed once."""
    dt = CASES[name][0]
    rp, ci, e, b, dy = (t.double().numpy() if t.is_floating_point() else t.numpy()
                        for t in problem(name))
    out, de, db = np.zeros((len(rp) - 1, e.shape[1])), np.zeros(e.shape), np.zeros(b.shape)
    peak = 0.0  # the largest finite partial sum of out and of db
    for r in range(len(rp) - 1):
        for j in range(rp[r], rp[r + 1]):
            brow = b[ci[j]] if ci[j] < K else np.zeros(e.shape[1])
            with np.errstate(invalid="ignore"):
                t = rounded(brow * e[j] if op == "mul" else brow + e[j], dt)
                live = t > 0 if act == "relu" else np.ones(t.shape, bool)
                out[r] = out[r] + (np.where(t <= 0, 0.0, t) if act == "relu" else t)
                de[j] = np.where(live, rounded(dy[r] * brow, dt) if op == "mul" else dy[r], 0.0)
                if ci[j] < K:
                    g = np.where(live, rounded(dy[r] * e[j], dt) if op == "mul" else dy[r], 0.0)
                    db[ci[j]] = db[ci[j]] + g
                    peak = max(peak, np.abs(db[ci[j]][np.isfinite(db[ci[j]])]).max(initial=0))
            peak = max(peak, np.abs(out[r][np.isfinite(out[r])]).max(initial=0))
    # the bound that makes equality exact: every partial sum of out and of db is a multiple of 1/4
    # below 2^22 (exact in the f32 accumulator) and every result is representable in the dtype
    assert 4 * peak < 2 ** 24
    for x in (out, de, db):
        fin = np.isfinite(x)
        assert np.array_equal(rounded(x, dt)[fin], x[fin]), f"{name}: not exact in {dt}"
    return out, de, db


def same(got, want, what):
    """Bit for bit (the sign of a zero included); a NaN where the reference has one."""
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else got
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions differ"
    bad = np.flatnonzero((got.view(np.int64) != want.view(np.int64)).ravel() & ~nan.ravel())
    assert bad.size == 0, f"{what}: {bad.size} elements differ, first at flat index {bad[0]}: " \
                          f"{got.ravel()[bad[0]]!r} != {want.ravel()[bad[0]]!r}"


def run(dev, name, op, act, num_threads=0):
    """(out, de, db) of the three C-ABI entries on `dev` for a case: its schedule, row range,
    leading dimensions and base shift.  A range of A's rows computes those rows of out and their
    nonzeros of de (from the range's rows of dy); a range of A^T's rows computes those rows of db
    from the range's rows of b and the whole dy."""
    kw = CASES[name][4]
    rp, ci, e, b, dy = (t.to(dev) for t in problem(name))
    m, n = rp.numel() - 1, b.shape[1]
    nt = dict(num_threads=num_threads) if b.device.type == "cpu" else {}
    o = options(split=kw["split"], chunk=kw["split"]) if "split" in kw else None
    lo, hi = kw.get("rows", (0, m))
    tlo, thi = kw.get("trows", (0, K))
    ld = lambda t: padded(t, kw.get("pad", 0), kw.get("shift", 0))  # noqa: E731
    code = (OPS[op], ACTS[act])
    out = ld(torch.zeros((hi - lo, n), dtype=b.dtype, device=b.device))
    ops.spmm_csr_edge(rp, ci, e, ld(b), m, K, *code, out=out, row_begin=lo, row_end=hi, options=o,
                      **nt)
    de = torch.zeros_like(e)
    ops.spmm_csr_edge_grad_e(rp, ci, e, ld(b), ld(dy[lo:hi]), m, K, *code, out=de, row_begin=lo,
                             row_end=hi, **nt)
    rp_t, ci_t, perm = flow_spmm.csr_transpose(rp, ci, K)
    db = ld(torch.zeros((thi - tlo, n), dtype=b.dtype, device=b.device))
    ops.spmm_csr_edge_grad_b(rp_t, ci_t, perm, e, ld(b[tlo:thi]), ld(dy), m, K, *code, out=db,
                             row_begin=tlo, row_end=thi, options=o, **nt)
    return out, de, db


def check_case(dev, name, op, act):
    want_out, want_de, want_db = reference(name, op, act)
    rp = problem(name)[0]
    lo, hi = CASES[name][4].get("rows", (0, rp.numel() - 1))
    out, de, db = run(dev, name, op, act)
    what = f"{name} {op} {act} on {dev}"
    same(out, want_out[lo:hi], f"{what}: out")
    j0, j1 = int(rp[lo]), int(rp[hi])
    same(de[j0:j1], want_de[j0:j1], f"{what}: de")
    assert not bool(de[:j0].any()) and not bool(de[j1:].any()), f"{what}: de outside its rows"
    tlo, thi = CASES[name][4].get("trows", (0, K))
    same(db, want_db[tlo:thi], f"{what}: db")


def random_problem(dt, dev, n=64, seed=5):
    """An order-sensitive problem (normal inputs; rows up to a hub of 600 under split 8 / default)."""
    rng = np.random.default_rng(seed)
    row_lens = (0, 1, 5, 17, 40, 600, 9, 130)
    rp = torch.from_numpy(np.concatenate([[0], np.cumsum(row_lens)]).astype(np.int32))
    ci = torch.from_numpy(rng.integers(0, K + 3, int(rp[-1])).astype(np.int32))
    e, b, dy = (torch.from_numpy(rng.standard_normal(s)).to(DTYPES[dt])
                for s in ((int(rp[-1]), n), (K, n), (len(row_lens), n)))
    return tuple(t.to(dev) for t in (rp, ci, e, b, dy))


def run_random(tensors, op, act, split=0, num_threads=0):
    rp, ci, e, b, dy = tensors
    m = rp.numel() - 1
    nt = dict(num_threads=num_threads) if b.device.type == "cpu" else {}
    o = options(split=split, chunk=split) if split else None
    code = (OPS[op], ACTS[act])
    rp_t, ci_t, perm = flow_spmm.csr_transpose(rp, ci, K)
    return (ops.spmm_csr_edge(rp, ci, e, b, m, K, *code, options=o, **nt),
            ops.spmm_csr_edge_grad_e(rp, ci, e, b, dy, m, K, *code, **nt),
            ops.spmm_csr_edge_grad_b(rp_t, ci_t, perm, e, b, dy, m, K, *code, options=o, **nt))


def bits_equal(a, b, what):
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    assert torch.equal(a.cpu().view(it), b.cpu().view(it)), what


def check_spmm_identity(dev, dt):
    """mul without an activation on e = values expanded over the columns: `spmm`'s bits, on light
    rows and a hub row (default schedule and split 8)."""
    rp, ci, e, b, _ = random_problem(dt, dev)
    m = rp.numel() - 1
    values = e[:, 0].contiguous()
    ee = values[:, None].expand(-1, b.shape[1]).contiguous()
    for split in (0, 8):
        o = options(split=split, chunk=split) if split else None
        run = ops.spmm_csr_cpu if b.device.type == "cpu" else ops.spmm_csr_device
        bits_equal(ops.spmm_csr_edge(rp, ci, ee, b, m, K, 0, 0, options=o),
                   run(rp, ci, values, b, m, K, options=o), f"spmm identity {dt} split={split}")


def check_tmp_sizes(vt, it):
    """The tmp-size queries of the three functional entries (inference and kernel choice; nothing
    is launched, the descriptors carry NULL) on kCPU and device 0: the workspace-size entries'."""
    import ctypes

    from oneflow_spmm import _lib
    from oneflow_spmm._lib import LIB, check
    m, k, nnz, n = 3, 4, 601, 16
    for dev in (-1, 0):
        def d(dtype, *shape):
            t = _lib.TensorDesc()
            t.dtype, t.device, t.ndim, t.data = dtype, dev, len(shape), None
            for i, s in enumerate(shape):
                t.shape[i] = s
                t.stride[i] = shape[1] if i == 0 and len(shape) == 2 else 1
            return ctypes.byref(t)
        e, b, dy = d(vt, nnz, n), d(vt, k, n), d(vt, m, n)
        want, got = [ctypes.c_size_t(5) for _ in range(3)], [ctypes.c_size_t(7) for _ in range(3)]
        check(LIB.ofx_spmm_csr_edge_workspace_size(it, vt, m, k, n, nnz, None,
                                                   ctypes.byref(want[0])), "query")
        check(LIB.ofx_sddmm_csr_heads_workspace_size(it, vt, m, 1, n, nnz, ctypes.byref(want[1])),
              "query")
        check(LIB.ofx_spmm_csr_edge_grad_b_workspace_size(it, vt, m, k, n, nnz, None,
                                                          ctypes.byref(want[2])), "query")
        check(LIB.ofx_functional_spmm_csr_edge(None, d(it, m + 1), d(it, nnz), e, b, m, k, 1, 1,
                                               None, None, 0, ctypes.byref(got[0])), "fwd")
        check(LIB.ofx_functional_spmm_csr_edge_grad_e(None, d(it, m + 1), d(it, nnz), e, b, dy, 1,
                                                      1, None, None, 0, ctypes.byref(got[1])), "de")
        check(LIB.ofx_functional_spmm_csr_edge_grad_b(None, d(it, k + 1), d(it, nnz), d(it, nnz), e,
                                                      b, dy, 1, 1, None, None, 0,
                                                      ctypes.byref(got[2])), "db")
        assert all(w.value > 0 for w in want)
        assert [g.value for g in got] == [w.value if dev == 0 else 0 for w in want], (dev, vt, it)


def check_errors(dev):
    """The documented codes of argument errors at the C-ABI, each followed by a good call."""
    import pytest

    from oneflow_spmm import _lib
    rp, ci, e, b, dy = (t.to(dev) for t in problem("f32_n64"))
    m = rp.numel() - 1
    rp_t, ci_t, perm = flow_spmm.csr_transpose(rp, ci, K)
    good = lambda: same(ops.spmm_csr_edge(rp, ci, e, b, m, K), reference("f32_n64", "mul", None)[0],  # noqa: E731
                        "a good call after an error")
    bad = [(_lib.OFX_EINVAL, lambda: ops.spmm_csr_edge(rp, ci, e, b, m, K, op=2)),
           (_lib.OFX_EINVAL, lambda: ops.spmm_csr_edge(rp, ci, e, b, m, K, act=7)),
           (_lib.OFX_EINVAL, lambda: ops.spmm_csr_edge(rp, ci, e, b, m, K, row_begin=3, row_end=m + 1)),
           (_lib.OFX_EINVAL, lambda: ops.spmm_csr_edge(rp, ci, e, b, m, K, options=options(planned=True))),
           (_lib.OFX_EINVAL, lambda: ops.spmm_csr_edge(rp, ci, e, b, m, K, out=b[:m])),
           (_lib.OFX_EINVAL, lambda: ops.spmm_csr_edge_grad_e(rp, ci, e, b, dy, m, K, out=e)),
           (_lib.OFX_EINVAL, lambda: ops.spmm_csr_edge_grad_b(rp_t, ci_t, perm, e, b, dy, m, K,
                                                              row_end=K + 1)),
           (_lib.OFX_EUNSUPPORTED, lambda: ops.spmm_csr_edge(rp, ci, e.int(), b.int(), m, K))]
    if b.device.type != "cpu":
        bad += [(_lib.OFX_EWORKSPACE, lambda: ops.spmm_csr_edge(rp, ci, e, b, m, K, workspace_bytes=8)),
                (_lib.OFX_EWORKSPACE, lambda: ops.spmm_csr_edge_grad_b(rp_t, ci_t, perm, e, b, dy, m, K,
                                                                       workspace_bytes=8))]
    for code, call in bad:
        with pytest.raises(_lib.OfxError) as err:
            call()
        assert err.value.code == code, str(err.value)
        good()
    with pytest.raises(ValueError, match="op should be"):
        flow_spmm.spmm_edge(rp, ci, e, m, K, b, op="sub")
    with pytest.raises(RuntimeError, match="is expected"):
        flow_spmm.spmm_edge(rp, ci, e[:, :3], m, K, b)
    same(flow_spmm.spmm_edge(rp, ci, e, m, K, b, "add", "relu"),
         reference("f32_n64", "add", "relu")[0], "the public entry")


def check_autograd(dev, monkeypatch):
    """gradcheck in f64 on a 5-row graph for the four pairs (|b op e| >= 0.25: no message at
    relu's kink), [K, H, D] inputs, and only the needed gradient launched."""
    from oneflow_spmm import _C
    rng = np.random.default_rng(3)
    rp = torch.tensor([0, 2, 2, 5, 6, 9], dtype=torch.int32, device=dev)
    ci = torch.tensor([0, 3, 1, 1, 2, 3, 0, 2, 1], dtype=torch.int32, device=dev)
    mag = lambda *s: torch.from_numpy(rng.uniform(1.5, 2.0, s) * rng.choice([-1, 1], s))  # noqa: E731
    e0, b0 = mag(9, 2, 3).to(dev), (mag(4, 2, 3) / 4).to(dev)  # |b| < 0.5 < 1.5 <= |e|
    for op, act in PAIRS:
        e, b = e0.clone().requires_grad_(), b0.clone().requires_grad_()
        fn = lambda e, b: flow_spmm.spmm_edge(rp, ci, e, 5, 4, b, op, act)  # noqa: E731
        assert fn(e, b).shape == (5, 2, 3)
        assert torch.autograd.gradcheck(fn, (e, b), eps=1e-6, atol=1e-7)
    calls = []
    for fname in ("spmm_csr_edge_grad_e", "spmm_csr_edge_grad_b"):
        real = getattr(_C, fname)
        monkeypatch.setattr(_C, fname, lambda *a, _n=fname, _r=real: (calls.append(_n), _r(*a))[1])
    for need_e, need_b in ((True, False), (False, True), (True, True)):
        calls.clear()
        e, b = e0.clone().requires_grad_(need_e), b0.clone().requires_grad_(need_b)
        flow_spmm.spmm_edge(rp, ci, e, 5, 4, b, "add", "relu").sum().backward()
        assert calls == ["spmm_csr_edge_grad_e"] * need_e + ["spmm_csr_edge_grad_b"] * need_b
        assert (e.grad is not None) == need_e and (b.grad is not None) == need_b

"""The checks of the edge softmax, written once for both devices (test_edge_softmax_cpu.py runs
them on host tensors, test_edge_softmax_gpu.py on the GPU, where every result is also compared
with the kCPU kernel's bits).  References: edge_softmax_helpers.py."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import oneflow_spmm as flow_spmm
from edge_softmax_helpers import (G, T, dense_attention, dense_softmax, ref_backward, ref_forward,
                                  run_backward, run_forward)
from helpers import assert_bitwise, from_f32, power_law_degrees, random_csr, to_oracle
from oneflow_spmm import _C
from oneflow_spmm._lib import LIB, check
from reduce_cases import hub_ranges, row_ranges
from reduce_helpers import assert_same, is_sentinel, options

M = 40
SHORT = [0, 1, 7, 8, 9, 63, 64, 65]
# around the widest in-register capacity G and the long-row tile T; 2T+1 and 3T+1 make the tile
# count 3 and 4 (a count that is not a power of two exercises the stack's fold)
LONG = sorted({G - 1, G, G + 1, T - 1, T, T + 1, 2 * T + 1, 3 * T + 1})
# mean degrees that pick each lane-group width of the HIP launch (2 * mean <= 8, 32, 128, beyond)
GROUP_MIXES = {"lg1": [0, 1, 2, 3, 9, 4, 1, 2], "lg4": [7, 8, 9, 1, 33, 16, 0, 12],
               "lg16": SHORT, "lg64": SHORT + LONG,
               # tile counts 6, 8, 8 (a whole number of tiles), 38: the stack past two levels
               "tiles": [5 * T + 1, 7 * T + 3, 8 * T, 37 * T + 5, 3, 64]}


def scores(nnz, dtype, rng, exact):
    if exact:
        x = rng.integers(-6, 7, size=nnz).astype(np.float32)
    else:
        x = rng.uniform(-4, 4, size=nnz).astype(np.float32)
    return from_f32(x, dtype)


def problem(lengths, dtype, idx_dtype=torch.int32, seed=0, exact=False, m=M):
    """(row_ptr, col_idx, e, g): rows of the given lengths (cycled, shuffled), scores and an
    upstream gradient."""
    rng = np.random.default_rng(seed)
    deg = np.array([lengths[i % len(lengths)] for i in range(m)])
    rng.shuffle(deg)
    np_idx = np.int32 if idx_dtype == torch.int32 else np.int64
    rp = np.zeros(m + 1, dtype=np_idx)
    rp[1:] = np.cumsum(deg)
    nnz = int(rp[-1])
    ci = torch.zeros(nnz, dtype=idx_dtype)  # not read by the kernels
    return torch.from_numpy(rp), ci, scores(nnz, dtype, rng, exact), scores(nnz, dtype, rng, exact)


def to_dev(dev, *ts):
    return tuple(t.to(dev) for t in ts)


def check_problem(dev, rp, e, g, *, opts=None, shift=0, what=""):
    """Forward and backward of one problem against the numpy restatement, bit for bit; on the GPU
    also against the kCPU kernel.  Returns (y, de) on `dev`."""
    m = rp.numel() - 1
    d_rp, d_e, d_g = to_dev(dev, rp, e, g)
    y = run_forward(d_rp, d_e, m, opts=opts, shift=shift)
    assert_bitwise(y, ref_forward(rp, e), f"{what} forward")
    de = run_backward(d_rp, y, d_g, m, opts=opts, shift=shift)
    assert_bitwise(de, ref_backward(rp, y.cpu(), g), f"{what} backward")
    if dev != "cpu":
        c_y = run_forward(rp, e, m)
        assert_same(y, c_y, f"{what} forward vs kCPU")
        assert_same(de, run_backward(rp, c_y, g, m), f"{what} backward vs kCPU")
    return y, de


def check_bit_identity(dev, mix, dtype, idx_dtype, exact):
    rp, _, e, g = problem(GROUP_MIXES[mix], dtype, idx_dtype, seed=len(mix) + int(exact),
                          exact=exact)
    check_problem(dev, rp, e, g, what=f"{mix} {dtype} {idx_dtype} exact={exact}")


def check_schedule_and_ranges(dev, dtype):
    """Options and row ranges change no bit; a range writes its own nonzeros only; an unaligned
    base pointer gives the same bits."""
    lengths = SHORT + [G + 1, 2 * T + 1]
    rp, _, e, g = problem(lengths, dtype, seed=11)
    m = rp.numel() - 1
    y, de = check_problem(dev, rp, e, g, what="default")
    d_rp, d_e, d_g = to_dev(dev, rp, e, g)
    for name, o in (("ordered", options(ordered=True)), ("split8", options(split=8, chunk=4))):
        assert_same(run_forward(d_rp, d_e, m, opts=o), y, f"forward {name}")
        assert_same(run_backward(d_rp, y, d_g, m, opts=o), de, f"backward {name}")
    assert_same(run_forward(d_rp, d_e, m, shift=1), y, "forward, base + 1 element")
    assert_same(run_backward(d_rp, y, d_g, m, shift=1), de, "backward, base + 1 element")
    rpn = rp.numpy().astype(np.int64)
    lens = np.diff(rpn)
    for lo, hi in tuple(row_ranges(m)) + tuple(hub_ranges(lens, 8)):
        j0, j1 = int(rpn[lo]), int(rpn[hi])
        for what, part, full in (("forward", run_forward(d_rp, d_e, m, row_begin=lo, row_end=hi), y),
                                 ("backward", run_backward(d_rp, y, d_g, m, row_begin=lo,
                                                           row_end=hi), de)):
            assert_same(part[j0:j1], full[j0:j1], f"{what} rows [{lo}, {hi})")
            kept = is_sentinel(part)
            assert bool(kept[:j0].all()) and bool(kept[j1:].all()), \
                f"{what} rows [{lo}, {hi}): wrote outside [{j0}, {j1})"


def special_problem(dtype):
    inf, nan = np.inf, np.nan
    rows = [[1.0, nan, 2.0],                 # 0: a NaN: the whole row is NaN
            [0.5, inf, 1.0],                 # 1: maximum +inf: NaN
            [-inf, -inf],                    # 2: all -inf: NaN
            [1.0, -inf, 2.0],                # 3: -inf in a finite row: +0 there
            [3.0, 203.0, -100.0],            # 4: 200 apart: beyond the cut-off, +0
            [2.5] * 5,                       # 5: all equal: 1 / deg rounded
            [-7.25],                         # 6: a single element: exactly 1
            [],                              # 7: empty
            [0.0, -0.0, 0.0, -0.0],          # 8: exp_acc(+-0) == 1: each is 1 / 4
            [4.0, 4.0, -200.0, -300.0, -inf, -250.0, -1e30, -120.0, -99.0, -88.0, -100.0],  # 9
            [nan] * 9,                       # 10: NaNs only, two leaves
            [0.0, -800.0]]                   # 11: beyond the f64 cut-off too
    rp = np.zeros(len(rows) + 1, dtype=np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    e = np.array([v for r in rows for v in r], dtype=np.float32)
    return torch.from_numpy(rp), from_f32(e, dtype), rows


def check_special(dev, dtype):
    rp, e, rows = special_problem(dtype)
    m = len(rows)
    rng = np.random.default_rng(3)
    g = scores(e.numel(), dtype, rng, exact=True)
    y, _ = check_problem(dev, rp, e, g, what=f"special {dtype}")
    yf = y.cpu().double().numpy()
    rpn = rp.numpy()
    row = lambda r: yf[rpn[r]:rpn[r + 1]]
    bits = lambda r: to_oracle(y.cpu()[rpn[r]:rpn[r + 1]]).view(np.uint8)
    one = to_oracle(torch.ones(1, dtype=dtype)).view(np.uint8)
    nan_bits = to_oracle(from_f32(np.array([np.nan], dtype=np.float32), dtype)).view(np.uint8)
    for r in (0, 1, 2, 10):  # the canonical NaN in every element
        assert np.array_equal(bits(r), np.tile(nan_bits, len(rows[r]))), f"row {r}: {row(r)}"
    assert row(3)[1] == 0 and not np.signbit(row(3)[1]) and abs(row(3).sum() - 1) < 1e-2
    # 200 apart: beyond the cut-off of the f32 accumulation (-87), so exactly +0; the f64 cut-off
    # is -708 (exp(-200) is a normal double), where row 11 is the case
    if dtype != torch.float64:
        assert row(4)[0] == 0 and row(4)[2] == 0 and row(4)[1] == 1
        assert not np.signbit(row(4)[[0, 2]]).any()
        assert np.array_equal(row(9)[:2], [0.5, 0.5]) and not row(9)[2:].any(), row(9)
    else:
        assert 0 < row(4)[0] < 1e-80 and row(4)[1] == 1
    assert np.array_equal(row(11), [1.0, 0.0]) and not np.signbit(row(11)[1])
    if dtype == torch.float64:
        fifth = np.array([1.0 / 5.0]).view(np.uint8)
    else:  # one division in f32, then the rounding to the storage type
        fifth = to_oracle(from_f32(np.array([np.float32(1) / np.float32(5)]), dtype)).view(np.uint8)
    assert np.array_equal(bits(5), np.tile(fifth, 5)), f"all equal: {row(5)}"
    assert np.array_equal(bits(6), one), f"single element: {row(6)}"
    assert np.array_equal(row(8), [0.25] * 4), f"exp_acc(+-0) == 1 through the sum: {row(8)}"
    # the empty row wrote nothing: its neighbours' entries are adjacent and all compared above


def check_many_rows(dev, dtype=torch.float32):
    """The binned-work-list size: 16 400+ rows, power-law degrees of mean 3, two long rows."""
    m = 16500
    rng = np.random.default_rng(5)
    deg = power_law_degrees(m, 3 * m, 4096, rng)
    deg[123], deg[9000] = 600, 1100
    rp = np.zeros(m + 1, dtype=np.int32)
    rp[1:] = np.cumsum(deg)
    nnz = int(rp[-1])
    rp = torch.from_numpy(rp)
    e, g = scores(nnz, dtype, rng, False), scores(nnz, dtype, rng, False)
    d_rp, d_e, d_g = to_dev(dev, rp, e, g)
    y = run_forward(d_rp, d_e, m)
    c_y = run_forward(rp, e, m)
    assert_same(y, c_y, "many rows forward vs kCPU")
    assert_same(run_backward(d_rp, y, d_g, m), run_backward(rp, c_y, g, m),
                "many rows backward vs kCPU")
    rpn = rp.numpy()
    for r in (123, 9000, 0, m - 1):  # and against numpy on the long rows and the ends
        sub = torch.tensor([0, int(rpn[r + 1] - rpn[r])], dtype=torch.int32)
        assert_bitwise(y[rpn[r]:rpn[r + 1]], ref_forward(sub, e[rpn[r]:rpn[r + 1]]), f"row {r}")


def check_softmax_accuracy(dev):
    """float64 output against torch.softmax per row (atol 1e-5, the tolerance of
    tests/test_backward.py); every row sums to 1 within it."""
    rp, ci, e, _ = problem(SHORT + [G + 1, 2 * T + 1], torch.float64, seed=21)
    d_rp, d_ci, d_e = to_dev(dev, rp, ci, e)
    y = flow_spmm.edge_softmax(d_rp, d_ci, d_e)
    ref = dense_softmax(rp, e)
    torch.testing.assert_close(y.cpu(), ref, rtol=0, atol=1e-5)
    rpn = rp.numpy()
    for r in range(len(rpn) - 1):
        if rpn[r + 1] > rpn[r]:
            assert abs(float(y[rpn[r]:rpn[r + 1]].sum()) - 1.0) <= 1e-5, r


def attention_problem(dtype, seed=2):
    """A 12 x 12 graph with an empty row, and q, k, v of width 5."""
    rng = np.random.default_rng(seed)
    deg = [3, 1, 0, 5, 2, 12, 4, 1, 7, 2, 3, 6]
    rp, ci, _ = random_csr(12, 12, deg, rng, val_dtype=dtype)
    q, k, v = (torch.from_numpy(rng.uniform(-1, 1, size=(12, 5))).to(dtype) for _ in range(3))
    return rp, ci, q, k, v


def attention(rp, ci, q, k, v):
    att = flow_spmm.edge_softmax(rp, ci, flow_spmm.sddmm(rp, ci, q, k))
    return flow_spmm.spmm(rp, ci, att, rp.numel() - 1, k.shape[0], v)


def check_gradcheck(dev):
    rp, ci, e, _ = problem([0, 1, 2, 3, 9, 17], torch.float64, seed=4, m=12)
    d_rp, d_ci = to_dev(dev, rp, ci)
    x = e.to(dev).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: flow_spmm.edge_softmax(d_rp, d_ci, t), (x,))
    rp, ci, q, k, v = attention_problem(torch.float64)
    d_rp, d_ci = to_dev(dev, rp, ci)
    ins = tuple(t.to(dev).requires_grad_(True) for t in (q, k, v))
    assert torch.autograd.gradcheck(lambda a, b, c: attention(d_rp, d_ci, a, b, c), ins)


def check_attention_f32(dev):
    """Gradients of the composed layer in f32 against the float64 dense run (atol 1e-5)."""
    rp, ci, q, k, v = attention_problem(torch.float64)
    w = torch.from_numpy(np.random.default_rng(8).uniform(-1, 1, size=(12, 5)))
    dense = tuple(t.clone().requires_grad_(True) for t in (q, k, v))
    (dense_attention(rp, ci, *dense) * w).sum().backward()
    d_rp, d_ci = to_dev(dev, rp, ci)
    ours = tuple(t.float().to(dev).requires_grad_(True) for t in (q, k, v))
    out = attention(d_rp, d_ci, *ours)
    torch.testing.assert_close(out.detach().cpu().double(), dense_attention(rp, ci, q, k, v),
                               rtol=0, atol=1e-5)
    (out * w.float().to(dev)).sum().backward()
    for name, a, b in zip("qkv", ours, dense):
        torch.testing.assert_close(a.grad.cpu().double(), b.grad, rtol=0, atol=1e-5,
                                   msg=lambda s, n=name: f"d({n}): {s}")


def check_op_layer(dev):
    rp, ci, e, g = problem(SHORT, torch.float32, seed=6)
    d_rp, d_ci, d_e, d_g = to_dev(dev, rp, ci, e, g)
    m = rp.numel() - 1
    y = _C.edge_softmax_csr(d_rp, d_ci, d_e)
    assert_same(y, run_forward(d_rp, d_e, m), "op vs C-ABI")
    assert_same(_C.edge_softmax_csr_grad(d_rp, d_ci, y, d_g), run_backward(d_rp, y, d_g, m),
                "grad op vs C-ABI")
    out = torch.empty_like(d_e)
    assert flow_spmm.edge_softmax(d_rp, d_ci, d_e, out=out) is out
    assert_same(out, y, "out=")
    # shape and dtype errors, from the Python layer and from the op's inference
    with pytest.raises(RuntimeError, match="1-D"):
        _C.edge_softmax_csr(d_rp, d_ci, d_e.view(-1, 1))
    with pytest.raises(RuntimeError, match="nnz"):
        _C.edge_softmax_csr(d_rp, d_ci, d_e[:-1])
    with pytest.raises(TypeError, match="dtype of a_csr_row_ptr"):
        _C.edge_softmax_csr(d_rp, d_ci.long(), d_e)
    with pytest.raises(TypeError):
        _C.edge_softmax_csr(d_rp, d_ci, d_e.to(torch.int32))
    with pytest.raises(TypeError, match="equal to y"):
        _C.edge_softmax_csr_grad(d_rp, d_ci, y, d_g.double())
    # the functional entry itself: tmp size first, then the run; a wrong length is the op's error
    descs = [_C.desc(t) for t in (d_rp, d_ci, d_e)]
    o = torch.empty_like(d_e)
    d_o = _C.desc(o)
    size = ctypes.c_size_t(123)
    args = [ctypes.byref(d) for d in descs] + [ctypes.byref(d_o)]
    check(LIB.ofx_functional_edge_softmax_csr(None, *args, None, 0, ctypes.byref(size)), "tmp")
    assert size.value == 0
    check(LIB.ofx_functional_edge_softmax_csr(_C.current_stream_handle(d_e), *args, None, 0, None),
          "run")
    assert_same(o, y, "functional entry")
    short = _C.desc(d_e[:-1].contiguous())
    rc = LIB.ofx_functional_edge_softmax_csr(None, args[0], args[1], ctypes.byref(short), args[3],
                                             None, 0, ctypes.byref(size))
    assert rc != 0 and b"nnz" in LIB.ofx_last_error()


def check_sbp():
    for op, vals in (("edge_softmax_csr", ("e", "out")), ("edge_softmax_csr_grad",
                                                          ("y", "dy", "dx"))):
        s = _C.sbp_signatures(op)
        sigs, no_grad = s.split("|")
        assert len(sigs.split(";")) == 1, s  # all-broadcast only
        want = {"a_csr_row_ptr:B", "a_csr_col_idx:B"} | {f"{v}:B" for v in vals}
        assert set(sigs.split(",")) == want, s
        assert set(no_grad.split(":")[1].split(",")) == {"a_csr_row_ptr", "a_csr_col_idx"}, s

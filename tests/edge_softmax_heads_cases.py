"""The checks of the multi-head edge softmax (ops "edge_softmax_csr_heads" and its gradient),
written once for both devices (test_edge_softmax_heads_cpu.py runs them on host tensors,
test_edge_softmax_heads_gpu.py on the GPU, where every result is also compared with the kCPU
kernel's bits).  Every comparison is bit for bit.  The reference is the numpy restatement of the
single-head contract (edge_softmax_helpers.ref_forward / ref_backward) applied per column."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import oneflow_spmm as flow_spmm
from edge_softmax_cases import scores
from edge_softmax_helpers import ref_backward, ref_forward
from helpers import assert_bitwise, from_f32
from oneflow_spmm import _C, _lib, autograd
from oneflow_spmm._C import current_stream_handle, dtype_code
from oneflow_spmm._lib import LIB, check
from reduce_helpers import assert_same, is_sentinel, options, sentinel

# every boundary the HIP kernel has: the capacities of LG = 1 / 4 / 16 / 64 (8, 32, 128, 512
# positions), the in-register limit, one full four-tile sweep (2048) and just past it, five tiles
BOUNDARY = [0, 1, 7, 8, 9, 31, 32, 33, 127, 128, 129, 511, 512, 513, 2048, 2049, 2563]
# mean degrees that make the launch choose each lane-group width (2 * mean <= 8, 32, 128; beyond:
# BOUNDARY itself), each with rows that do not fit the group and are taken over by the wave
LG_MIXES = {"lg1": [0, 1, 2, 3, 9, 4, 1, 2], "lg4": [7, 8, 9, 1, 33, 16, 0, 12],
            "lg16": [0, 1, 7, 8, 9, 63, 64, 65, 129, 513, 1, 2, 3, 4, 5, 6, 10, 12]}
HEADS = {"f32": [1, 2, 3, 4, 8, 12, 16], "f64": [1, 2, 3, 4, 8, 12, 16],
         "bf16": [1, 4, 5, 8, 16], "f16": [1, 4, 5, 8, 16]}
HEADS_DT = [(h, dt) for dt, hs in HEADS.items() for h in hs]


def csr_of(lengths, idx_dtype=torch.int32, m=None, seed=0):
    """(row_ptr, col_idx) with rows of the given lengths (cycled up to m rows, shuffled)."""
    m = len(lengths) if m is None else m
    deg = np.array([lengths[i % len(lengths)] for i in range(m)])
    np.random.default_rng(seed).shuffle(deg)
    rp = np.zeros(m + 1, dtype=np.int32 if idx_dtype == torch.int32 else np.int64)
    rp[1:] = np.cumsum(deg)
    return torch.from_numpy(rp), torch.zeros(int(rp[-1]), dtype=idx_dtype)  # col_idx is not read


def problem(lengths, heads, dtype, idx_dtype=torch.int32, m=None, seed=0, exact=False):
    """(row_ptr, col_idx, e [nnz, H], g [nnz, H])."""
    rp, ci = csr_of(lengths, idx_dtype, m, seed)
    rng = np.random.default_rng(seed + 1)
    n = ci.numel() * heads
    e = scores(n, dtype, rng, exact).view(ci.numel(), heads)
    g = scores(n, dtype, rng, exact).view(ci.numel(), heads)
    return rp, ci, e, g


def to_dev(dev, *ts):
    return tuple(t.to(dev) for t in ts)


# ---- C-ABI callers --------------------------------------------------------------------------------
def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def shifted(t: torch.Tensor, shift: int) -> torch.Tensor:
    """A contiguous copy of the [nnz, H] tensor that starts `shift` elements into its buffer."""
    buf = torch.empty(t.numel() + shift, dtype=t.dtype, device=t.device)
    buf[shift:].copy_(t.reshape(-1))
    return buf[shift:].view(t.shape)


def _out(shape, dtype, dev, shift):
    return sentinel((shape[0] * shape[1] + shift,), dtype, dev)[shift:].view(shape)


def _workspace(it, vt, m, heads, nnz, o, dev):
    size = ctypes.c_size_t(0)
    check(LIB.ofx_edge_softmax_csr_heads_workspace_size(it, vt, m, heads, nnz, o,
                                                        ctypes.byref(size)), "heads workspace size")
    return torch.empty(max(size.value, 1), dtype=torch.uint8, device=dev), size.value


def run_forward(rp, e, m, *, row_begin=0, row_end=None, opts=None, shift=0):
    """ofx_edge_softmax_csr_heads(_cpu) on the tensors' device: all [nnz, H] entries of y, those
    outside the rows [row_begin, row_end) still holding sentinel()'s bits.  e and y start `shift`
    elements into their buffers."""
    row_end = m if row_end is None else row_end
    dev, (nnz, heads) = e.device, e.shape
    ee, y = shifted(e, shift), _out(e.shape, e.dtype, dev, shift)
    it, vt = dtype_code(rp.dtype), dtype_code(e.dtype)
    o = ctypes.byref(opts) if opts is not None else None
    if dev.type == "cpu":
        check(LIB.ofx_edge_softmax_csr_heads_cpu(0, it, vt, m, heads, nnz, _ptr(rp), _ptr(ee),
                                                 _ptr(y), row_begin, row_end, o), "heads cpu")
    else:
        ws, size = _workspace(it, vt, m, heads, nnz, o, dev)
        check(LIB.ofx_edge_softmax_csr_heads(current_stream_handle(e), it, vt, m, heads, nnz,
                                             _ptr(rp), _ptr(ee), _ptr(y), row_begin, row_end,
                                             ws.data_ptr(), size, o), "heads")
    return y


def run_backward(rp, y, g, m, *, row_begin=0, row_end=None, opts=None, shift=0):
    """ofx_edge_softmax_csr_heads_grad(_cpu): all [nnz, H] entries of de, as run_forward."""
    row_end = m if row_end is None else row_end
    dev, (nnz, heads) = y.device, y.shape
    yy, gg, de = shifted(y, shift), shifted(g, shift), _out(y.shape, y.dtype, dev, shift)
    it, vt = dtype_code(rp.dtype), dtype_code(y.dtype)
    o = ctypes.byref(opts) if opts is not None else None
    if dev.type == "cpu":
        check(LIB.ofx_edge_softmax_csr_heads_grad_cpu(0, it, vt, m, heads, nnz, _ptr(rp), _ptr(yy),
                                                      _ptr(gg), _ptr(de), row_begin, row_end, o),
              "heads grad cpu")
    else:
        ws, size = _workspace(it, vt, m, heads, nnz, o, dev)
        check(LIB.ofx_edge_softmax_csr_heads_grad(current_stream_handle(y), it, vt, m, heads, nnz,
                                                  _ptr(rp), _ptr(yy), _ptr(gg), _ptr(de),
                                                  row_begin, row_end, ws.data_ptr(), size, o),
              "heads grad")
    return de


# ---- checks ---------------------------------------------------------------------------------------
def check_problem(dev, rp, ci, e, g, *, shift=0, single_head_op=True, what=""):
    """Forward and gradient of one problem: every head's column against the numpy restatement of
    the single-head contract, against the single-head op on the contiguous column, and on the GPU
    against the kCPU heads kernel.  Returns (y, de) on `dev`."""
    m, heads = rp.numel() - 1, e.shape[1]
    d_rp, d_ci, d_e, d_g = to_dev(dev, rp, ci, e, g)
    y = run_forward(d_rp, d_e, m, shift=shift)
    de = run_backward(d_rp, y, d_g, m, shift=shift)
    c_y = y.cpu()
    for h in range(heads):
        assert_bitwise(y[:, h], ref_forward(rp, e[:, h].contiguous()), f"{what} forward head {h}")
        assert_bitwise(de[:, h], ref_backward(rp, c_y[:, h].contiguous(), g[:, h].contiguous()),
                       f"{what} backward head {h}")
        if single_head_op:
            y1 = _C.edge_softmax_csr(d_rp, d_ci, d_e[:, h].contiguous())
            assert_same(y[:, h], y1, f"{what} forward head {h} vs edge_softmax_csr")
            assert_same(de[:, h], _C.edge_softmax_csr_grad(d_rp, d_ci, y1,
                                                           d_g[:, h].contiguous()),
                        f"{what} backward head {h} vs edge_softmax_csr_grad")
    if dev != "cpu":
        k_y = run_forward(rp, e, m)
        assert_same(y, k_y, f"{what} forward vs kCPU")
        assert_same(de, run_backward(rp, k_y, g, m), f"{what} backward vs kCPU")
    return y, de


def check_boundaries(dev, heads, dtype, idx_dtype):
    """One CSR with a row of every boundary length, every head count of both paths."""
    rp, ci, e, g = problem(BOUNDARY, heads, dtype, idx_dtype, seed=heads)
    check_problem(dev, rp, ci, e, g, what=f"boundary H={heads} {dtype} {idx_dtype}")


def check_lane_groups(dev, mix, heads, dtype):
    """CSRs whose mean degree picks LG = 1, 4 and 16 (BOUNDARY picks 64), 40 rows each."""
    lengths = LG_MIXES[mix]
    rp, ci, e, g = problem(lengths, heads, dtype, m=40, seed=len(mix) + heads, exact=True)
    mean2 = 2 * (ci.numel() // 40)
    lo, hi = {"lg1": (0, 8), "lg4": (8, 32), "lg16": (32, 128)}[mix]
    assert lo < mean2 <= hi or (mix == "lg1" and mean2 <= hi), (mix, mean2)
    check_problem(dev, rp, ci, e, g, what=f"{mix} H={heads} {dtype}")


def check_many_tiles(dev, heads, dtype):
    """Rows of 6, 8, 8 (a whole number of tiles) and 38 tiles: the binary-counter stack past its
    first two levels, V values per level."""
    rp, ci, e, g = problem([5 * 512 + 1, 7 * 512 + 3, 8 * 512, 37 * 512 + 5, 3, 64], heads, dtype,
                           seed=13)
    check_problem(dev, rp, ci, e, g, what=f"tiles H={heads} {dtype}")


def check_many_rows(dev, heads, dtype):
    """16,500 rows with power-law degrees of mean 3 and two long rows (more than one block, LG = 1
    with take-overs), against the kCPU kernel."""
    from helpers import power_law_degrees
    m = 16500
    rng = np.random.default_rng(5)
    deg = power_law_degrees(m, 3 * m, 4096, rng)
    deg[123], deg[9000] = 600, 1100
    rp = np.zeros(m + 1, dtype=np.int32)
    rp[1:] = np.cumsum(deg)
    rp = torch.from_numpy(rp)
    n = int(rp[-1]) * heads
    e, g = (scores(n, dtype, rng, False).view(-1, heads) for _ in range(2))
    d_rp, d_e, d_g = to_dev(dev, rp, e, g)
    y, k_y = run_forward(d_rp, d_e, m), run_forward(rp, e, m)
    assert_same(y, k_y, "many rows forward vs kCPU")
    assert_same(run_backward(d_rp, y, d_g, m), run_backward(rp, k_y, g, m),
                "many rows backward vs kCPU")
    rpn = rp.numpy()
    for r in (123, 9000, 0, m - 1):  # and against numpy on the long rows and the ends
        sub = torch.tensor([0, int(rpn[r + 1] - rpn[r])], dtype=torch.int32)
        for h in (0, heads - 1):
            assert_bitwise(y[rpn[r]:rpn[r + 1], h],
                           ref_forward(sub, e[rpn[r]:rpn[r + 1], h].contiguous()),
                           f"row {r} head {h}")


def check_unaligned_and_ranges(dev, heads, dtype):
    """e / y one element into their buffers (the general path) give the aligned bits; a row range
    writes exactly [row_ptr[rb] * H, row_ptr[re] * H), aligned or not; options change no bit."""
    lengths = [0, 1, 7, 8, 9, 33, 64, 65, 129, 513, 1030, 3]
    rp, ci, e, g = problem(lengths, heads, dtype, seed=17)
    m = rp.numel() - 1
    y, de = check_problem(dev, rp, ci, e, g, single_head_op=False, what="aligned")
    d_rp, d_e, d_g = to_dev(dev, rp, e, g)
    assert_same(run_forward(d_rp, d_e, m, shift=1), y, "forward, base + 1 element")
    assert_same(run_backward(d_rp, y, d_g, m, shift=1), de, "backward, base + 1 element")
    for name, o in (("ordered", options(ordered=True)), ("split8", options(split=8, chunk=4)),
                    ("planned", options(planned=True))):
        assert_same(run_forward(d_rp, d_e, m, opts=o), y, f"forward {name}")
        assert_same(run_backward(d_rp, y, d_g, m, opts=o), de, f"backward {name}")
    rpn = rp.numpy().astype(np.int64)
    for lo, hi in ((1, m - 1), (3, 4), (2, 9), (5, 5), (0, 0), (m, m), (0, m)):
        j0, j1 = int(rpn[lo]), int(rpn[hi])
        for shift in (0, 1):
            for what, part, full in (
                    ("forward", run_forward(d_rp, d_e, m, row_begin=lo, row_end=hi, shift=shift), y),
                    ("backward", run_backward(d_rp, y, d_g, m, row_begin=lo, row_end=hi,
                                              shift=shift), de)):
                assert_same(part[j0:j1], full[j0:j1], f"{what} rows [{lo}, {hi}) shift {shift}")
                kept = is_sentinel(part)
                assert bool(kept[:j0].all()) and bool(kept[j1:].all()), \
                    f"{what} rows [{lo}, {hi}) shift {shift}: wrote outside [{j0}, {j1}) * H"


def check_special_confined(dev, dtype):
    """Within one row, head 0 holds a NaN, head 1 +inf, head 2 only -inf, head 3 one -inf among
    finite scores, head 4 scores 200 apart (800 for f64); heads 5..7 are ordinary.  Every head is
    bit-equal to the reference on its column, so no special value leaks into a neighbour."""
    heads, lens = 8, [3, 11, 0, 70, 5]
    rp, ci, e, g = problem(lens, heads, dtype, seed=5)
    apart = 800.0 if dtype == torch.float64 else 200.0
    rpn = rp.numpy()
    ef = e.float() if dtype != torch.float64 else e.clone()
    for r in range(len(lens)):
        j0, j1 = int(rpn[r]), int(rpn[r + 1])
        if j1 == j0:
            continue
        mid = j0 + (j1 - j0) // 2
        ef[mid, 0] = float("nan")
        ef[mid, 1] = float("inf")
        ef[j0:j1, 2] = float("-inf")
        ef[mid, 3] = float("-inf")
        ef[j0:j1, 4] = 3.0
        ef[mid, 4] = 3.0 + apart
    e = ef.to(dtype)
    y, _ = check_problem(dev, rp, ci, e, g, what=f"special {dtype}")
    yc = y.cpu().double()
    for r in range(len(lens)):
        j0, j1 = int(rpn[r]), int(rpn[r + 1])
        if j1 == j0:
            continue
        mid = j0 + (j1 - j0) // 2
        assert bool(torch.isnan(yc[j0:j1, :3]).all()), f"row {r}: heads 0..2 are NaN"
        assert not bool(torch.isnan(yc[j0:j1, 3:]).any()), f"row {r}: a NaN leaked into heads 3.."
        if j1 - j0 > 1:
            assert yc[mid, 3] == 0 and abs(float(yc[j0:j1, 3].sum()) - 1) < 1e-2
            others = torch.cat([yc[j0:mid, 4], yc[mid + 1:j1, 4]])
            assert yc[mid, 4] == 1 and not bool(others.any()), f"row {r}: {apart} apart"
        for h in (5, 6, 7):
            assert abs(float(yc[j0:j1, h].sum()) - 1) < 2e-2, f"row {r} head {h}"


def check_single_head_bits(dev, dtype):
    """H == 1 gives the bits of the single-head entries; H == 0 and nnz == 0 write nothing."""
    rp, ci, e, g = problem(BOUNDARY, 1, dtype, seed=23)
    m = rp.numel() - 1
    d_rp, d_ci, d_e, d_g = to_dev(dev, rp, ci, e, g)
    y = run_forward(d_rp, d_e, m)
    y1 = _C.edge_softmax_csr(d_rp, d_ci, d_e[:, 0].contiguous())
    assert_same(y[:, 0], y1, "H == 1 forward")
    assert_same(run_backward(d_rp, y, d_g, m)[:, 0],
                _C.edge_softmax_csr_grad(d_rp, d_ci, y1, d_g[:, 0].contiguous()), "H == 1 backward")
    empty = torch.empty((ci.numel(), 0), dtype=dtype, device=dev)
    assert run_forward(d_rp, empty, m).shape == (ci.numel(), 0)
    assert run_backward(d_rp, empty, empty, m).shape == (ci.numel(), 0)
    rp0 = torch.zeros(4, dtype=torch.int32, device=dev)
    none = torch.empty((0, 4), dtype=dtype, device=dev)
    assert run_forward(rp0, none, 3).shape == (0, 4)
    assert tuple(flow_spmm.edge_softmax(rp0, rp0[:0], none).shape) == (0, 4)
    assert tuple(flow_spmm.edge_softmax(d_rp, d_ci, empty).shape) == (ci.numel(), 0)


def check_public_api(dev, monkeypatch):
    """edge_softmax on e [nnz, H] equals the per-head composition bit for bit, forward and
    e.grad; out= is written directly without autograd and refused with it; non-contiguous inputs
    are accepted; the single-head op is not called."""
    rp, ci, e, g = problem([0, 1, 7, 9, 33, 65, 129, 600], 3, torch.float32, seed=31)
    d_rp, d_ci, d_e, d_g = to_dev(dev, rp, ci, e, g)
    a = d_e.clone().requires_grad_(True)
    b = d_e.clone().requires_grad_(True)
    want = autograd._edge_softmax_heads_composed(d_rp, d_ci, b)
    (want * d_g).sum().backward()
    calls = []
    real = (_C.edge_softmax_csr_heads, _C.edge_softmax_csr_heads_grad)

    def refuse(*_a, **_k):
        raise AssertionError("the 2-D edge_softmax called the single-head op")

    monkeypatch.setattr(_C, "edge_softmax_csr", refuse)
    monkeypatch.setattr(_C, "edge_softmax_csr_grad", refuse)
    monkeypatch.setattr(_C, "edge_softmax_csr_heads",
                        lambda *x, **k: (calls.append("fwd"), real[0](*x, **k))[1])
    monkeypatch.setattr(_C, "edge_softmax_csr_heads_grad",
                        lambda *x, **k: (calls.append("bwd"), real[1](*x, **k))[1])
    got = flow_spmm.edge_softmax(d_rp, d_ci, a)
    (got * d_g).sum().backward()
    assert calls == ["fwd", "bwd"], calls  # one launch each way
    assert_same(got.detach(), want.detach(), "forward vs composition")
    assert_same(a.grad, b.grad, "e.grad vs composition")
    out = sentinel(tuple(d_e.shape), d_e.dtype, dev)
    assert flow_spmm.edge_softmax(d_rp, d_ci, d_e, out=out) is out
    assert_same(out, want.detach(), "out=")
    with pytest.raises(RuntimeError, match="out="):
        flow_spmm.edge_softmax(d_rp, d_ci, a, out=out)
    with pytest.raises(RuntimeError, match="out must be"):
        flow_spmm.edge_softmax(d_rp, d_ci, d_e, out=torch.empty_like(d_e).t().contiguous().t())
    # a non-contiguous e (a column slice of a wider tensor) and a non-contiguous upstream gradient
    wide = torch.zeros((d_e.shape[0], 5), dtype=d_e.dtype, device=dev)
    wide[:, 1:4] = d_e
    c = wide[:, 1:4].detach().requires_grad_(True)
    y = flow_spmm.edge_softmax(d_rp, d_ci, c)
    assert_same(y.detach(), want.detach(), "non-contiguous e")
    gw = torch.zeros_like(wide)
    gw[:, 1:4] = d_g
    y.backward(gw[:, 1:4])
    assert_same(c.grad, b.grad, "non-contiguous upstream gradient")


def check_op_layer(dev):
    """Both ops through the registry dispatch: against the C-ABI, the functional entry's two
    phases, and the refusals of the Python layer and of the op's shape / dtype inference."""
    rp, ci, e, g = problem([0, 1, 7, 8, 9, 63, 64, 65], 4, torch.float32, m=24, seed=6)
    d_rp, d_ci, d_e, d_g = to_dev(dev, rp, ci, e, g)
    m = rp.numel() - 1
    y = _C.edge_softmax_csr_heads(d_rp, d_ci, d_e)
    assert y.shape == d_e.shape and y.dtype == d_e.dtype
    assert_same(y, run_forward(d_rp, d_e, m), "op vs C-ABI")
    assert_same(_C.edge_softmax_csr_heads_grad(d_rp, d_ci, y, d_g), run_backward(d_rp, y, d_g, m),
                "grad op vs C-ABI")
    for dt, it in ((torch.float64, torch.int64), (torch.bfloat16, torch.int32),
                   (torch.float16, torch.int64)):
        r2, c2, e2, g2 = problem([3, 0, 9, 40], 5, dt, it, seed=8)
        x_rp, x_ci, x_e, x_g = to_dev(dev, r2, c2, e2, g2)
        y2 = _C.edge_softmax_csr_heads(x_rp, x_ci, x_e)
        assert_same(y2, run_forward(x_rp, x_e, 4), f"op vs C-ABI {dt} {it}")
        assert_same(_C.edge_softmax_csr_heads_grad(x_rp, x_ci, y2, x_g),
                    run_backward(x_rp, y2, x_g, 4), f"grad op vs C-ABI {dt} {it}")
    with pytest.raises(RuntimeError, match="2-D"):
        _C.edge_softmax_csr_heads(d_rp, d_ci, d_e[:, 0].contiguous())
    with pytest.raises(RuntimeError, match="nnz"):
        _C.edge_softmax_csr_heads(d_rp, d_ci, d_e[:-1])
    with pytest.raises(RuntimeError, match="number of heads"):
        _C.edge_softmax_csr_heads_grad(d_rp, d_ci, y, d_g[:, :3])
    with pytest.raises(TypeError, match="dtype of a_csr_row_ptr"):
        _C.edge_softmax_csr_heads(d_rp, d_ci.long(), d_e)
    with pytest.raises(TypeError):
        _C.edge_softmax_csr_heads(d_rp, d_ci, d_e.to(torch.int32))
    with pytest.raises(TypeError, match="equal to y"):
        _C.edge_softmax_csr_heads_grad(d_rp, d_ci, y, d_g.double())
    # the functional entries themselves: tmp size first, then the run; the op's own inference
    # refuses a 1-D e and a dy with another number of heads
    o = torch.empty_like(d_e)
    byref = lambda *ts: [ctypes.byref(_C.desc(t)) for t in ts]
    args = byref(d_rp, d_ci, d_e, o)
    size = ctypes.c_size_t(123)
    check(LIB.ofx_functional_edge_softmax_csr_heads(None, *args, None, 0, ctypes.byref(size)),
          "tmp")
    assert size.value == 0
    check(LIB.ofx_functional_edge_softmax_csr_heads(current_stream_handle(d_e), *args, None, 0,
                                                    None), "run")
    assert_same(o, y, "functional entry")
    dx = torch.empty_like(d_e)
    check(LIB.ofx_functional_edge_softmax_csr_heads_grad(
        current_stream_handle(d_e), *byref(d_rp, d_ci, y, d_g, dx), None, 0, None), "run grad")
    assert_same(dx, run_backward(d_rp, y, d_g, m), "functional grad entry")
    flat = d_e[:, 0].contiguous()
    rc = LIB.ofx_functional_edge_softmax_csr_heads(None, *byref(d_rp, d_ci, flat, o), None, 0,
                                                   ctypes.byref(size))
    assert rc != 0 and b"2-D" in LIB.ofx_last_error()
    rc = LIB.ofx_functional_edge_softmax_csr_heads_grad(
        None, *byref(d_rp, d_ci, y, d_g[:, :3].contiguous(), dx), None, 0, ctypes.byref(size))
    assert rc != 0 and b"heads" in LIB.ofx_last_error()
    rc = LIB.ofx_functional_edge_softmax_csr_heads_grad(
        None, *byref(d_rp, d_ci, y, d_g[:-1].contiguous(), dx), None, 0, ctypes.byref(size))
    assert rc != 0 and b"nnz" in LIB.ofx_last_error()


def check_sbp():
    for op, vals in (("edge_softmax_csr_heads", ("e", "out")),
                     ("edge_softmax_csr_heads_grad", ("y", "dy", "dx"))):
        s = _C.sbp_signatures(op)
        sigs, no_grad = s.split("|")
        assert len(sigs.split(";")) == 1, s  # all-broadcast only
        want = {"a_csr_row_ptr:B", "a_csr_col_idx:B"} | {f"{v}:B" for v in vals}
        assert set(sigs.split(",")) == want, s
        assert set(no_grad.split(":")[1].split(",")) == {"a_csr_row_ptr", "a_csr_col_idx"}, s


def check_argument_checks(dev):
    """A negative heads, a NULL pointer, a bad row range and a bad dtype return the documented
    code, and nothing is launched: the output keeps its sentinel."""
    rp = torch.tensor([0, 2, 3], dtype=torch.int32, device=dev)
    e = torch.tensor([[1.0, 2.0], [2.0, 0.0], [3.0, 1.0]], device=dev)
    y = sentinel((3, 2), torch.float32, dev)
    de = sentinel((3, 2), torch.float32, dev)
    I, F = _lib.DT_INT32, _lib.DT_FLOAT
    if dev == "cpu":
        fwd = lambda *a: LIB.ofx_edge_softmax_csr_heads_cpu(0, *a, None)
        bwd = lambda *a: LIB.ofx_edge_softmax_csr_heads_grad_cpu(0, *a, None)
    else:
        s = current_stream_handle(e)
        fwd = lambda *a: LIB.ofx_edge_softmax_csr_heads(s, *a, None, 0, None)
        bwd = lambda *a: LIB.ofx_edge_softmax_csr_heads_grad(s, *a, None, 0, None)
    p = (rp.data_ptr(), e.data_ptr(), y.data_ptr())
    q = (rp.data_ptr(), e.data_ptr(), e.data_ptr(), de.data_ptr())
    for call, ptrs in ((fwd, p), (bwd, q)):
        assert call(I, F, 2, -1, 3, *ptrs, 0, 2) == _lib.OFX_EINVAL            # negative heads
        assert call(I, F, 2, 2, -3, *ptrs, 0, 2) == _lib.OFX_EINVAL            # negative nnz
        assert call(I, F, 2, 2, 3, *ptrs, 1, 3) == _lib.OFX_EINVAL             # row range
        assert call(I, F, 2, 2, 3, *ptrs, 2, 1) == _lib.OFX_EINVAL
        assert call(I, F, 2, 2, 3, ptrs[0], None, *ptrs[2:], 0, 2) == _lib.OFX_EINVAL  # NULL
        assert call(I, F, 2, 2, 3, *ptrs[:-1], None, 0, 2) == _lib.OFX_EINVAL
        assert call(I, _lib.DT_INT64, 2, 2, 3, *ptrs, 0, 2) == _lib.OFX_EUNSUPPORTED
        assert call(F, F, 2, 2, 3, *ptrs, 0, 2) == _lib.OFX_EUNSUPPORTED
        assert call(I, F, 2, 2, 1 << 31, *ptrs, 0, 2) == _lib.OFX_EINVAL       # int32 and nnz
        assert call(I, F, 2, 0, 3, *ptrs, 0, 2) == _lib.OFX_OK                 # H == 0: nothing
    size = ctypes.c_size_t(7)
    assert LIB.ofx_edge_softmax_csr_heads_workspace_size(I, F, 2, 2, 3, None,
                                                         ctypes.byref(size)) == _lib.OFX_OK
    assert size.value == 0
    assert LIB.ofx_edge_softmax_csr_heads_workspace_size(I, F, 2, 2, 3, None,
                                                         None) == _lib.OFX_EINVAL
    assert LIB.ofx_edge_softmax_csr_heads_workspace_size(I, F, 2, -2, 3, None,
                                                         ctypes.byref(size)) == _lib.OFX_EINVAL
    bad = _lib.Options()
    bad.magic = 0
    if dev == "cpu":
        assert LIB.ofx_edge_softmax_csr_heads_cpu(0, I, F, 2, 2, 3, *p, 0, 2,
                                                  ctypes.byref(bad)) == _lib.OFX_EINVAL
    else:
        s = current_stream_handle(e)
        assert LIB.ofx_edge_softmax_csr_heads(s, I, F, 2, 2, 3, *p, 0, 2, None, 0,
                                              ctypes.byref(bad)) == _lib.OFX_EINVAL
        # a NULL workspace with a non-zero size
        assert LIB.ofx_edge_softmax_csr_heads(s, I, F, 2, 2, 3, *p, 0, 2, None, 16,
                                              None) == _lib.OFX_EWORKSPACE
        assert LIB.ofx_edge_softmax_csr_heads_grad(s, I, F, 2, 2, 3, *q, 0, 2, None, 16,
                                                   None) == _lib.OFX_EWORKSPACE
        torch.cuda.synchronize()
    assert bool(is_sentinel(y).all()) and bool(is_sentinel(de).all())
    assert fwd(I, F, 2, 2, 3, *p, 0, 2) == _lib.OFX_OK
    assert not bool(is_sentinel(y).any())


def check_threads_do_not_matter():
    """The kCPU result does not depend on num_threads."""
    rp, _, e, g = problem(BOUNDARY, 5, torch.float32, m=60, seed=9)
    m, (nnz, heads) = rp.numel() - 1, e.shape
    I, F = dtype_code(rp.dtype), dtype_code(e.dtype)
    outs = []
    for threads in (1, 3, 8):
        y, de = torch.empty_like(e), torch.empty_like(e)
        check(LIB.ofx_edge_softmax_csr_heads_cpu(threads, I, F, m, heads, nnz, rp.data_ptr(),
                                                 e.data_ptr(), y.data_ptr(), 0, m, None), "fwd")
        check(LIB.ofx_edge_softmax_csr_heads_grad_cpu(threads, I, F, m, heads, nnz, rp.data_ptr(),
                                                      y.data_ptr(), g.data_ptr(), de.data_ptr(),
                                                      0, m, None), "bwd")
        outs.append((y, de))
    for y, de in outs[1:]:
        assert_same(y, outs[0][0], "forward across thread counts")
        assert_same(de, outs[0][1], "backward across thread counts")

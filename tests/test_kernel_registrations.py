"""CPU: the kernel registrations of every CSR op, through the tmp-size query of its functional
entry.  A query runs the op's inference and the kernel choice and launches nothing, so it needs
no GPU and no data (the descriptors carry NULL).  OFX_OK means exactly one kernel matched the
(device, value dtype, index dtype) of the call; on device 0 the bytes are those of the op's own
ofx_*_workspace_size for the same shapes, i.e. the kernel was registered with its tmp-size function.

Shapes: m = 2 rows (row_ptr [0, 600, 601]: 3 elements), k = 4, nnz = 601; N = 8 single-head (a
600-long row is past the hub split of 512: the planned-item ops -- max / min, their gradients, the
SDDMMs, the multi-head SpMM, the attention, the transpose -- need a workspace; the sum op takes its
one-kernel form at this size and the edge softmaxes never need one, so theirs is 0 on both
sides), H = 2 heads of D = 4."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "of-spmm_amd"))

from oneflow_spmm import _lib  # noqa: E402
from oneflow_spmm._lib import LIB, TensorDesc  # noqa: E402

M, K, NNZ, N, H, D = 2, 4, 601, 8, 2, 4
VALUE_DTYPES = {"f32": _lib.DT_FLOAT, "f64": _lib.DT_DOUBLE, "f16": _lib.DT_FLOAT16,
                "bf16": _lib.DT_BFLOAT16}
INDEX_DTYPES = {"i32": _lib.DT_INT32, "i64": _lib.DT_INT64}


def _queries(dev, vt, it):
    """{entry: (tmp-size query, workspace query)}, each taking a byref(size_t)."""
    def d(dtype, *shape):
        t = TensorDesc()
        t.dtype, t.device, t.ndim, t.data = dtype, dev, len(shape), None
        for i, s in enumerate(shape):
            t.shape[i] = s
            t.stride[i] = shape[1] if i == 0 and len(shape) == 2 else 1
        return ctypes.byref(t)

    rp, ci, rp_t = d(it, M + 1), d(it, NNZ), d(it, K + 1)
    v, perm = d(vt, NNZ), d(it, NNZ)
    a, b, out = d(vt, M, N), d(vt, K, N), d(vt, M, N)
    arg, dy = d(it, M, N), d(vt, M, N)
    e1, e2, vh = d(vt, NNZ), d(vt, NNZ, H), d(vt, NNZ, H)
    hier, axes = (ctypes.c_int64 * 1)(1), (ctypes.c_int32 * 1)(-1)
    spmm_ws = lambda s: LIB.ofx_spmm_csr_workspace_size(it, vt, M, K, N, NNZ, None, s)  # noqa: E731
    sddmm_ws = lambda s: LIB.ofx_sddmm_csr_workspace_size(it, vt, M, N, NNZ, s)  # noqa: E731
    softmax_ws = lambda s: LIB.ofx_edge_softmax_csr_workspace_size(it, vt, M, NNZ, None, s)  # noqa: E731
    softmax_heads_ws = lambda s: LIB.ofx_edge_softmax_csr_heads_workspace_size(  # noqa: E731
        it, vt, M, H, NNZ, None, s)
    q = {
        "spmm_csr_tmp_size": (
            lambda s: LIB.ofx_functional_spmm_csr_tmp_size(rp, ci, v, M, K, b, s), spmm_ws),
        "spmm_csr_global": (
            lambda s: LIB.ofx_functional_spmm_csr_global(None, rp, ci, v, M, K, b, -1, None, None,
                                                         0, 1, hier, axes, 0, 0, s), spmm_ws),
        "spmm_csr_global_attrs": (
            lambda s: LIB.ofx_functional_spmm_csr_global_attrs(
                None, rp, ci, v, M, K, b, -1, None, None, 0, 1, hier, axes, 0, 0, s, None), spmm_ws),
        "fused_spmm_csr": (
            lambda s: LIB.ofx_functional_fused_spmm_csr(None, rp, ci, v, b, None, M, K, 1, None,
                                                        None, 0, s), spmm_ws),
        "spmm_csr_gathered": (
            lambda s: LIB.ofx_functional_spmm_csr_gathered(None, rp, ci, v, perm, b, M, K, None,
                                                           None, 0, s), spmm_ws),
        "sddmm_csr": (
            lambda s: LIB.ofx_functional_sddmm_csr(None, rp, ci, a, b, M, K, None, None, 0, s),
            sddmm_ws),
        "csr_transpose": (
            lambda s: LIB.ofx_functional_csr_transpose(None, rp, ci, M, K, None, None, None, None,
                                                       0, s),
            lambda s: LIB.ofx_csr_transpose_workspace_size(it, M, K, NNZ, s)),
        "spmm_csr_reduce_grad_b": (
            lambda s: LIB.ofx_functional_spmm_csr_reduce_grad_b(None, rp_t, ci, perm, v, arg, dy, M,
                                                                K, None, None, 0, s),
            lambda s: LIB.ofx_spmm_csr_select_workspace_size(it, vt, M, K, N, NNZ, None, s)),
        "spmm_csr_reduce_grad_values": (
            lambda s: LIB.ofx_functional_spmm_csr_reduce_grad_values(None, rp, ci, arg, dy, b, M, K,
                                                                     None, None, 0, s), sddmm_ws),
        "edge_softmax_csr": (
            lambda s: LIB.ofx_functional_edge_softmax_csr(None, rp, ci, e1, None, None, 0, s),
            softmax_ws),
        "edge_softmax_csr_grad": (
            lambda s: LIB.ofx_functional_edge_softmax_csr_grad(None, rp, ci, e1, e1, None, None, 0,
                                                               s), softmax_ws),
        "spmm_csr_heads": (
            lambda s: LIB.ofx_functional_spmm_csr_heads(None, rp, ci, vh, b, M, K, None, None, 0, s),
            lambda s: LIB.ofx_spmm_csr_heads_workspace_size(it, vt, M, K, H, D, NNZ, None, s)),
        "sddmm_csr_heads": (
            lambda s: LIB.ofx_functional_sddmm_csr_heads(None, rp, ci, a, b, H, None, None, 0, s),
            lambda s: LIB.ofx_sddmm_csr_heads_workspace_size(it, vt, M, H, D, NNZ, s)),
        "edge_softmax_csr_heads": (
            lambda s: LIB.ofx_functional_edge_softmax_csr_heads(None, rp, ci, e2, None, None, 0, s),
            softmax_heads_ws),
        "edge_softmax_csr_heads_grad": (
            lambda s: LIB.ofx_functional_edge_softmax_csr_heads_grad(None, rp, ci, e2, e2, None,
                                                                     None, 0, s), softmax_heads_ws),
        "graph_attention_csr_heads": (
            lambda s: LIB.ofx_functional_graph_attention_csr_heads(None, rp, ci, a, b, b, H, None,
                                                                   None, None, 0, s),
            lambda s: LIB.ofx_graph_attention_csr_heads_workspace_size(it, vt, M, K, H, D, NNZ,
                                                                       None, s)),
    }
    for name, code in _C_REDUCE.items():
        q[f"spmm_csr_reduce[{name}]"] = (
            lambda s, code=code: LIB.ofx_functional_spmm_csr_reduce(
                None, rp, ci, v, M, K, b, code, None, None, None, 0, 0, 1, -1, -1, 0, s),
            lambda s, code=code: LIB.ofx_spmm_csr_reduce_workspace_size(it, vt, M, K, N, NNZ, code,
                                                                        None, s))
    return q


_C_REDUCE = {"sum": _lib.REDUCE_SUM, "mean": _lib.REDUCE_MEAN, "max": _lib.REDUCE_MAX,
             "min": _lib.REDUCE_MIN}
ENTRIES = sorted(_queries(-1, _lib.DT_FLOAT, _lib.DT_INT32))


@pytest.mark.parametrize("dev", [-1, 0], ids=["cpu", "hip0"])
@pytest.mark.parametrize("it", sorted(INDEX_DTYPES))
@pytest.mark.parametrize("vt", sorted(VALUE_DTYPES))
@pytest.mark.parametrize("entry", ENTRIES)
def test_one_kernel_matches_with_its_tmp_size(entry, vt, it, dev):
    tmp_size, workspace = _queries(dev, VALUE_DTYPES[vt], INDEX_DTYPES[it])[entry]
    got = ctypes.c_size_t(1 << 40)
    assert tmp_size(ctypes.byref(got)) == _lib.OFX_OK, LIB.ofx_last_error()
    if dev < 0:
        return
    want = ctypes.c_size_t(0)
    assert workspace(ctypes.byref(want)) == _lib.OFX_OK, LIB.ofx_last_error()
    assert got.value == want.value

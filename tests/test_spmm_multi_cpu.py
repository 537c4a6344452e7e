"""CPU: the multi-aggregator SpMM (`spmm_multi`, op "spmm_csr_multi") through its kCPU kernel
(csrc/spmm_multi_cpu.cpp): the case table of spmm_multi_cases.py against the float64 reference, the
contract's var / std bits and bound and the existing ops' bits; the gradients against torch autograd
on a dense restatement; the public layout; the op layer's registrations and the argument errors."""
from __future__ import annotations

import ctypes

import pytest
import torch

import oneflow_spmm as flow_spmm
import spmm_multi_cases as mc
from oneflow_spmm import _C, _lib, ops
from oneflow_spmm._lib import LIB, TensorDesc


@pytest.mark.parametrize("name", mc.CASES)
def test_case_table(name):
    mc.check_case(torch.device("cpu"), name)


@pytest.mark.parametrize("aggrs", [mc.AGGRS, ("std", "max"), ("mean",)])
def test_gradients_match_torch_autograd(aggrs):
    mc.check_gradients(torch.device("cpu"), aggrs)


def test_public_layout_and_thread_count():
    """out[:, a, :] is aggrs[a] in the caller's order; b [K, H, D] is N = H*D; the bits do not
    depend on the thread count."""
    rp, ci, vals, b = mc.problem("f32_n64_split8")
    m = rp.numel() - 1
    stored = mc.run("cpu", "f32_n64_split8", num_threads=3)[0]
    mc.bits_equal(stored, mc.run("cpu", "f32_n64_split8", num_threads=1)[0], "threads")
    aggrs = ("std", "max", "sum")
    out = flow_spmm.spmm_multi(rp, ci, vals, m, mc.K, b.view(mc.K, 4, 16), aggrs, mc.EPS)
    assert out.shape == (m, 3, 64)
    for i, a in enumerate(aggrs):  # the public call runs the default schedule: rows up to 17 alike
        mc.bits_equal(out[:, i, :], stored[:, mc.AGGRS.index(a), :], a)


@pytest.mark.parametrize("dev", [-1, 0])
@pytest.mark.parametrize("it", [_lib.DT_INT32, _lib.DT_INT64])
@pytest.mark.parametrize("vt", [_lib.DT_FLOAT, _lib.DT_DOUBLE, _lib.DT_FLOAT16, _lib.DT_BFLOAT16])
def test_one_kernel_per_device_and_dtypes(dev, vt, it):
    """The tmp-size query runs inference and the kernel choice and launches nothing: exactly one
    kernel matches, registered on the device with ofx_spmm_csr_multi_workspace_size (m = 2 rows of
    600 and 1 nonzeros: past the hub split, so the size is not 0)."""
    def d(dtype, *shape):
        t = TensorDesc()
        t.dtype, t.device, t.ndim, t.data = dtype, dev, len(shape), None
        for i, s in enumerate(shape):
            t.shape[i] = s
            t.stride[i] = shape[1] if i == 0 and len(shape) == 2 else 1
        return ctypes.byref(t)

    m, k, nnz, n, mask = 2, 4, 601, 8, 63
    got, want = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _lib.check(LIB.ofx_functional_spmm_csr_multi(None, d(it, m + 1), d(it, nnz), d(vt, nnz), m, k,
                                                 d(vt, k, n), mask, 1e-5, None, None, None, None,
                                                 0, ctypes.byref(got)))
    _lib.check(LIB.ofx_spmm_csr_multi_workspace_size(it, vt, m, k, n, nnz, mask, None,
                                                     ctypes.byref(want)))
    assert want.value > 0 and got.value == (want.value if dev == 0 else 0)


def test_argument_errors():
    rp, ci, vals, b = mc.problem("f32_n16")
    m = rp.numel() - 1
    for bad in ((), ("mean", "mean"), ("median",), "avg"):
        with pytest.raises(ValueError, match="aggrs"):
            flow_spmm.spmm_multi(rp, ci, vals, m, mc.K, b, bad)
    with pytest.raises(ValueError, match="eps"):
        flow_spmm.spmm_multi(rp, ci, vals, m, mc.K, b, eps=-1.0)
    for mask in (0, 64):
        with pytest.raises(flow_spmm.OfxError, match="aggr_mask"):
            ops.spmm_csr_multi(rp, ci, vals, b, m, mc.K, mask)
    with pytest.raises(flow_spmm.OfxError, match="arg_max"):  # an arg without its aggregator
        ops.spmm_csr_multi(rp, ci, vals, b, m, mc.K, _C.AGGR_BITS["sum"],
                           arg_max=torch.empty((m, 16), dtype=rp.dtype))
    with pytest.raises(TypeError):
        flow_spmm.spmm_multi(rp, ci, vals.double(), m, mc.K, b)

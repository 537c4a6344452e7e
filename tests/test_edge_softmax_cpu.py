"""Edge softmax over CSR rows (op "edge_softmax_csr" and its gradient) on host tensors: the kCPU
kernels against the numpy restatement of the contract bit for bit, the accuracy of exp_acc, the
op layer, autograd, and the kCPU kernels under the host sanitizers (edge_softmax_cases.py)."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest
import torch

import edge_softmax_cases as ec
from edge_softmax_helpers import exp_acc, run_forward
from helpers import DTYPES
from oneflow_spmm import _lib
from oneflow_spmm._lib import LIB
from sanitize_helpers import CLANG, build_and_run


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("it", [torch.int32, torch.int64])
@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
@pytest.mark.parametrize("mix", ["lg16", "lg64"])
def test_bit_identity(mix, dt, it, exact):
    ec.check_bit_identity("cpu", mix, DTYPES[dt], it, exact)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_schedule_and_ranges(dt):
    ec.check_schedule_and_ranges("cpu", DTYPES[dt])


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_special_values(dt):
    ec.check_special("cpu", DTYPES[dt])


def test_exp_acc_f32_accuracy():
    """exp_acc in f32 against float64 exp on every 37th float32 bit pattern of [-87, 0]: the
    maximum error is 0.96 ulp at the two digits the figure is stated with (0.9623 on this sample;
    the exhaustive maximum is in DESIGN.md §3e), no subnormal result, exp_acc(+-0) == 1."""
    lo = np.array([-87.0], dtype=np.float32).view(np.uint32)[0]
    neg_zero = np.array([-0.0], dtype=np.float32).view(np.uint32)[0]
    t = np.arange(neg_zero, lo + 1, 37, dtype=np.uint32).view(np.float32)
    got = exp_acc(t)
    want = np.exp(t.astype(np.float64))
    ulp = np.spacing(want.astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want) / ulp
    print(f"exp_acc f32: max error {err.max():.4f} ulp over {len(t)} points")
    assert round(float(err.max()), 2) <= 0.96
    assert (got >= np.finfo(np.float32).tiny).all()
    one = exp_acc(np.array([0.0, -0.0], dtype=np.float32))
    assert np.array_equal(one.view(np.uint32), np.array([1.0, 1.0], dtype=np.float32).view(np.uint32))
    assert exp_acc(np.array([-87.5, -np.inf], dtype=np.float32)).view(np.uint32).tolist() == [0, 0]
    assert np.isnan(exp_acc(np.array([np.nan], dtype=np.float32)))[0]


def test_exp_acc_f64_accuracy():
    """exp_acc in f64 against long-double exp on a sample of [-708, 0]: within 2 ulp.  The bound
    is the Cephes rational form's published peak relative error, 2.0e-16, in units of the smallest
    relative ulp of a double, 2^-53 = 1.11e-16 (1.8, rounded up); the maximum measured on 10^7
    points is in DESIGN.md §3e.  No subnormal result."""
    if np.finfo(np.longdouble).nmant <= 52:
        pytest.skip("no extended-precision long double on this host")
    rng = np.random.default_rng(0)
    t = np.concatenate([-rng.uniform(0, 708, size=200000), -np.logspace(-300, 2.85, 20000),
                        np.array([-708.0, -0.0, 0.0])])
    got = exp_acc(t)
    want = np.exp(t.astype(np.longdouble))
    err = np.abs(got.astype(np.longdouble) - want) / np.spacing(want.astype(np.float64))
    print(f"exp_acc f64: max error {float(err.max()):.4f} ulp over {len(t)} points")
    assert float(err.max()) <= 2.0
    assert (got >= np.finfo(np.float64).tiny).all()
    assert exp_acc(np.array([-708.5, -np.inf])).view(np.uint64).tolist() == [0, 0]


def test_exp_acc_through_the_kernel():
    """The kCPU kernel's exponential is the restatement's: rows (0, t) give y[1] / y[0] = exp_acc(t)
    exactly wherever the sum 1 + exp_acc(t) rounds to 1."""
    t = -np.linspace(20.0, 86.9, 400).astype(np.float32)
    e = np.stack([np.zeros_like(t), t], axis=1).reshape(-1)
    rp = torch.arange(0, 2 * len(t) + 1, 2, dtype=torch.int32)
    y = run_forward(rp, torch.from_numpy(e), len(t)).numpy().reshape(-1, 2)
    assert np.array_equal(y[:, 0], np.ones(len(t), dtype=np.float32))
    assert np.array_equal(y[:, 1].view(np.uint32), exp_acc(t).view(np.uint32))


def test_many_rows():
    ec.check_many_rows("cpu")


def test_softmax_accuracy():
    ec.check_softmax_accuracy("cpu")


def test_gradcheck():
    ec.check_gradcheck("cpu")


def test_attention_layer_f32():
    ec.check_attention_f32("cpu")


def test_op_layer():
    ec.check_op_layer("cpu")


def test_sbp_signatures():
    ec.check_sbp()


def test_argument_checks():
    rp = torch.tensor([0, 2, 3], dtype=torch.int32)
    e = torch.tensor([1.0, 2.0, 3.0])
    y = torch.empty_like(e)
    I, F = _lib.DT_INT32, _lib.DT_FLOAT
    call = lambda *a: LIB.ofx_edge_softmax_csr_cpu(0, *a, None)
    p = (rp.data_ptr(), e.data_ptr(), y.data_ptr())
    assert call(I, F, 2, 3, *p, 0, 2) == _lib.OFX_OK
    assert call(I, F, 2, 3, *p, 1, 3) == _lib.OFX_EINVAL          # row range outside [0, m)
    assert call(I, F, 2, -1, *p, 0, 2) == _lib.OFX_EINVAL         # negative size
    assert call(I, F, 2, 3, rp.data_ptr(), None, y.data_ptr(), 0, 2) == _lib.OFX_EINVAL
    assert call(I, _lib.DT_INT64, 2, 3, *p, 0, 2) == _lib.OFX_EUNSUPPORTED
    assert call(F, F, 2, 3, *p, 0, 2) == _lib.OFX_EUNSUPPORTED
    assert call(I, F, 2, 1 << 31, *p, 0, 2) == _lib.OFX_EINVAL    # int32 cannot address nnz
    size = ctypes.c_size_t(7)
    assert LIB.ofx_edge_softmax_csr_workspace_size(I, F, 2, 3, None, ctypes.byref(size)) == 0
    assert size.value == 0
    assert LIB.ofx_edge_softmax_csr_workspace_size(I, F, 2, 3, None, None) == _lib.OFX_EINVAL
    bad = _lib.Options()
    bad.magic = 0
    assert LIB.ofx_edge_softmax_csr_cpu(0, I, F, 2, 3, *p, 0, 2, ctypes.byref(bad)) == \
        _lib.OFX_EINVAL


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not found")
def test_cpu_kernels_under_sanitizers(tmp_path):
    """The two kCPU kernels (edge_softmax_cpu.cpp with errors.cpp) built from source with
    AddressSanitizer + UndefinedBehaviorSanitizer and driven by
    tests/native/edge_softmax_sanitize.cpp, which also checks them against a naive softmax.
    Host code only: nothing is loaded into Python and nothing runs on the GPU."""
    build_and_run(tmp_path, "edge_softmax_sanitize", ["edge_softmax_cpu.cpp", "errors.cpp"])

"""Per-row top-k selection, the kCPU kernel (csrc/row_topk_cpu.cpp) against the numpy
restatement over the case table of tests/row_topk_cases.py, bad inputs, and the selection between
`sddmm` and `edge_softmax`."""
import numpy as np
import pytest
import torch

import oneflow_spmm as fs
from oneflow_spmm import _lib
from tests import row_topk_cases as cases

IDX = cases.IDX


@pytest.mark.parametrize("idx", list(IDX))
@pytest.mark.parametrize("val", list(cases.VAL))
@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("k", cases.KS)
def test_equals_reference(k, largest, val, idx):
    it = IDX[idx]
    rp, ci, values, ref = cases.case(k, largest, val)
    got = fs.row_topk(cases.tensor(rp, it), cases.tensor(ci, it), values, k, largest=largest)
    cases.assert_topk(got, ref, ci, it, "cpu")


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65])
def test_partial_groups(m):
    rp, ci, values = cases.uniform_rows(m)
    ref = cases.reference(rp, values, 3, True)[:2]
    got = fs.row_topk(cases.tensor(rp, torch.int32), cases.tensor(ci, torch.int32), values, 3)
    cases.assert_topk(got, ref, ci, torch.int32, "cpu")


@pytest.mark.parametrize("threads", [1, 3])
def test_threads_do_not_change_the_result(threads):
    rp, ci, values, ref = cases.case(64, True, "f32")
    got = fs.row_topk(cases.tensor(rp, torch.int64), cases.tensor(ci, torch.int64), values, 64,
                      num_threads=threads)
    cases.assert_topk(got, ref, ci, torch.int64, "cpu")


@pytest.mark.parametrize("idx", list(IDX))
def test_bad_inputs_raise_and_the_next_call_is_right(idx):
    it = IDX[idx]
    rp, ci, values, ref = cases.case(3, True, "f32")
    for broken in cases.bad_row_ptrs(rp):
        with pytest.raises(RuntimeError, match="outside"):
            fs.row_topk(cases.tensor(broken, it), cases.tensor(ci, it), values, 3)
    cases.assert_topk(fs.row_topk(cases.tensor(rp, it), cases.tensor(ci, it), values, 3), ref, ci, it, "cpu")


def test_arguments_and_names():
    rp, ci, values, _ = cases.case(3, True, "f32")
    rp, ci = cases.tensor(rp, torch.int64), cases.tensor(ci, torch.int64)
    for k in (0, -1):
        with pytest.raises(RuntimeError, match="k"):
            fs.row_topk(rp, ci, values, k)
    with pytest.raises(RuntimeError, match="values"):
        fs.row_topk(rp, ci, values[:-1], 3)
    lib, dt = _lib.LIB, _lib.DT_INT64
    assert lib.ofx_row_topk(None, dt, _lib.DT_FLOAT, 4, 4, None, None, None, 0, 1, None, None, None,
                            None, None, None, 0) == _lib.OFX_EINVAL
    empty = fs.row_topk(torch.zeros(5, dtype=torch.int32), ci[:0].int(), values[:0], 2)  # nnz = 0
    assert empty[0].tolist() == [0] * 5 and empty[1].numel() == 0 and empty[2].numel() == 0
    assert fs.row_topk is fs.sampling.row_topk and "row_topk" in fs.__all__
    assert {"ofx_row_topk_workspace_size", "ofx_row_topk", "ofx_row_topk_cpu"} <= set(_lib.EXPORTED)


def test_through_the_ops():
    cases.check_attention(torch.device("cpu"))

"""CSR x CSR, the kCPU kernel (csrc/spgemm_cpu.cpp) against the dense float64
reference over the case table of tests/spgemm_cases.py: every value and index dtype, pattern only,
the order of the sum, chaining into itself and into `spmm`, bad inputs, names."""
import pytest
import torch

import oneflow_spmm as fs
from oneflow_spmm import _lib
from tests import spgemm_cases as cases

CPU = torch.device("cpu")


@pytest.mark.parametrize("idx", list(cases.IDX))
@pytest.mark.parametrize("val", list(cases.VAL))
@pytest.mark.parametrize("name", list(cases.CASES))
def test_equals_reference(name, val, idx):
    cases.check_case(fs, name, val, idx, CPU)


@pytest.mark.parametrize("name", ["classes", "m9"])
def test_threads_do_not_change_the_result(name):
    args = cases.operands(name, "f32", torch.int64)
    one, four = (fs.spgemm(*args, num_threads=t) for t in (1, 4))
    assert all(torch.equal(x, y) for x, y in zip(one, four))


def test_the_order_of_the_sum():
    cases.check_order(fs, CPU)


def test_chaining():
    cases.check_chain(fs, CPU)


@pytest.mark.parametrize("idx", list(cases.IDX))
def test_bad_inputs_raise_and_the_next_call_is_right(idx):
    cases.check_bad_inputs(fs, idx, CPU)


def test_arguments_and_names():
    args = cases.operands("m7", "f32", torch.int32)
    with pytest.raises(RuntimeError, match="both"):
        fs.spgemm(args[0], args[1], None, *args[3:])
    with pytest.raises(TypeError):
        fs.spgemm(*args[:5], args[5].double(), args[6])
    lib, dt = _lib.LIB, _lib.DT_INT32
    nbytes = _lib.ctypes.c_size_t(0)
    for sizes in ((2 ** 31, 1, 1, 0, 0), (1, 1, 1, 0, 2 ** 31), (1, 1, -1, 0, 0)):
        assert lib.ofx_spgemm_workspace_size(dt, _lib.DT_FLOAT, *sizes, _lib.ctypes.byref(nbytes)) == _lib.OFX_EINVAL
    assert fs.spgemm is fs.build.spgemm and "spgemm" in fs.__all__
    assert {"ofx_spgemm_workspace_size", "ofx_spgemm_count", "ofx_spgemm_fill", "ofx_spgemm_count_cpu",
            "ofx_spgemm_fill_cpu"} <= set(_lib.EXPORTED)

"""The SpMM over per-edge feature vectors on the host (`spmm_edge`; ops "spmm_csr_edge", "_grad_e",
"_grad_b"): the kCPU kernels of csrc/spmm_edge_cpu.cpp against the float64 reference, bit for bit
(spmm_edge_cases.py), over the case table; thread-count independence, the `spmm` identity,
autograd, the op layer's tmp sizes and the argument errors."""
from __future__ import annotations

import pytest

import spmm_edge_cases as ec
from oneflow_spmm import _lib


@pytest.mark.parametrize("op,act", ec.PAIRS)
@pytest.mark.parametrize("name", ec.CASES)
def test_case_table(name, op, act):
    ec.check_case("cpu", name, op, act)


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_bits_do_not_depend_on_num_threads(dt):
    tensors = ec.random_problem(dt, "cpu")
    for op, act in ec.PAIRS:
        for split in (0, 8):
            one = ec.run_random(tensors, op, act, split, num_threads=1)
            four = ec.run_random(tensors, op, act, split, num_threads=4)
            for a, b, what in zip(one, four, ("out", "de", "db")):
                ec.bits_equal(a, b, f"{what} {dt} {op} {act} split={split}: 1 vs 4 threads")


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_mul_on_expanded_values_has_spmm_bits(dt):
    ec.check_spmm_identity("cpu", dt)


def test_autograd(monkeypatch):
    ec.check_autograd("cpu", monkeypatch)


@pytest.mark.parametrize("it", [_lib.DT_INT32, _lib.DT_INT64])
@pytest.mark.parametrize("vt", [_lib.DT_FLOAT, _lib.DT_DOUBLE, _lib.DT_FLOAT16, _lib.DT_BFLOAT16])
def test_functional_tmp_sizes(vt, it):
    ec.check_tmp_sizes(vt, it)


def test_argument_errors():
    ec.check_errors("cpu")

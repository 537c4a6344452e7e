"""`segment_matmul` on the host: the kCPU kernels of csrc/segment_matmul_cpu.cpp through the op
layer and autograd against the float64 torch loop (segment_matmul_cases.py): the exact case table,
the contract's bound on normal inputs with repeatability, and the argument errors."""
from __future__ import annotations

import pytest

import segment_matmul_cases as sc


@pytest.mark.parametrize("trans_w", [False, True])
@pytest.mark.parametrize("it", sc.INDEX)
@pytest.mark.parametrize("dt", sc.DTYPES)
@pytest.mark.parametrize("name", sc.CASES)
def test_case_table(name, dt, it, trans_w):
    sc.check_exact("cpu", name, dt, it, trans_w)


@pytest.mark.parametrize("with_idx", [False, True])
@pytest.mark.parametrize("dt", sc.DTYPES)
def test_bound_and_repeatability(dt, with_idx):
    sc.check_bound("cpu", dt, with_idx)


def test_argument_errors():
    sc.check_errors("cpu")

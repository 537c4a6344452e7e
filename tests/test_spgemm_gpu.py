"""CSR x CSR on the GPU (csrc/spgemm.hip): the HIP hash kernels against the dense
float64 reference and, bit for bit, the kCPU kernel over the case table of tests/spgemm_cases.py
(rows on eight lanes, a wave, a block, and hub rows over column ranges), pattern only, the order of
the sum, chaining, bad inputs."""
import pytest
import torch

import oneflow_spmm as fs
from tests import spgemm_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("idx", list(cases.IDX))
@pytest.mark.parametrize("val", list(cases.VAL))
@pytest.mark.parametrize("name", list(cases.CASES))
def test_equals_reference_and_the_cpu_kernel(device, name, val, idx):
    got = cases.check_case(fs, name, val, idx, device)
    host = fs.spgemm(*cases.operands(name, val, cases.IDX[idx]))
    for g, h in zip(got, host):
        assert torch.equal(g.cpu().view(torch.uint8), h.view(torch.uint8))


def test_the_order_of_the_sum(device):
    cases.check_order(fs, device)


def test_chaining(device):
    cases.check_chain(fs, device)


@pytest.mark.parametrize("idx", list(cases.IDX))
def test_bad_inputs_raise_and_the_next_call_is_right(device, idx):
    cases.check_bad_inputs(fs, idx, device)

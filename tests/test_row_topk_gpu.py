"""Per-row top-k selection on the GPU (csrc/row_topk.hip): the HIP kernels against
the numpy restatement and the kCPU kernel over the case table of tests/row_topk_cases.py (rows of
up to 64 entries on eight lanes, up to 512 on a wave, hub rows on a block), partial groups, bad
inputs, and the selection between `sddmm` and `edge_softmax`."""
import pytest
import torch

import oneflow_spmm as fs
from tests import row_topk_cases as cases

pytestmark = pytest.mark.gpu

IDX = cases.IDX


@pytest.mark.parametrize("idx", list(IDX))
@pytest.mark.parametrize("val", list(cases.VAL))
@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("k", cases.KS)
def test_equals_reference(device, k, largest, val, idx):
    it = IDX[idx]
    rp, ci, values, ref = cases.case(k, largest, val)
    host = (cases.tensor(rp, it), cases.tensor(ci, it), values)
    got = fs.row_topk(*(a.to(device) for a in host), k, largest=largest)
    cases.assert_topk(got, ref, ci, it, "cuda")
    cases.assert_topk(got, fs.row_topk(*host, k, largest=largest)[::2], ci, it, "cuda")


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65])
def test_partial_groups(device, m):
    rp, ci, values = cases.uniform_rows(m)
    ref = cases.reference(rp, values, 3, True)[:2]
    got = fs.row_topk(cases.tensor(rp, torch.int32, device), cases.tensor(ci, torch.int32, device),
                      values.to(device), 3)
    cases.assert_topk(got, ref, ci, torch.int32, "cuda")


@pytest.mark.parametrize("idx", list(IDX))
def test_bad_inputs_raise_and_the_next_call_is_right(device, idx):
    it = IDX[idx]
    rp, ci, values, ref = cases.case(3, True, "f32")
    good = (cases.tensor(rp, it, device), cases.tensor(ci, it, device), values.to(device))
    for broken in cases.bad_row_ptrs(rp):
        with pytest.raises(RuntimeError, match="outside"):
            fs.row_topk(cases.tensor(broken, it, device), good[1], good[2], 3)
    torch.cuda.synchronize()
    cases.assert_topk(fs.row_topk(*good, 3), ref, ci, it, "cuda")


def test_no_entries(device):
    got = fs.row_topk(torch.zeros(5, dtype=torch.int32, device=device),
                      torch.zeros(0, dtype=torch.int32, device=device),
                      torch.zeros(0, device=device), 2)
    assert got[0].tolist() == [0] * 5 and got[1].numel() == 0 and got[2].numel() == 0


def test_through_the_ops(device):
    cases.check_attention(device)

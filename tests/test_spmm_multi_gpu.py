"""The multi-aggregator SpMM on the MI355X (`spmm_multi`): the HIP kernels of csrc/spmm_multi.hip
against the float64 reference, the contract's var / std bits and bound and the existing ops' bits
(spmm_multi_cases.py): every lane group and a second column tile, the general path, the boundary
row lengths under the default and a forced schedule (the hub combine), repeated columns, columns
outside [0, K), a shifted leading dimension, a row range, a subset of the aggregators, the
specials; against the kCPU kernel on every slice; the gradients; a workspace that is too small."""
from __future__ import annotations

import pytest
import torch

import oneflow_spmm as flow_spmm
import spmm_multi_cases as mc
from oneflow_spmm import ops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", mc.CASES)
def test_case_table(device, name):
    mc.check_case(device, name)
    for got, want, what in zip(mc.run(device, name), mc.run("cpu", name),
                               ("out", "arg_max", "arg_min")):
        if want is not None:
            mc.bits_equal(got, want, f"{name} {what}: HIP vs kCPU")


@pytest.mark.parametrize("aggrs", [mc.AGGRS, ("std", "max"), ("mean",)])
def test_gradients_match_torch_autograd(device, aggrs):
    mc.check_gradients(device, aggrs)


def test_public_call_and_small_workspace(device):
    rp, ci, vals, b = (t.to(device) for t in mc.problem("f32_n64"))
    m = rp.numel() - 1
    out = flow_spmm.spmm_multi(rp, ci, vals, m, mc.K, b, ("min", "var"), mc.EPS)
    stored = mc.run(device, "f32_n64")[0]
    for i, a in enumerate(("min", "var")):
        mc.bits_equal(out[:, i, :], stored[:, mc.AGGRS.index(a), :], a)
    with pytest.raises(flow_spmm.OfxError, match="workspace"):  # the hub row needs its records
        ops.spmm_csr_multi(rp, ci, vals, b, m, mc.K, 63, workspace_bytes=8)

"""GAT attention weights (ops "gat_softmax_csr_heads" and its gradient) on host tensors: the kCPU
kernels against the numpy restatement of the scores fed to the existing multi-head edge softmax,
bit for bit; the activation's edges, special values, the public API, autograd, the op layer, the
C-ABI's argument checks, and the kCPU kernels under the host sanitizers (gat_softmax_cases.py)."""
from __future__ import annotations

import os

import pytest
import torch

import edge_softmax_heads_cases as hc
import gat_softmax_cases as gc
from helpers import DTYPES
from sanitize_helpers import CLANG, build_and_run


@pytest.mark.parametrize("it", [torch.int32, torch.int64])
@pytest.mark.parametrize("h,dt", hc.HEADS_DT)
def test_boundary_lengths_and_head_counts(h, dt, it):
    gc.check_boundaries("cpu", h, DTYPES[dt], it)


@pytest.mark.parametrize("h,dt", [(3, "f32"), (8, "f32"), (8, "bf16"), (5, "f16"), (2, "f64")])
@pytest.mark.parametrize("mix", list(hc.LG_MIXES))
def test_lane_group_mixes(mix, h, dt):
    gc.check_lane_groups("cpu", mix, h, DTYPES[dt])


def test_many_rows():
    gc.check_many_rows("cpu", 3, torch.float32)


@pytest.mark.parametrize("h,dt", [(4, "f32"), (3, "f32"), (8, "bf16"), (2, "f64")])
def test_unaligned_base_and_row_ranges(h, dt):
    gc.check_unaligned_and_ranges("cpu", h, DTYPES[dt])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_columns_out_of_range(dt):
    gc.check_columns_out_of_range("cpu", DTYPES[dt])


@pytest.mark.parametrize("slope", gc.SLOPES)
@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_activation_edges(dt, slope):
    gc.check_activation_edges("cpu", DTYPES[dt], slope)


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_special_values_stay_in_their_head_and_row(dt):
    gc.check_special_confined("cpu", DTYPES[dt])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_single_head_and_empty(dt):
    gc.check_degenerate("cpu", DTYPES[dt])


def test_argument_checks():
    gc.check_argument_checks("cpu")


def test_kernel_registrations():
    gc.check_registrations()


def test_sbp_signatures():
    gc.check_sbp()


def test_op_layer():
    gc.check_op_layer("cpu")


def test_public_api():
    gc.check_public_api("cpu")


@pytest.mark.parametrize("h,dt", [(3, "f32"), (8, "f32"), (4, "bf16"), (2, "f64"), (1, "f16")])
def test_gradients_match_the_reference_chain(h, dt):
    gc.check_grads("cpu", h, DTYPES[dt])


def test_needs_input_grad():
    gc.check_needs_input_grad("cpu")


def test_gradcheck():
    gc.check_gradcheck("cpu")


def test_gat_attention_dense_reference_f32():
    gc.check_dense_reference_f32("cpu")


def test_result_does_not_depend_on_threads():
    gc.check_threads_do_not_matter()


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not found")
def test_cpu_kernels_under_sanitizers(tmp_path):
    """The kCPU kernels (gat_softmax_cpu.cpp with errors.cpp) built from source with
    AddressSanitizer + UndefinedBehaviorSanitizer and driven by
    tests/native/gat_softmax_sanitize.cpp, which also checks them against a naive loop.  Host code
    only: nothing is loaded into Python and nothing runs on the GPU."""
    build_and_run(tmp_path, "gat_softmax_sanitize", ["gat_softmax_cpu.cpp", "errors.cpp"])

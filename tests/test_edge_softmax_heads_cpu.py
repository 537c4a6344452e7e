"""Multi-head edge softmax (ops "edge_softmax_csr_heads" and its gradient) on host tensors: the
kCPU kernels against the numpy restatement of the single-head contract per column and against the
single-head op, bit for bit; the public API, the op layer, the C-ABI's argument checks, and the
kCPU kernels under the host sanitizers (edge_softmax_heads_cases.py)."""
from __future__ import annotations

import os

import pytest
import torch

import edge_softmax_heads_cases as hc
import heads_cases
from helpers import DTYPES
from sanitize_helpers import CLANG, build_and_run


@pytest.mark.parametrize("it", [torch.int32, torch.int64])
@pytest.mark.parametrize("h,dt", hc.HEADS_DT)
def test_boundary_lengths_and_head_counts(h, dt, it):
    hc.check_boundaries("cpu", h, DTYPES[dt], it)


@pytest.mark.parametrize("h,dt", [(3, "f32"), (8, "f32"), (8, "bf16"), (5, "f16"), (2, "f64")])
@pytest.mark.parametrize("mix", list(hc.LG_MIXES))
def test_lane_group_mixes(mix, h, dt):
    hc.check_lane_groups("cpu", mix, h, DTYPES[dt])


@pytest.mark.parametrize("h,dt", [(4, "f32"), (3, "f32"), (8, "bf16"), (2, "f64")])
def test_unaligned_base_and_row_ranges(h, dt):
    hc.check_unaligned_and_ranges("cpu", h, DTYPES[dt])


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_special_values_stay_in_their_head(dt):
    hc.check_special_confined("cpu", DTYPES[dt])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_single_head_and_empty(dt):
    hc.check_single_head_bits("cpu", DTYPES[dt])


def test_public_api(monkeypatch):
    hc.check_public_api("cpu", monkeypatch)


def test_attention_layer_heads_f32():
    heads_cases.check_attention_heads_f32("cpu")


def test_op_layer():
    hc.check_op_layer("cpu")


def test_sbp_signatures():
    hc.check_sbp()


def test_argument_checks():
    hc.check_argument_checks("cpu")


def test_result_does_not_depend_on_threads():
    hc.check_threads_do_not_matter()


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not found")
def test_cpu_kernels_under_sanitizers(tmp_path):
    """The kCPU multi-head kernels (edge_softmax_cpu.cpp with errors.cpp) built from source with
    AddressSanitizer + UndefinedBehaviorSanitizer and driven by
    tests/native/edge_softmax_heads_sanitize.cpp, which also checks them against a naive per-column
    softmax.  Host code only: nothing is loaded into Python and nothing runs on the GPU."""
    build_and_run(tmp_path, "edge_softmax_heads_sanitize", ["edge_softmax_cpu.cpp", "errors.cpp"])

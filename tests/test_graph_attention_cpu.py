"""Fused multi-head graph attention (op "graph_attention_csr_heads", `oneflow_spmm.graph_attention`)
on host tensors: the kCPU entry against the composition of the three C-ABI entries, bit for bit;
the public API, the op layer, autograd against the composed layer's, the C-ABI's argument checks,
and the kCPU entry under the host sanitizers (graph_attention_cases.py)."""
from __future__ import annotations

import os

import pytest

import graph_attention_cases as gc
from sanitize_helpers import CLANG, build_and_run


@pytest.mark.parametrize("h,d,dt", gc.HD_DT)
def test_matrix(h, d, dt):
    """Every (H, D) and dtype over every boundary length, under the default schedule and the two
    that chunk short rows."""
    gc.check_forward("cpu", h, d, dt, schedules=("default", "split8", "split8_chunk4"))


@pytest.mark.parametrize("h,d,dt", [(3, 5, "f32"), (8, 16, "bf16"), (4, 16, "f64"), (5, 1, "f16")])
def test_int64_indices_padded_and_shifted(h, d, dt):
    gc.check_forward("cpu", h, d, dt, "i64", exact=True, schedules=("default", "split8"), pad=gc.PAD,
                     shift=1)


def test_hub_schedule_comes_from_d():
    """H = 8, D = 64: a 300-nonzero row stays whole (the split of D = 64 is 512; that of
    H*D = 512 would be 128), next to rows that are cut."""
    gc.check_forward("cpu", 8, 64, "f32", lengths=(300, 3, 0, 513, 1100), k=1200)


@pytest.mark.parametrize("h,d,dt", [(3, 5, "f32"), (4, 16, "bf16")])
def test_row_ranges(h, d, dt):
    gc.check_row_ranges("cpu", h, d, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_columns_out_of_range(dt):
    gc.check_columns_out_of_range("cpu", dt)


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_special_values_stay_in_their_head(dt):
    gc.check_special_confined("cpu", dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_single_head_and_empty(dt):
    gc.check_single_head_and_empty("cpu", dt)


def test_public_api():
    gc.check_public_api("cpu")


def test_op_layer():
    gc.check_op_layer("cpu")


def test_argument_checks():
    gc.check_argument_checks("cpu")


@pytest.mark.parametrize("with_attn", [False, True])
@pytest.mark.parametrize("h,d", [(3, 5), (8, 16)])
def test_gradients_match_composed_layer(h, d, with_attn):
    gc.check_grads_match_composition("cpu", h, d, with_attn)


def test_only_requested_gradients():
    gc.check_needs_input_grad("cpu")


def test_gradcheck_f64():
    gc.check_gradcheck("cpu")


def test_dense_reference_f32():
    gc.check_dense_reference_f32("cpu")


def test_result_does_not_depend_on_threads():
    gc.check_threads_do_not_matter()


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not found")
def test_cpu_kernel_under_sanitizers(tmp_path):
    """The kCPU entry (graph_attention_heads_cpu.cpp with the three kCPU kernels it runs and
    errors.cpp) built from source with AddressSanitizer + UndefinedBehaviorSanitizer and driven by
    tests/native/graph_attention_sanitize.cpp, which also checks it against a naive attention.
    Host code only: nothing is loaded into Python and nothing runs on the GPU."""
    build_and_run(tmp_path, "graph_attention_sanitize",
                  ["graph_attention_heads_cpu.cpp", "spmm_heads_cpu.cpp", "edge_softmax_cpu.cpp", "errors.cpp"])

"""GATv2 attention scores (ops "gatv2_scores_csr_heads" and its gradient) on host tensors: the kCPU
kernels against the numpy restatement of the per-nonzero tensors fed to the existing multi-head
SDDMM / SpMM, bit for bit; the activation's edges, special values, the public API, autograd, the op
layer, the C-ABI's argument checks, and the kCPU kernels under the host sanitizers
(gatv2_cases.py)."""
from __future__ import annotations

import os

import pytest

import gatv2_cases as gc
from helpers import DTYPES
from sanitize_helpers import CLANG, build_and_run


@pytest.mark.parametrize("h,d,dt", gc.fwd_cases(gc.FAST_HD))
def test_scores_fast_path_shapes(h, d, dt):
    gc.check_forward("cpu", h, d, dt)


@pytest.mark.parametrize("h,d,dt", gc.fwd_cases(gc.GENERAL_HD))
def test_scores_general_path_shapes(h, d, dt):
    gc.check_forward("cpu", h, d, dt)


@pytest.mark.parametrize("h,d,dt", [(8, 8, "f32"), (3, 5, "bf16")])
def test_scores_int64_indices(h, d, dt):
    gc.check_forward("cpu", h, d, dt, "i64")


@pytest.mark.parametrize("h,d,dt", [(h, d, dt) for dt, hds in gc.GRAD_HD.items() for h, d in hds])
def test_gradient_widths(h, d, dt):
    gc.check_grad("cpu", h, d, dt, lengths=None if h * d <= 128 else tuple(gc.SHORT))


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
@pytest.mark.parametrize("h,d", gc.GRAD_GENERAL_HD)
def test_gradient_general_path(h, d, dt):
    gc.check_grad("cpu", h, d, dt)


@pytest.mark.parametrize("h,d,dt", [(4, 16, "f32"), (3, 5, "bf16")])
def test_gradient_int64_indices(h, d, dt):
    gc.check_grad("cpu", h, d, dt, "i64", schedules=("default", "split8"))


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_scores_against_tree_sum(dt):
    gc.check_tree_sum("cpu", dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_identity_activation_is_the_sddmm(dt):
    gc.check_sddmm_identity("cpu", dt)


@pytest.mark.parametrize("h,d,dt", [(4, 16, "f32"), (3, 5, "f32"), (8, 8, "bf16"), (2, 8, "f64")])
def test_row_ranges(h, d, dt):
    gc.check_row_ranges("cpu", h, d, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_columns_out_of_range(dt):
    gc.check_columns_out_of_range("cpu", dt)


@pytest.mark.parametrize("slope", gc.SLOPES)
@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_activation_edges(dt, slope):
    gc.check_activation_edges("cpu", DTYPES[dt], slope)


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_special_values_stay_in_their_head_and_row(dt):
    gc.check_special_confined("cpu", dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_degenerate_sizes(dt):
    gc.check_degenerate("cpu", dt)


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


@pytest.mark.parametrize("h,d,dt", [(3, 5, "f32"), (8, 8, "f32"), (4, 8, "bf16"), (2, 4, "f64"),
                                    (1, 16, "f16")])
def test_gradients_match_the_reference_chain(h, d, dt):
    gc.check_grads("cpu", h, d, dt)


def test_needs_input_grad(monkeypatch):
    gc.check_needs_input_grad("cpu", monkeypatch)


def test_gradcheck():
    gc.check_gradcheck("cpu")


def test_gatv2_attention_dense_reference_f32():
    gc.check_dense_reference_f32("cpu")


def test_result_does_not_depend_on_threads():
    gc.check_threads_do_not_matter()


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not found")
def test_cpu_kernels_under_sanitizers(tmp_path):
    """The kCPU kernels (gatv2_scores_cpu.cpp with errors.cpp) built from source with
    AddressSanitizer + UndefinedBehaviorSanitizer and driven by tests/native/gatv2_sanitize.cpp,
    which also checks them against a naive loop.  Host code only: nothing is loaded into Python and
    nothing runs on the GPU."""
    build_and_run(tmp_path, "gatv2_sanitize", ["gatv2_scores_cpu.cpp", "errors.cpp"])

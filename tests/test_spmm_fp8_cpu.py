"""Multi-head SpMM over an FP8 feature table (op "spmm_csr_heads_fp8") on host tensors: the kCPU
kernel against the torch restatement of the scaled values and the dequantised table fed to the
existing kCPU multi-head SpMM, bit for bit; every code of both formats, special values, addressing,
row ranges, quantize_rows_fp8, the public API, autograd, the op layer, the C-ABI's argument checks,
and the kCPU kernel under the host sanitizers (spmm_fp8_cases.py)."""
from __future__ import annotations

import os

import pytest

import spmm_fp8_cases as fc
from sanitize_helpers import CLANG, build_and_run


@pytest.mark.parametrize("h,d,fmt,dt", fc.grid(fc.FAST_HD))
def test_fast_path_shapes(h, d, fmt, dt):
    fc.check_forward("cpu", h, d, fmt, dt)


@pytest.mark.parametrize("fmt,dt", [("e4m3", "bf16"), ("e5m2", "f32")])
def test_second_column_tile(fmt, dt):
    fc.check_forward("cpu", *fc.TILE_HD, fmt, dt)


@pytest.mark.parametrize("h,d,fmt,dt", fc.grid(fc.GENERAL_HD))
def test_general_path_shapes(h, d, fmt, dt):
    fc.check_forward("cpu", h, d, fmt, dt)


@pytest.mark.parametrize("h,d,fmt,dt", [(8, 16, "e4m3", "f32"), (3, 5, "e5m2", "bf16"),
                                        (16, 16, "e5m2", "f16")])
def test_int64_indices(h, d, fmt, dt):
    fc.check_forward("cpu", h, d, fmt, dt, "i64")


@pytest.mark.parametrize("dt", fc.TYPES)
@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_every_code(fmt, dt):
    fc.check_every_code("cpu", fmt, dt)


@pytest.mark.parametrize("dt", fc.TYPES)
@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_special_values_stay_in_their_head_and_row(fmt, dt):
    fc.check_special_values("cpu", fmt, dt)


@pytest.mark.parametrize("h,d,fmt,dt", [(8, 16, "e4m3", "f32"), (3, 5, "e4m3", "f16"),
                                        (4, 16, "e5m2", "bf16")])
def test_repeated_columns(h, d, fmt, dt):
    fc.check_repeated_columns("cpu", h, d, fmt, dt)


@pytest.mark.parametrize("fmt,dt", [("e4m3", "f32"), ("e5m2", "bf16"), ("e4m3", "f16")])
def test_columns_out_of_range(fmt, dt):
    fc.check_columns_out_of_range("cpu", fmt, dt)


@pytest.mark.parametrize("h,d,fmt,dt", [(4, 16, "e4m3", "f32"), (3, 5, "e5m2", "f32"),
                                        (8, 16, "e5m2", "bf16")])
def test_row_ranges(h, d, fmt, dt):
    fc.check_row_ranges("cpu", h, d, fmt, dt)


@pytest.mark.parametrize("dt", fc.TYPES)
@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_without_a_scale_it_is_spmm_on_the_converted_table(fmt, dt):
    fc.check_no_scale_identity("cpu", fmt, dt)


def test_quantize_rows_fp8():
    fc.check_quantize("cpu")


@pytest.mark.parametrize("dt", fc.TYPES)
def test_degenerate_sizes(dt):
    fc.check_degenerate("cpu", dt)


def test_argument_checks():
    fc.check_argument_checks("cpu")


def test_kernel_registrations():
    fc.check_registrations()


def test_sbp_signatures():
    fc.check_sbp()


def test_op_layer_and_public_api():
    fc.check_op_layer("cpu")


@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_gradient_in_values_matches_the_reference_composition(fmt):
    fc.check_autograd("cpu", fmt)


def test_needs_input_grad(monkeypatch):
    fc.check_needs_input_grad("cpu", monkeypatch)


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not found")
def test_cpu_kernel_under_sanitizers(tmp_path):
    """The kCPU kernel (spmm_heads_fp8_cpu.cpp with errors.cpp) built from source with
    AddressSanitizer + UndefinedBehaviorSanitizer and driven by tests/native/spmm_fp8_sanitize.cpp,
    which also checks it against a naive loop.  Host code only: nothing is loaded into Python and
    nothing runs on the GPU."""
    build_and_run(tmp_path, "spmm_fp8_sanitize", ["spmm_heads_fp8_cpu.cpp", "errors.cpp"])

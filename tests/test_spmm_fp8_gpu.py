"""Multi-head SpMM over an FP8 feature table (op "spmm_csr_heads_fp8") on the MI355X: the HIP
kernel of csrc/spmm_heads_fp8.hip against the torch restatement of the scaled values and the
dequantised table fed to the existing kCPU multi-head SpMM and against the new kCPU entry, bit for
bit (spmm_fp8_cases.py): every step of the fast path's lane ladder and a second column tile, the
general path, the boundary row lengths under every schedule, both formats x three value types with
and without the scale, every code, special values, repeated columns, columns outside [0, K),
unaligned bases, row ranges, the public API, autograd, the op layer, the argument checks and graph
capture."""
from __future__ import annotations

import pytest

import spmm_fp8_cases as fc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("h,d,fmt,dt", fc.grid(fc.FAST_HD))
def test_fast_path_shapes(device, h, d, fmt, dt):
    fc.check_forward(device, h, d, fmt, dt)


@pytest.mark.parametrize("fmt,dt", [("e4m3", "bf16"), ("e5m2", "f32")])
def test_second_column_tile(device, fmt, dt):
    fc.check_forward(device, *fc.TILE_HD, fmt, dt)


@pytest.mark.parametrize("h,d,fmt,dt", fc.grid(fc.GENERAL_HD))
def test_general_path_shapes(device, h, d, fmt, dt):
    fc.check_forward(device, h, d, fmt, dt)


@pytest.mark.parametrize("h,d,fmt,dt", [(8, 16, "e4m3", "f32"), (3, 5, "e5m2", "bf16"),
                                        (16, 16, "e5m2", "f16")])
def test_int64_indices(device, h, d, fmt, dt):
    fc.check_forward(device, h, d, fmt, dt, "i64")


@pytest.mark.parametrize("dt", fc.TYPES)
@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_every_code(device, fmt, dt):
    fc.check_every_code(device, fmt, dt)


@pytest.mark.parametrize("dt", fc.TYPES)
@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_special_values_stay_in_their_head_and_row(device, fmt, dt):
    fc.check_special_values(device, fmt, dt)


@pytest.mark.parametrize("h,d,fmt,dt", [(8, 16, "e4m3", "f32"), (3, 5, "e4m3", "f16"),
                                        (4, 16, "e5m2", "bf16")])
def test_repeated_columns(device, h, d, fmt, dt):
    fc.check_repeated_columns(device, h, d, fmt, dt)


@pytest.mark.parametrize("fmt,dt", [("e4m3", "f32"), ("e5m2", "bf16"), ("e4m3", "f16")])
def test_columns_out_of_range(device, fmt, dt):
    fc.check_columns_out_of_range(device, fmt, dt)


@pytest.mark.parametrize("h,d,fmt,dt", [(4, 16, "e4m3", "f32"), (3, 5, "e5m2", "f32"),
                                        (8, 16, "e5m2", "bf16")])
def test_row_ranges(device, h, d, fmt, dt):
    fc.check_row_ranges(device, h, d, fmt, dt)


@pytest.mark.parametrize("dt", fc.TYPES)
@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_without_a_scale_it_is_spmm_on_the_converted_table(device, fmt, dt):
    fc.check_no_scale_identity(device, fmt, dt)


def test_quantize_rows_fp8(device):
    fc.check_quantize(device)


@pytest.mark.parametrize("dt", fc.TYPES)
def test_degenerate_sizes(device, dt):
    fc.check_degenerate(device, dt)


def test_argument_checks(device):
    fc.check_argument_checks(device)


def test_op_layer_and_public_api(device):
    fc.check_op_layer(device)


@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_gradient_in_values_matches_the_reference_composition(device, fmt):
    fc.check_autograd(device, fmt)


def test_needs_input_grad(device, monkeypatch):
    fc.check_needs_input_grad(device, monkeypatch)


@pytest.mark.graph_capture
@pytest.mark.parametrize("h,d,fmt,dt", [(8, 16, "e4m3", "bf16"), (3, 5, "e5m2", "f32")])
def test_graph_capture(h, d, fmt, dt):
    """The forward captured into a graph and replayed on new inputs: the same bits as a fresh eager
    launch, the kCPU entry and the composition.  (8, 16) takes the fast path, (3, 5) the general
    one."""
    fc.check_graph_capture(h, d, fmt, dt)

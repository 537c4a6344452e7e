"""GATv2 attention scores (ops "gatv2_scores_csr_heads" and its gradient) on the MI355X: the HIP
kernels of csrc/gatv2_scores_heads.hip and csrc/gatv2_scores_grad.hip against the numpy restatement
of the per-nonzero tensors fed to the existing kCPU multi-head SDDMM / SpMM and against the new kCPU
entries, bit for bit (gatv2_cases.py): every LG x L configuration of the forward's fast path, the
general path, every LPR and a second column tile of the gradient, the boundary row lengths under
every schedule, repeated columns, columns outside [0, K), unaligned bases, row ranges, the
activation's edges, special values, the public API, autograd, the op layer, the argument checks
and graph capture."""
from __future__ import annotations

import pytest

import gatv2_cases as gc
from helpers import DTYPES

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("h,d,dt", gc.fwd_cases(gc.FAST_HD))
def test_scores_fast_path_shapes(device, h, d, dt):
    gc.check_forward(device, h, d, dt)


@pytest.mark.parametrize("h,d,dt", gc.fwd_cases(gc.GENERAL_HD))
def test_scores_general_path_shapes(device, h, d, dt):
    gc.check_forward(device, h, d, dt)


@pytest.mark.parametrize("h,d,dt", [(8, 8, "f32"), (3, 5, "bf16")])
def test_scores_int64_indices(device, h, d, dt):
    gc.check_forward(device, h, d, dt, "i64")


@pytest.mark.parametrize("h,d,dt", [(h, d, dt) for dt, hds in gc.GRAD_HD.items() for h, d in hds])
def test_gradient_widths(device, h, d, dt):
    gc.check_grad(device, h, d, dt, lengths=None if h * d <= 128 else tuple(gc.SHORT))


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
@pytest.mark.parametrize("h,d", gc.GRAD_GENERAL_HD)
def test_gradient_general_path(device, h, d, dt):
    gc.check_grad(device, h, d, dt)


@pytest.mark.parametrize("h,d,dt", [(4, 16, "f32"), (3, 5, "bf16")])
def test_gradient_int64_indices(device, h, d, dt):
    gc.check_grad(device, h, d, dt, "i64", schedules=("default", "split8"))


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_scores_against_tree_sum(device, dt):
    gc.check_tree_sum(device, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_identity_activation_is_the_sddmm(device, dt):
    gc.check_sddmm_identity(device, dt)


@pytest.mark.parametrize("h,d,dt", [(4, 16, "f32"), (3, 5, "f32"), (8, 8, "bf16"), (2, 8, "f64")])
def test_row_ranges(device, h, d, dt):
    gc.check_row_ranges(device, h, d, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_columns_out_of_range(device, dt):
    gc.check_columns_out_of_range(device, dt)


@pytest.mark.parametrize("slope", gc.SLOPES)
@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_activation_edges(device, dt, slope):
    gc.check_activation_edges(device, DTYPES[dt], slope)


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_special_values_stay_in_their_head_and_row(device, dt):
    gc.check_special_confined(device, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_degenerate_sizes(device, dt):
    gc.check_degenerate(device, dt)


def test_argument_checks(device):
    gc.check_argument_checks(device)


def test_op_layer(device):
    gc.check_op_layer(device)


def test_public_api(device):
    gc.check_public_api(device)


@pytest.mark.parametrize("h,d,dt", [(3, 5, "f32"), (8, 8, "f32"), (4, 8, "bf16"), (2, 4, "f64"),
                                    (1, 16, "f16")])
def test_gradients_match_the_reference_chain(device, h, d, dt):
    gc.check_grads(device, h, d, dt)


def test_needs_input_grad(device, monkeypatch):
    gc.check_needs_input_grad(device, monkeypatch)


def test_gradcheck(device):
    gc.check_gradcheck(device)


def test_gatv2_attention_dense_reference_f32(device):
    gc.check_dense_reference_f32(device)


@pytest.mark.graph_capture
@pytest.mark.parametrize("h,d", [(8, 16), (3, 5)])
def test_graph_capture(device, h, d):
    """The forward and both gradient launches (on A with p, on the transpose without) captured
    into one graph and replayed on new inputs: the same bits as fresh eager launches and as the
    kCPU entries.  (8, 16) takes the fast paths, (3, 5) the general ones."""
    gc.check_graph_capture(h, d, "f32")

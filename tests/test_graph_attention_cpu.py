"""Fused multi-head graph attention (op "graph_attention_csr_heads", `oneflow_spmm.graph_attention`)
on host tensors: the kCPU entry against the composition of the three C-ABI entries, bit for bit;
the public API, the op layer, autograd against the composed layer's, the C-ABI's argument checks,
and the kCPU entry under the host sanitizers (graph_attention_cases.py)."""
from __future__ import annotations

import os
import subprocess

import pytest

import graph_attention_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


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
    exe = tmp_path / "graph_attention_sanitize"
    csrc = os.path.join(ROOT, "of-spmm_amd", "csrc")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fopenmp",
                    "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    "-Wno-duplicate-decl-specifier", "-Wno-unused-function",
                    "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(ROOT, "tests", "native", "graph_attention_sanitize.cpp"),
                    os.path.join(csrc, "graph_attention_heads_cpu.cpp"),
                    os.path.join(csrc, "spmm_heads_cpu.cpp"),
                    os.path.join(csrc, "edge_softmax_cpu.cpp"), os.path.join(csrc, "errors.cpp"),
                    "-o", str(exe)], check=True)
    supp = tmp_path / "lsan.supp"
    supp.write_text("leak:___kmp_allocate\n")  # the OpenMP runtime's own thread-pool state
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               LSAN_OPTIONS=f"suppressions={supp}", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("OK") and "runtime error" not in r.stderr, r.stdout + r.stderr

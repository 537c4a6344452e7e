"""CPU: the configuration every forward launch of a grid of (dtype, index type, shape, width, view,
variant, row range) takes, through ofx_spmm_csr_describe, against the recorded choices of
tests/fixtures/forward_config_grid.json (written by scripts/make_forward_config_grid.py from the
library before the launch rules were rearranged: of-spmm_amd/csrc/spmm_launch.h launch_form,
spmm_forward_rules.h launch_typed).  The comparison is exact: the whole describe string, the
workspace size included, or the error text of a call that fails.  Nothing is launched."""
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "of-spmm_amd"))

from oneflow_spmm import _lib, ops  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "fixtures", "forward_config_grid.json")

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}
ELEM = {"f32": 4, "bf16": 2, "f16": 2, "f64": 8}
INDEX = {"i32": torch.int32, "i64": torch.int64}
# both sides of kSmallRows, kSmallFormNnz, kMidFormElems (at N = 128) and kPrefetchNnz, and the
# graphs the rules were measured on (Cora, PubMed, 20k x 400k, arxiv, 1M power-law, products, papers)
SHAPES = [(2708, 10556), (19717, 88648), (20000, 400000), (32768, 131072), (32769, 131072),
          (32768, 131073), (32768, (1 << 28) // 128), (32768, (1 << 28) // 128 + 1),
          (169343, 1166243), (120000, 3 << 20), (120000, (3 << 20) + 1), (1000000, 20000000),
          (2449029, 123718280), (111059956, 1615685872)]
WIDTHS = [1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 24, 31, 32, 33, 41, 47, 48, 63, 64, 65, 99, 100,
          127, 128, 129, 200, 255, 256, 257, 301, 512]
VARIANTS = [30000, 30001, 30002, 30003, 30004, 30005, 30006, 116, 416, 164, 232, 864]
VARIANT_SHAPES = [(19717, 88648), (169343, 1166243), (1000000, 20000000)]
VARIANT_WIDTHS = [8, 16, 41, 64, 128]
RANGE_SHAPES = [(169343, 1166243), (2449029, 123718280)]
RANGE_WIDTHS = [16, 64, 128]
RANGE_NNZ = [0, 100000, 2000000, 10**12]


def cases():
    """Every case, in generation order: (dtype, index type, m, nnz, n, odd view, variant, row_end
    (0: all rows), range_nnz, planned)."""
    out = []
    for dt in DTYPES:
        for idx in INDEX:
            for m, nnz in SHAPES:
                for n in WIDTHS:
                    for odd in (0, 1):
                        out.append((dt, idx, m, nnz, n, odd, 0, 0, 0, 0))
    for dt in DTYPES:
        for idx in INDEX:
            for variant in VARIANTS:
                for m, nnz in VARIANT_SHAPES:
                    for n in VARIANT_WIDTHS:
                        out.append((dt, idx, m, nnz, n, 0, variant, 0, 0, 0))
    for dt in DTYPES:
        for idx in INDEX:
            for m, nnz in RANGE_SHAPES:
                for n in RANGE_WIDTHS:
                    for row_end in (m // 8, 30000):
                        for range_nnz in RANGE_NNZ:
                            for planned in (0, 1):
                                out.append((dt, idx, m, nnz, n, 0, 0, row_end, range_nnz, planned))
    return out


def describe(case):
    """The describe string of one case, or "error: <text>" for a call that fails."""
    dt, idx, m, nnz, n, odd, variant, row_end, range_nnz, planned = case
    e = ELEM[dt]
    # the element-aligned odd view: offsets of 1 and 3 elements, strides of n + 3 and n + 1
    b_addr, c_addr, ldb, ldc = (256 + e, 256 + 3 * e, n + 3, n + 1) if odd else (256, 256, n, n)
    opts = ops.make_options(variant=variant, range_nnz=range_nnz, planned=bool(planned))
    buf = ctypes.create_string_buffer(512)
    rc = _lib.LIB.ofx_spmm_csr_describe(ops.dtype_code(INDEX[idx]), ops.dtype_code(DTYPES[dt]), m,
                                        m, n, nnz, b_addr, ldb, c_addr, ldc, 0, row_end or m,
                                        ctypes.byref(opts), buf, len(buf))
    if rc != 0:
        return "error: " + _lib.last_error()
    return buf.value.decode()


def split_ws(text):
    """(the string without its workspace size, the size); errors carry no size (-1)."""
    head, sep, ws = text.rpartition(" ws=")
    return (head, int(ws)) if sep and not text.startswith("error: ") else (text, -1)


def test_forward_config_grid():
    with open(FIXTURE) as f:
        recorded = json.load(f)
    strings, choices = recorded["strings"], recorded["cases"]
    grid = cases()
    assert len(choices) == len(grid), (len(choices), len(grid))
    wrong = []
    for case, (index, ws) in zip(grid, choices):
        got = split_ws(describe(case))
        if got != (strings[index], ws):
            wrong.append((case, got, (strings[index], ws)))
    assert not wrong, f"{len(wrong)} of {len(grid)} cases differ; first: {wrong[0]}"

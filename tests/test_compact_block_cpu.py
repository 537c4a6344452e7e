"""Block compaction: the kCPU kernel behind `compact_block` against `np.unique` and
`np.searchsorted` over the case table of tests/compact_block_cases.py, its errors, the size checks
of the device entries (which launch nothing) and `sample_blocks` against the torch route."""
import ctypes

import pytest
import torch

import oneflow_spmm as fs
from oneflow_spmm import _lib
from tests import compact_block_cases as cases
from tests import sample_neighbors_cases as graphs

IDX = cases.IDX


@pytest.mark.parametrize("idx", list(IDX))
@pytest.mark.parametrize("name", cases.CASES)
def test_cpu_equals_numpy(name, idx):
    it = IDX[idx]
    n, seeds, cols, ref = cases.case(name)
    got = fs.compact_block(cases.tensor(seeds, it), cases.tensor(cols, it), n)
    cases.assert_block(got, ref, it, "cpu")
    if name.startswith("full"):
        assert got[0].numel() == n


@pytest.mark.parametrize("idx", list(IDX))
@pytest.mark.parametrize("name", ["boundary-65541", "hub", "sparse"])
def test_thread_count_does_not_change_the_arrays(name, idx):
    it = IDX[idx]
    n, seeds, cols, ref = cases.case(name)
    for nt in (1, 16):
        got = fs.compact_block(cases.tensor(seeds, it), cases.tensor(cols, it), n, num_threads=nt)
        cases.assert_block(got, ref, it, "cpu")


@pytest.mark.parametrize("idx", list(IDX))
def test_bad_ids_are_refused_and_the_next_call_is_right(idx):
    it = IDX[idx]
    n, seeds, cols, ref = cases.case("seeds-overlapping")
    for bad in (-1, n, 2 ** 31 - 1) + ((2 ** 40,) if it == torch.int64 else ()):
        for where in (seeds, cols):
            spoiled = [seeds.copy(), cols.copy()]
            spoiled[where is cols][17] = bad
            with pytest.raises(fs.OfxError, match="outside") as e:
                fs.compact_block(cases.tensor(spoiled[0], it), cases.tensor(spoiled[1], it), n)
            assert e.value.code == _lib.OFX_EINVAL
    cases.assert_block(fs.compact_block(cases.tensor(seeds, it), cases.tensor(cols, it), n), ref, it, "cpu")


@pytest.mark.parametrize("num_nodes", [2 ** 31, -1])
def test_bad_num_nodes_is_refused_before_any_launch(num_nodes):
    ids = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(fs.OfxError) as e:
        fs.compact_block(ids, ids, num_nodes)
    assert e.value.code == _lib.OFX_EINVAL
    # the device entries check the sizes first: no pointer is read, no GPU is needed
    size = ctypes.c_size_t(0)
    assert _lib.LIB.ofx_compact_ids_workspace_size(_lib.DT_INT64, num_nodes, 3, 3,
                                                   ctypes.byref(size)) == _lib.OFX_EINVAL
    assert _lib.LIB.ofx_compact_ids(None, _lib.DT_INT64, num_nodes, 3, None, 3, None, None, None,
                                    None, None, None, None, 0) == _lib.OFX_EINVAL


def test_a_misaligned_workspace_is_refused_before_any_launch():
    ids, out = torch.zeros(3, dtype=torch.int64), torch.zeros(64, dtype=torch.int64)
    p = out.data_ptr()  # every pointer is valid; none is read: the alignment check comes first
    assert p % 16 == 0
    assert _lib.LIB.ofx_compact_ids(None, _lib.DT_INT64, 5, 3, ids.data_ptr(), 3, ids.data_ptr(), p,
                                    p, p, p, None, p + 8, 504) == _lib.OFX_EWORKSPACE


def test_arguments_and_exports():
    ids = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(TypeError):
        fs.compact_block(ids, ids.to(torch.int32), 5)
    with pytest.raises(RuntimeError, match="1-D"):
        fs.compact_block(ids.view(3, 1), ids, 5)
    assert fs.compact_block is fs.sampling.compact_block and "compact_block" in fs.__all__
    assert {"ofx_compact_ids_workspace_size", "ofx_compact_ids", "ofx_compact_ids_cpu"} <= set(_lib.EXPORTED)


@pytest.mark.parametrize("idx", list(IDX))
def test_sample_blocks_equal_the_torch_route(idx):
    it = IDX[idx]
    rp, ci, seeds, _ = graphs.gpu_case(5)
    args = [cases.tensor(a, it) for a in (rp, ci, seeds)]
    cases.assert_blocks_equal(fs.sample_blocks(*args, (3, 2), seed=4),
                              cases.torch_route_blocks(*args, (3, 2), seed=4))
    # columns past the row count: compact_block refuses them, the layer takes the torch route
    wide = [cases.tensor(a, it) for a in cases.WIDE]
    with pytest.raises(RuntimeError, match="outside"):
        fs.compact_block(wide[2], wide[1], 4)
    cases.assert_blocks_equal(fs.sample_blocks(*wide, (2,)), cases.torch_route_blocks(*wide, (2,)))

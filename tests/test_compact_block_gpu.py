"""Block compaction on the GPU (csrc/compact_ids.hip): the HIP kernels against
`np.unique` / `np.searchsorted` and the kCPU kernel over the case table of
tests/compact_block_cases.py, bad ids, and `sample_blocks` against the torch route and the CPU."""
import numpy as np
import pytest
import torch

import oneflow_spmm as fs
from tests import compact_block_cases as cases
from tests import sample_neighbors_cases as graphs

pytestmark = pytest.mark.gpu

IDX = cases.IDX


@pytest.mark.parametrize("idx", list(IDX))
@pytest.mark.parametrize("name", cases.CASES)
def test_gpu_equals_numpy_and_cpu(device, name, idx):
    it = IDX[idx]
    n, seeds, cols, ref = cases.case(name)
    got = fs.compact_block(cases.tensor(seeds, it, device), cases.tensor(cols, it, device), n)
    cases.assert_block(got, ref, it, "cuda")
    cases.assert_block(got, fs.compact_block(cases.tensor(seeds, it), cases.tensor(cols, it), n), it, "cuda")
    if name.startswith("full"):
        assert got[0].numel() == n


@pytest.mark.parametrize("idx", list(IDX))
def test_bad_ids_raise_and_the_next_call_is_right(device, idx):
    it = IDX[idx]
    n, seeds, cols, ref = cases.case("seeds-overlapping")
    for bad in (-1, n, 2 ** 31 - 1) + ((2 ** 40,) if it == torch.int64 else ()):
        for where in (seeds, cols):
            spoiled = [seeds.copy(), cols.copy()]
            spoiled[where is cols][17] = bad
            with pytest.raises(RuntimeError, match="outside"):
                fs.compact_block(cases.tensor(spoiled[0], it, device), cases.tensor(spoiled[1], it, device), n)
    torch.cuda.synchronize()
    got = fs.compact_block(cases.tensor(seeds, it, device), cases.tensor(cols, it, device), n)
    cases.assert_block(got, ref, it, "cuda")


@pytest.mark.parametrize("idx", list(IDX))
def test_sample_blocks_equal_the_torch_route_and_the_cpu(device, idx):
    it = IDX[idx]
    rp, ci, seeds, _ = graphs.gpu_case(5)
    host = [cases.tensor(a, it) for a in (rp, ci, seeds)]
    dev = [a.to(device) for a in host]
    blocks = fs.sample_blocks(*dev, (3, 2), seed=4)
    assert all(x.device.type == "cuda" for b in blocks for x in b)
    cases.assert_blocks_equal(blocks, cases.torch_route_blocks(*dev, (3, 2), seed=4))
    cpu_blocks = fs.sample_blocks(*host, (3, 2), seed=4)
    cases.assert_blocks_equal(blocks, cpu_blocks)

    # one mean layer over the input block: the GPU's block and the CPU's give the same bits
    def layer(block):
        rp_s, col_local, eid, src, seed_pos = (x.to(device) for x in block)
        gen = np.random.default_rng(6)
        vals = torch.from_numpy(gen.uniform(0.5, 1.5, eid.numel()).astype(np.float32)).to(device)
        h = torch.from_numpy(gen.uniform(-1, 1, (src.numel(), 8)).astype(np.float32)).to(device)
        return fs.spmm(rp_s, col_local, vals, seed_pos.numel(), src.numel(), h, reduce="mean")

    assert torch.equal(layer(blocks[0]).view(torch.int32), layer(cpu_blocks[0]).view(torch.int32))
    # columns past the row count: the layer takes the torch route
    wide = [cases.tensor(a, it, device) for a in cases.WIDE]
    cases.assert_blocks_equal(fs.sample_blocks(*wide, (2,)), cases.torch_route_blocks(*wide, (2,)))

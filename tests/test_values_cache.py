"""The transpose cache's values policy (autograd._TransposeCache.transposed_values), which
grad_b ([nnz] values) and grad_b_heads ([nnz, H] values) share: what `seen` and `value_entries`
hold after each sighting of unchanged values, that an in-place update starts over, the bound on
both dicts, and the capture rule (a copy gathered while the stream captures is never stored).
The policy is under test, not a kernel: a 5-row CSR with empty rows, K = 4."""
from __future__ import annotations

import pytest
import torch

import oneflow_spmm as fs
from oneflow_spmm import _C
from oneflow_spmm.autograd import TRANSPOSE_CACHE as CACHE

M, K, N, H, D = 5, 4, 8, 2, 4
LENGTHS = [0, 3, 1, 0, 2]
COLS = [0, 1, 3, 2, 1, 3]


def csr(dev="cpu"):
    """A fresh CSR (its own storage, so its own cache keys) and its transpose's (rp, ci, perm)."""
    rp = torch.tensor([0] + LENGTHS, dtype=torch.int32).cumsum(0).to(torch.int32).to(dev)
    ci = torch.tensor(COLS, dtype=torch.int32, device=dev)
    return rp, ci, fs.csr_transpose(rp, ci, K)


def rand(*shape, seed=0, dev="cpu"):
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) - 0.5).to(dev)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                              b.contiguous().view(torch.int32))


def grad_b(rank, rp, ci, values, x):
    if rank == 1:
        return CACHE.grad_b(rp, ci, values, M, K, x)
    return CACHE.grad_b_heads(rp, ci, values, M, K, x)


def plain(rank, at, values, x):
    """The plain op on A^T with values[perm], gathered here."""
    rp_t, ci_t, perm = at
    op = fs.spmm_csr if rank == 1 else _C.spmm_csr_heads
    return op(rp_t, ci_t, values[perm.long()], K, M, x)


@pytest.mark.parametrize("rank", [1, 2])
def test_cpu_sightings(rank):
    """[nnz] on the CPU: cached at the first sight.  [nnz, H]: a sighting mark first, the copy at
    the second sight, a hit at the third.  values.mul_(2) makes the next call a first sight."""
    rp, ci, at = csr()
    values = rand(6, seed=1) if rank == 1 else rand(6, H, seed=1)
    x = rand(M, N, seed=2)
    key = lambda: CACHE._values_key(rp, ci, K, values)  # noqa: E731
    want_first = {1: (False, True), 2: (True, False)}[rank]  # (in seen, in value_entries)
    for round_ in range(2):
        k0 = key()
        assert k0 not in CACHE.seen and k0 not in CACHE.value_entries, "a first sight"
        want = plain(rank, at, values, x)
        assert same_bits(grad_b(rank, rp, ci, values, x), want), "call 1"
        assert (k0 in CACHE.seen, k0 in CACHE.value_entries) == want_first
        assert same_bits(grad_b(rank, rp, ci, values, x), want), "call 2"
        assert k0 in CACHE.value_entries and (k0 in CACHE.seen) == (rank == 2)
        kept = CACHE.value_entries[k0][1]
        assert same_bits(kept, values[at[2].long()])
        assert same_bits(grad_b(rank, rp, ci, values, x), want), "call 3"
        assert CACHE.value_entries[k0][1] is kept, "call 3 is a hit"
        values.mul_(2)
        assert key() != k0, f"round {round_}: an in-place update changes the key"


@pytest.mark.parametrize("rank", [1, 2])
def test_cpu_dicts_stay_bounded(rank):
    rp, ci, at = csr()
    x = rand(M, N, seed=3)
    alive = []  # the tensors stay alive: distinct storage, distinct keys
    for i in range(CACHE.capacity + 2):
        values = rand(6, seed=10 + i) if rank == 1 else rand(6, H, seed=10 + i)
        alive.append(values)
        for _ in range(2):
            assert same_bits(grad_b(rank, rp, ci, values, x), plain(rank, at, values, x))
            assert len(CACHE.seen) <= CACHE.capacity
            assert len(CACHE.value_entries) <= CACHE.capacity
    assert len(CACHE.value_entries) == CACHE.capacity


@pytest.mark.gpu
@pytest.mark.graph_capture
@pytest.mark.parametrize("rank", [1, 2])
def test_gpu_capture_stores_no_gathered_copy(device, rank):
    """An eager warm step (first sight), then the same step captured (second sight: the copy is
    gathered inside the capture, so it lives in the graph's pool): value_entries is left as it
    was, and the replay on new numbers is the eager step."""
    rp, ci, _ = csr(device)
    values = (rand(6, seed=1) if rank == 1 else rand(6, H, seed=1)).to(device).requires_grad_(True)
    b = (rand(K, N, seed=2) if rank == 1 else rand(K, H, D, seed=2)).to(device).requires_grad_(True)
    w = (rand(M, N, seed=3) if rank == 1 else rand(M, H, D, seed=3)).to(device)

    def step():
        out = fs.spmm(rp, ci, values, M, K, b)
        gv, gb = torch.autograd.grad((out * w).sum(), (values, b))
        return out.detach(), gv, gb

    s = torch.cuda.Stream(device)
    s.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(s):
        step()  # warm (outside capture): the transpose, the first sight, the allocator
    torch.cuda.current_stream(device).wait_stream(s)
    key = CACHE._values_key(rp, ci, K, values)
    assert key in CACHE.seen and key not in CACHE.value_entries
    before = list(CACHE.value_entries.items())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = step()
    after = list(CACHE.value_entries.items())
    assert len(after) == len(before)
    assert all(ka == kb and va[1] is vb[1] for (ka, va), (kb, vb) in zip(after, before)), \
        "a tensor created inside the capture was cached"
    with torch.no_grad():
        values.copy_(rand(*values.shape, seed=4).to(device))
        b.copy_(rand(*b.shape, seed=5).to(device))
    g.replay()
    torch.cuda.synchronize()
    want = step()
    torch.cuda.synchronize()
    for name, x, y in zip(("out", "d(values)", "d(b)"), got, want):
        assert same_bits(x, y), f"graph replay {name}"

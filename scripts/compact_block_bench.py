#!/usr/bin/env python3
"""Times the block compaction (`compact_block`, csrc/compact_ids.hip) on the bench's
products-shaped synthetic CSR (oneflow_spmm.synth, int32: 2,449,029 rows, 123,718,280 nonzeros)
with 1,000,000 distinct seeds.  Per fanout in 5, 10, 15, 25 the pair (seeds, col_idx_s) that
`sample_neighbors` returns is compacted by:

  * "call":    `compact_block` on the GPU as a user calls it: the allocations, the launches and the
               one read-back of the count and the flag;
  * "device":  the C-ABI entry alone on preallocated buffers (HIP events, no read-back);
  * "torch":   what `sample_blocks` did before: `unique(cat(...))` and two `searchsorted`;
  * "cpu":     the same call on CPU tensors, the kCPU kernel at 16 threads (wall clock).

Also: a two-layer `sample_blocks(..., (10, 10))` on 100,000 seeds against the same loop with the
torch route, and the fixed cost at num_nodes = 111,059,956 (papers100M) with 10,240 ids.

The GPU arrays are checked against the kCPU kernel's (and the torch route's) before anything is
timed.  Protocol (scripts/sample_neighbors_bench.py): HIP events around each call, 3 warm-up
rounds, median (and minimum) of --reps runs, the GPU candidates alternating round by round in one
process.  Results: one JSON line, and profiles/compact_block_bench.json."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "of-spmm_amd"), ROOT, os.path.join(ROOT, "scripts")]

FANOUTS = (5, 10, 15, 25)
NUM_SEEDS = 1_000_000
BLOCK_SEEDS = 100_000
PAPERS_NODES, PAPERS_IDS = 111_059_956, 10_240
CPU_THREADS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=5)
    ap.add_argument("--scale", type=int, default=1, help="divide the problem's sizes (rehearsal)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact_block_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import oneflow_spmm as flow_spmm
    from heads_bench import timed
    from oneflow_spmm import _C, _lib, synth
    cfg = synth.CONFIGS["products"]
    m, nnz, s = cfg["m"] // args.scale, cfg["nnz"] // args.scale, NUM_SEEDS // args.scale
    dev = torch.device("cuda", 0)
    rp_h = synth.row_ptr(m, m, nnz)
    ci_h = torch.from_numpy(synth.columns(m, m, rp_h, threads=CPU_THREADS)).to(torch.int32)
    rp_h = torch.from_numpy(rp_h).to(torch.int32)
    perm = np.random.default_rng(0).permutation(m)
    rp, ci, seeds = rp_h.to(dev), ci_h.to(dev), torch.from_numpy(perm[:s].astype(np.int32)).to(dev)
    idt = _C.dtype_code(torch.int32)

    def torch_route(cur, cols):
        src = torch.unique(torch.cat((cur, cols)))
        return src, torch.searchsorted(src, cols).to(cols.dtype), torch.searchsorted(src, cur)

    def record(t, ratios):
        return {"timings": {k: {"median_ms": round(v[0], 4), "min_ms": round(v[1], 4)}
                            for k, v in t.items()},
                "ratios": {f"{a}_over_{b}": round(t[a][0] / t[b][0], 3) for a, b in ratios}}

    def device_entry(num_nodes, cur, cols):
        """The C-ABI entry on buffers allocated once; returns (callable, buffers)."""
        n = cur.numel() + cols.numel()
        ws_bytes = ctypes.c_size_t(0)
        _lib.check(_lib.LIB.ofx_compact_ids_workspace_size(idt, num_nodes, cur.numel(), cols.numel(),
                                                           ctypes.byref(ws_bytes)))
        ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8, device=dev)
        src = torch.empty(min(n, num_nodes), dtype=torch.int32, device=dev)
        col_local = torch.empty(cols.numel(), dtype=torch.int32, device=dev)
        seed_pos = torch.empty(cur.numel(), dtype=torch.int64, device=dev)
        scalars = torch.zeros(2, dtype=torch.int64, device=dev)

        def run():
            _lib.check(_lib.LIB.ofx_compact_ids(
                _C.current_stream_handle(cur), idt, num_nodes, cur.numel(), cur.data_ptr(),
                cols.numel(), cols.data_ptr(), src.data_ptr(), seed_pos.data_ptr(),
                col_local.data_ptr(), scalars.data_ptr(), scalars.data_ptr() + 8, ws.data_ptr(),
                ws_bytes.value))
        return run, (src, col_local, seed_pos, scalars), ws_bytes.value

    rows = []
    for fanout in FANOUTS:
        cols = flow_spmm.sample_neighbors(rp, ci, seeds, fanout, seed=1, return_edge_ids=False)[1]
        seeds_h, cols_h = seeds.cpu(), cols.cpu()
        got = flow_spmm.compact_block(seeds, cols, m)
        ref = flow_spmm.compact_block(seeds_h, cols_h, m, num_threads=CPU_THREADS)
        assert all(torch.equal(g.cpu(), r) for g, r in zip(got, ref)), "GPU != kCPU"
        assert all(torch.equal(g, r) for g, r in zip(got, torch_route(seeds, cols))), "GPU != torch"
        device, (src, col_local, seed_pos, scalars), ws_bytes = device_entry(m, seeds, cols)
        device()
        count = got[0].numel()
        assert scalars.tolist() == [count, 0] and torch.equal(src[:count], got[0])
        assert torch.equal(col_local, got[1]) and torch.equal(seed_pos, got[2])
        t = timed({"call": lambda: flow_spmm.compact_block(seeds, cols, m), "device": device,
                   "torch": lambda: torch_route(seeds, cols)}, args.reps)
        cpu = []
        for _ in range(args.cpu_reps):
            t0 = time.perf_counter()
            flow_spmm.compact_block(seeds_h, cols_h, m, num_threads=CPU_THREADS)
            cpu.append((time.perf_counter() - t0) * 1e3)
        t["cpu"] = (float(np.median(cpu)), float(np.min(cpu)))
        rows.append({"fanout": fanout, "ids": s + cols.numel(), "distinct": count,
                     "workspace_bytes": ws_bytes,
                     **record(t, (("call", "torch"), ("device", "torch"), ("cpu", "call")))})
        del got, ref, src, col_local, seed_pos, device

    # two layers of blocks, with compact_block and with the torch route
    bseeds = torch.from_numpy(perm[:BLOCK_SEEDS // args.scale].astype(np.int32)).to(dev)

    def blocks_torch():
        out, cur = [], bseeds
        for layer in (1, 0):
            rp_s, ci_s, eid = flow_spmm.sample_neighbors(rp, ci, cur, 10, seed=layer)
            src, col_local, seed_pos = torch_route(cur, ci_s)
            out.append((rp_s, col_local, eid, src, seed_pos))
            cur = src
        return out[::-1]

    new, old = flow_spmm.sample_blocks(rp, ci, bseeds, (10, 10)), blocks_torch()
    assert all(torch.equal(x, y) for b, w in zip(new, old) for x, y in zip(b, w)), "blocks differ"
    tb = timed({"sample_blocks": lambda: flow_spmm.sample_blocks(rp, ci, bseeds, (10, 10)),
                "sample_blocks_torch": blocks_torch}, args.reps)
    blocks = {"seeds": bseeds.numel(), "fanouts": [10, 10], "src": [b[3].numel() for b in new],
              **record(tb, (("sample_blocks", "sample_blocks_torch"),))}
    del new, old

    # the fixed cost: a papers100M-sized id space, a small batch
    big = PAPERS_NODES // args.scale
    ids = torch.from_numpy(np.random.default_rng(1).integers(0, big, PAPERS_IDS).astype(np.int32)).to(dev)
    a, b = ids[:1024].contiguous(), ids[1024:].contiguous()
    assert all(torch.equal(g, r) for g, r in zip(flow_spmm.compact_block(a, b, big), torch_route(a, b)))
    device, _, ws_bytes = device_entry(big, a, b)
    tf = timed({"call": lambda: flow_spmm.compact_block(a, b, big), "device": device,
                "torch": lambda: torch_route(a, b)}, args.reps)
    fixed = {"num_nodes": big, "ids": ids.numel(), "workspace_bytes": ws_bytes,
             **record(tf, (("call", "torch"), ("device", "torch")))}

    res = {"graph": "products", "device": torch.cuda.get_device_name(0), "m": m, "nnz": nnz,
           "num_seeds": s, "idx": "int32", "reps": args.reps, "cpu_threads": CPU_THREADS,
           "fanouts": rows, "blocks": blocks, "fixed_cost": fixed,
           "call_below_torch_at_every_fanout": all(r["ratios"]["call_over_torch"] < 1 for r in rows)}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

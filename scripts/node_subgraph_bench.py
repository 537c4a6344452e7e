#!/usr/bin/env python3
"""Times the induced-subgraph extraction (`node_subgraph`, csrc/node_subgraph.hip) on the bench's
products-shaped synthetic CSR (oneflow_spmm.synth, int32: 2,449,029 rows, 123,718,280 nonzeros)
over three node sets: 100,000 uniformly random nodes (GraphSAINT-like), a contiguous range of M/15
nodes (ClusterGCN-like) and all M nodes.  Per node set:

  * "call":    `node_subgraph` on the GPU as a user calls it: the allocations, the launches of the
               count entry, the one read-back of (C, nnz_s, flag), the fill entry;
  * "device":  the two C-ABI entries on preallocated buffers, the sizes known (no read-back);
  * "torch":   the route a user builds today, written out below: mask, `nonzero`,
               `repeat_interleave`, gather, mask lookup, `nonzero`, `cumsum`, `bincount`, giving the
               same five arrays;
  * "cpu":     the same call on CPU tensors, the kCPU kernel at 16 threads (wall clock).

Also the fixed cost at papers100M scale: M = 111,059,956 rows of 14 entries (an edge bitmap over
1.55e9 entries) for 10,240 nodes.

The GPU arrays are checked against the kCPU kernel's and the torch route's before anything is
timed.  Protocol (scripts/compact_block_bench.py): HIP events around each call, 3 warm-up rounds,
median (and minimum) of --reps runs, the GPU candidates alternating round by round in one process.
Results: one JSON line, and profiles/node_subgraph_bench.json."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "of-spmm_amd"), ROOT, os.path.join(ROOT, "scripts")]

RANDOM_NODES = 100_000
PAPERS_NODES, PAPERS_DEGREE, PAPERS_IDS = 111_059_956, 14, 10_240
CPU_THREADS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--scale", type=int, default=1, help="divide the problem's sizes (rehearsal)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "node_subgraph_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import oneflow_spmm as flow_spmm
    from heads_bench import timed
    from oneflow_spmm import _C, _lib, synth
    cfg = synth.CONFIGS["products"]
    m, nnz = cfg["m"] // args.scale, cfg["nnz"] // args.scale
    dev = torch.device("cuda", 0)
    it = torch.int32
    idt = _C.dtype_code(it)
    rp_h = synth.row_ptr(m, m, nnz)
    ci_h = torch.from_numpy(synth.columns(m, m, rp_h, threads=CPU_THREADS)).to(it)
    rp_h = torch.from_numpy(rp_h).to(it)
    rp, ci = rp_h.to(dev), ci_h.to(dev)
    perm = np.random.default_rng(0).permutation(m)
    node_sets = {"random": perm[:RANDOM_NODES // args.scale], "range": m // 3 + np.arange(m // 15),
                 "all": np.arange(m)}

    def torch_route(rp, ci, nodes):
        n = rp.numel() - 1
        mask = torch.zeros(n, dtype=torch.bool, device=rp.device)
        mask[nodes.long()] = True
        src = mask.nonzero().squeeze(1)
        new_id = torch.cumsum(mask, 0) - 1
        lo = rp[src].long()
        deg = rp[src + 1].long() - lo
        row_of = torch.repeat_interleave(torch.arange(src.numel(), device=rp.device), deg)
        start = torch.cumsum(deg, 0) - deg
        j = lo[row_of] + (torch.arange(row_of.numel(), device=rp.device) - start[row_of])
        cols = ci[j].long()  # a square CSR: every column is a node
        sel = mask[cols].nonzero().squeeze(1)
        counts = torch.bincount(row_of[sel], minlength=src.numel())
        rp_s = torch.cat((counts.new_zeros(1), torch.cumsum(counts, 0)))
        return (src.to(ci.dtype), rp_s.to(ci.dtype), new_id[cols[sel]].to(ci.dtype),
                j[sel].to(ci.dtype), new_id[nodes.long()])

    def record(t, ratios):
        return {"timings": {k: {"median_ms": round(v[0], 4), "min_ms": round(v[1], 4)}
                            for k, v in t.items()},
                "ratios": {f"{a}_over_{b}": round(t[a][0] / t[b][0], 3) for a, b in ratios}}

    def device_entries(rp, ci, nodes, count, nnz_s):
        """Both C-ABI entries on buffers allocated once, the sizes given; (callable, buffers)."""
        n, e, s = rp.numel() - 1, ci.numel(), nodes.numel()
        ws_bytes = ctypes.c_size_t(0)
        _lib.check(_lib.LIB.ofx_node_subgraph_workspace_size(idt, n, e, s, ctypes.byref(ws_bytes)))
        ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8, device=dev)
        new = lambda k: torch.empty(k, dtype=it, device=dev)  # noqa: E731
        src, rp_s, col_local, eid = new(min(s, n)), new(count + 1), new(nnz_s), new(nnz_s)
        node_pos = torch.empty(s, dtype=torch.int64, device=dev)
        scalars = torch.zeros(3, dtype=torch.int64, device=dev)

        def run():
            stream = _C.current_stream_handle(rp)
            _lib.check(_lib.LIB.ofx_node_subgraph_count(
                stream, idt, n, e, s, rp.data_ptr(), ci.data_ptr(), nodes.data_ptr(), src.data_ptr(),
                node_pos.data_ptr(), scalars.data_ptr(), scalars.data_ptr() + 16, ws.data_ptr(),
                ws_bytes.value))
            _lib.check(_lib.LIB.ofx_node_subgraph_fill(
                stream, idt, n, e, s, count, nnz_s, rp.data_ptr(), ci.data_ptr(), src.data_ptr(),
                rp_s.data_ptr(), col_local.data_ptr(), eid.data_ptr(), ws.data_ptr(), ws_bytes.value))
        return run, (src[:count], rp_s, col_local, eid, node_pos), scalars, ws_bytes.value

    def same(got, want):
        return all(g.dtype == w.dtype and torch.equal(g.cpu(), w.cpu()) for g, w in zip(got, want))

    rows = []
    for name, ids in node_sets.items():
        nodes_h = torch.from_numpy(ids.astype(np.int32))
        nodes = nodes_h.to(dev)
        got = flow_spmm.node_subgraph(rp, ci, nodes)
        assert same(got, flow_spmm.node_subgraph(rp_h, ci_h, nodes_h, num_threads=CPU_THREADS)), "GPU != kCPU"
        assert same(got, torch_route(rp, ci, nodes)), "GPU != torch"
        count, nnz_s = got[0].numel(), got[2].numel()
        device, bufs, scalars, ws_bytes = device_entries(rp, ci, nodes, count, nnz_s)
        device()
        assert scalars.tolist() == [count, nnz_s, 0] and same(bufs, got), "device entries != call"
        t = timed({"call": lambda: flow_spmm.node_subgraph(rp, ci, nodes), "device": device,
                   "torch": lambda: torch_route(rp, ci, nodes)}, args.reps)
        cpu = []
        for _ in range(args.cpu_reps):
            t0 = time.perf_counter()
            flow_spmm.node_subgraph(rp_h, ci_h, nodes_h, num_threads=CPU_THREADS)
            cpu.append((time.perf_counter() - t0) * 1e3)
        t["cpu"] = (float(np.median(cpu)), float(np.min(cpu)))
        rows.append({"nodes": name, "selected": count, "entries_of_selected_rows":
                     int((rp_h[ids + 1].long() - rp_h[ids].long()).sum()), "kept": nnz_s,
                     "workspace_bytes": ws_bytes,
                     **record(t, (("call", "torch"), ("device", "torch"), ("cpu", "call")))})
        del got, bufs, device
    del rp, ci
    torch.cuda.empty_cache()

    # the fixed cost: a papers100M-sized node range and edge bitmap, a small batch
    big = PAPERS_NODES // args.scale
    rp_b = (torch.arange(big + 1, device=dev, dtype=torch.int64) * PAPERS_DEGREE).to(it)
    ci_b = torch.randint(0, big, (big * PAPERS_DEGREE,), device=dev, dtype=it,
                         generator=torch.Generator(device=dev).manual_seed(1))
    ids = torch.from_numpy(np.random.default_rng(1).integers(0, big, PAPERS_IDS).astype(np.int32)).to(dev)
    got = flow_spmm.node_subgraph(rp_b, ci_b, ids)
    assert same(got, torch_route(rp_b, ci_b, ids)), "GPU != torch at the papers100M scale"
    device, _, _, ws_bytes = device_entries(rp_b, ci_b, ids, got[0].numel(), got[2].numel())
    tf = timed({"call": lambda: flow_spmm.node_subgraph(rp_b, ci_b, ids), "device": device,
                "torch": lambda: torch_route(rp_b, ci_b, ids)}, args.reps)
    fixed = {"m": big, "nnz": ci_b.numel(), "nodes": ids.numel(), "selected": got[0].numel(),
             "kept": got[2].numel(), "workspace_bytes": ws_bytes,
             **record(tf, (("call", "torch"), ("device", "torch")))}

    res = {"graph": "products", "device": torch.cuda.get_device_name(0), "m": m, "nnz": nnz,
           "idx": "int32", "reps": args.reps, "cpu_threads": CPU_THREADS, "node_sets": rows,
           "fixed_cost": fixed,
           "call_below_torch_on_every_node_set": all(r["ratios"]["call_over_torch"] < 1 for r in rows)}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

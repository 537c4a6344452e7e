#!/usr/bin/env python3
"""Times the random walks (`random_walk`, csrc/random_walk.hip) on the bench's products-shaped
synthetic CSR (oneflow_spmm.synth, int32: 2,449,029 rows, 123,718,280 nonzeros) from 1,000,000
starts.

First order (p = q = 1), length 4, 40 and 80:
  * "call":    `random_walk` on the GPU as a user calls it: the allocation, the launch and the one
               read-back of the flag;
  * "device":  the C-ABI entry alone on preallocated buffers (HIP events, no read-back);
  * "torch":   the loop a user wrote before: per step a degree, `torch.rand`, a multiply, a cast,
               an add and a gather (it does not mark walks that ended, which would cost it more);
  * "cpu":     the same call on CPU tensors, the kCPU kernel at 16 threads (wall clock).
and GraphSAINT's setting, 8,000 starts of length 2: `random_walk_subgraph` against that torch loop
followed by `node_subgraph`.

Second order, length 40, (p, q) in (0.25, 4), (4, 0.25), (1, 2): "call", "device", "cpu", the ratio
to the first-order kernel on the same starts, and the mean attempts per step, counted by the Python
restatement of tests/random_walk_cases.py on every 100th start, not by the kernel.  No torch route
exists for the biased walk.

The GPU arrays are checked against the kCPU kernel's before anything is timed.  Protocol
(scripts/compact_block_bench.py): HIP events around each call, 3 warm-up rounds, median (and
minimum) of --reps runs, the GPU candidates alternating round by round in one process.  Results:
one JSON line, and profiles/random_walk_bench.json."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "of-spmm_amd"), ROOT, os.path.join(ROOT, "scripts")]

LENGTHS = (4, 40, 80)
PQ = ((0.25, 4.0), (4.0, 0.25), (1.0, 2.0))
NUM_STARTS = 1_000_000
SAINT_STARTS, SAINT_LENGTH = 8_000, 2
SECOND_LENGTH = 40
CPU_THREADS = 16
SEED = 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--scale", type=int, default=1, help="divide the problem's sizes (rehearsal)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "random_walk_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import oneflow_spmm as flow_spmm
    from heads_bench import timed
    from oneflow_spmm import _C, _lib, synth
    from tests import random_walk_cases as restatement
    cfg = synth.CONFIGS["products"]
    m, nnz, s = cfg["m"] // args.scale, cfg["nnz"] // args.scale, NUM_STARTS // args.scale
    dev = torch.device("cuda", 0)
    rp_n = synth.row_ptr(m, m, nnz)
    ci_n = synth.columns(m, m, rp_n, threads=CPU_THREADS)
    rp_h, ci_h = torch.from_numpy(rp_n).to(torch.int32), torch.from_numpy(ci_n).to(torch.int32)
    perm = np.random.default_rng(0).permutation(m)
    starts_h = torch.from_numpy(perm[:s].astype(np.int32))
    rp, ci, starts = rp_h.to(dev), ci_h.to(dev), starts_h.to(dev)
    idt = _C.dtype_code(torch.int32)

    def torch_walk(cur, length):
        cur = cur.long()
        out = [cur]
        for _ in range(length):
            lo = rp[cur]
            deg = rp[cur + 1] - lo
            e = lo + (torch.rand(cur.numel(), device=dev) * deg).long()
            cur = ci[e.clamp_(max=nnz - 1)].long()
            out.append(cur)
        return torch.stack(out, 1)

    def record(t, ratios):
        return {"timings": {k: {"median_ms": round(v[0], 4), "min_ms": round(v[1], 4)}
                            for k, v in t.items()},
                "ratios": {f"{a}_over_{b}": round(t[a][0] / t[b][0], 3) for a, b in ratios}}

    def device_entry(length, p, q):
        walks = torch.empty((s, length + 1), dtype=torch.int32, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)

        def run():
            _lib.check(_lib.LIB.ofx_random_walk(
                _C.current_stream_handle(rp), idt, m, nnz, s, rp.data_ptr(), ci.data_ptr(),
                starts.data_ptr(), length, p, q, SEED, walks.data_ptr(), None, bad.data_ptr()))
        return run, walks, bad

    def cpu_times(length, p, q):
        ts = []
        for _ in range(args.cpu_reps):
            t0 = time.perf_counter()
            flow_spmm.random_walk(rp_h, ci_h, starts_h, length, p=p, q=q, seed=SEED,
                                  num_threads=CPU_THREADS)
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), float(np.min(ts))

    def checked(length, p, q):
        """The device entry, after its arrays and the call's equalled the kCPU kernel's."""
        ref = flow_spmm.random_walk(rp_h, ci_h, starts_h, length, p=p, q=q, seed=SEED,
                                    return_edge_ids=True, num_threads=CPU_THREADS)
        got = flow_spmm.random_walk(rp, ci, starts, length, p=p, q=q, seed=SEED, return_edge_ids=True)
        assert torch.equal(got[0].cpu(), ref[0]) and torch.equal(got[1].cpu(), ref[1]), "GPU != kCPU"
        device, walks, bad = device_entry(length, p, q)
        device()
        assert torch.equal(walks.cpu(), ref[0]) and int(bad.item()) == 0, "device entry != kCPU"
        steps = int((ref[0][:, 1:] >= 0).sum())
        return device, steps

    first, first_device_ms = [], {}
    for length in LENGTHS:
        device, steps = checked(length, 1.0, 1.0)
        t = timed({"call": lambda: flow_spmm.random_walk(rp, ci, starts, length, seed=SEED),
                   "device": device, "torch": lambda: torch_walk(starts, length)}, args.reps)
        t["cpu"] = cpu_times(length, 1.0, 1.0)
        first_device_ms[length] = t["device"][0]
        first.append({"length": length, "steps": steps,
                      "steps_per_s_device": round(steps / (t["device"][0] * 1e-3)),
                      **record(t, (("call", "torch"), ("device", "torch"), ("cpu", "call")))})
        del device

    sstarts = starts[:max(SAINT_STARTS // args.scale, 1)].contiguous()

    def saint_torch():
        nodes = torch_walk(sstarts, SAINT_LENGTH).reshape(-1).to(torch.int32)
        return flow_spmm.node_subgraph(rp, ci, nodes)

    ts = timed({"random_walk_subgraph":
                lambda: flow_spmm.random_walk_subgraph(rp, ci, sstarts, SAINT_LENGTH, seed=SEED),
                "torch_walk_then_node_subgraph": saint_torch}, args.reps)
    saint = {"starts": sstarts.numel(), "length": SAINT_LENGTH,
             **record(ts, (("random_walk_subgraph", "torch_walk_then_node_subgraph"),))}

    second = []
    sample = perm[:s:100].astype(np.int64)
    for p, q in PQ:
        device, steps = checked(SECOND_LENGTH, p, q)
        t = timed({"call": lambda: flow_spmm.random_walk(rp, ci, starts, SECOND_LENGTH, p=p, q=q,
                                                         seed=SEED), "device": device}, args.reps)
        t["cpu"] = cpu_times(SECOND_LENGTH, p, q)
        w, _, stats = restatement.reference(rp_n, ci_n, sample, SECOND_LENGTH, p, q, SEED)
        second.append({"p": p, "q": q, "length": SECOND_LENGTH, "steps": steps,
                       "mean_attempts_per_step": round(stats["attempts"] / max(int((w[:, 1:] >= 0).sum()), 1), 3),
                       "device_over_first_order_device":
                           round(t["device"][0] / first_device_ms[SECOND_LENGTH], 3),
                       "steps_per_s_device": round(steps / (t["device"][0] * 1e-3)),
                       **record(t, (("cpu", "call"),))})
        del device

    res = {"graph": "products", "device": torch.cuda.get_device_name(0), "m": m, "nnz": nnz,
           "num_starts": s, "idx": "int32", "reps": args.reps, "cpu_threads": CPU_THREADS,
           "first_order": first, "graphsaint": saint, "second_order": second,
           "call_below_torch_at_every_length": all(r["ratios"]["call_over_torch"] < 1 for r in first)}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

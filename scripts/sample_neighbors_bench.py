#!/usr/bin/env python3
"""Times the neighbour sampler (`sample_neighbors`, csrc/sample_neighbors.hip) on the bench's
products-shaped synthetic CSR (oneflow_spmm.synth, int32: 2,449,029 rows, 123,718,280 nonzeros)
with 1,000,000 distinct seeds at fanout 5, 10, 15 and 25.  Per fanout, on the same CSR and seeds:

  * "call":    `sample_neighbors` on the GPU as a user calls it: the allocations, the three
               launches and the one read-back of the count and the flag;
  * "device":  the C-ABI entry alone on preallocated outputs (HIP events, no read-back);
  * "cpu":     the same call on CPU tensors, the kCPU kernel at 16 threads (wall clock);
  * "gather":  the floor: `col_idx[positions]` in torch on the GPU for as many random positions
               as the call returns entries (its reads are as scattered, and it draws nothing).

The GPU arrays are checked against the kCPU kernel's before anything is timed.

Protocol (scripts/heads_bench.py): HIP events around each call, 3 warm-up rounds, median (and
minimum) of --reps runs, the GPU candidates alternating round by round in one process.
Results: one JSON line with the four fanouts, and profiles/sample_neighbors_bench.json."""
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
CPU_THREADS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=5)
    ap.add_argument("--scale", type=int, default=1, help="divide the problem's sizes (rehearsal)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_neighbors_bench.json"))
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
    seeds_h = torch.from_numpy(np.random.default_rng(0).permutation(m)[:s].astype(np.int32))
    rp, ci, seeds = rp_h.to(dev), ci_h.to(dev), seeds_h.to(dev)
    idt = _C.dtype_code(torch.int32)
    gen = torch.Generator(device=dev).manual_seed(1)
    rows = []
    for fanout in FANOUTS:
        got = flow_spmm.sample_neighbors(rp, ci, seeds, fanout, seed=1)
        ref = flow_spmm.sample_neighbors(rp_h, ci_h, seeds_h, fanout, seed=1, num_threads=CPU_THREADS)
        assert all(torch.equal(g.cpu(), r) for g, r in zip(got, ref)), "GPU != kCPU"
        nnz_s = got[1].numel()
        positions = torch.randint(0, nnz, (nnz_s,), device=dev, generator=gen)

        ws_bytes = ctypes.c_size_t(0)
        _lib.check(_lib.LIB.ofx_sample_neighbors_workspace_size(idt, s, ctypes.byref(ws_bytes)))
        ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8, device=dev)
        out_rp = torch.empty(s + 1, dtype=torch.int32, device=dev)
        out_ci, out_eid = (torch.empty(s * fanout, dtype=torch.int32, device=dev) for _ in range(2))
        scalars = torch.zeros(2, dtype=torch.int64, device=dev)

        def call():
            return flow_spmm.sample_neighbors(rp, ci, seeds, fanout, seed=1)

        def device():
            _lib.check(_lib.LIB.ofx_sample_neighbors(
                _C.current_stream_handle(rp), idt, m, s, rp.data_ptr(), ci.data_ptr(),
                seeds.data_ptr(), fanout, 1, out_rp.data_ptr(), out_ci.data_ptr(),
                out_eid.data_ptr(), scalars.data_ptr(), scalars.data_ptr() + 8, ws.data_ptr(),
                ws_bytes.value))

        def gather():
            return ci[positions]

        device()
        assert torch.equal(out_eid[:nnz_s], got[2]) and scalars.tolist() == [nnz_s, 0]
        t = timed({"call": call, "device": device, "gather": gather}, args.reps)
        cpu = []
        for _ in range(args.cpu_reps):
            t0 = time.perf_counter()
            flow_spmm.sample_neighbors(rp_h, ci_h, seeds_h, fanout, seed=1, num_threads=CPU_THREADS)
            cpu.append((time.perf_counter() - t0) * 1e3)
        t["cpu"] = (float(np.median(cpu)), float(np.min(cpu)))
        rows.append({"fanout": fanout, "nnz_s": nnz_s,
                     "timings": {k: {"median_ms": round(v[0], 4), "min_ms": round(v[1], 4)}
                                 for k, v in t.items()},
                     "ratios": {"call_over_gather": round(t["call"][0] / t["gather"][0], 2),
                                "device_over_gather": round(t["device"][0] / t["gather"][0], 2),
                                "cpu_over_call": round(t["cpu"][0] / t["call"][0], 2)}})
    res = {"graph": "products", "device": torch.cuda.get_device_name(0), "m": m, "nnz": nnz,
           "num_seeds": s, "idx": "int32", "reps": args.reps, "cpu_threads": CPU_THREADS,
           "fanouts": rows}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

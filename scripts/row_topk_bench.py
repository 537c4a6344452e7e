#!/usr/bin/env python3
"""Times the per-row top-k selection (`row_topk`, csrc/row_topk.hip) on the bench's products-shaped
synthetic CSR (oneflow_spmm.synth, int32: 2,449,029 rows, 123,718,280 nonzeros) with float32 values,
k = 1, 8, 32 and 128:
  * "call":    `row_topk` on the GPU as a user calls it: the allocations, the launches and the one
               read-back of nnz_s and the flag;
  * "device":  the C-ABI entry alone on preallocated buffers (HIP events, no read-back);
  * "torch":   the only device route torch offers: a stable argsort of all nnz values, a stable
               argsort of their row ids, the rank inside the row < k, nonzero (the row id of every
               entry is made outside the timed window, and the kept entries come out by value, not
               by position: ordering them would cost it one more sort);
  * "copy":    a torch copy of `values`, nnz elements: the cost of touching the input once;
  * "cpu":     the same call on CPU tensors, the kCPU kernel at 16 threads (wall clock).
The GPU arrays are checked against the kCPU kernel's before anything is timed.  Protocol
(scripts/compact_block_bench.py): HIP events around each call, 3 warm-up rounds, median (and
minimum) of --reps runs, the GPU candidates alternating round by round in one process.  Results:
one JSON line, and profiles/row_topk_bench.json."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "of-spmm_amd"), ROOT, os.path.join(ROOT, "scripts")]

KS = (1, 8, 32, 128)
CPU_THREADS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--scale", type=int, default=1, help="divide the problem's sizes (rehearsal)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "row_topk_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import oneflow_spmm as flow_spmm
    from heads_bench import timed
    from oneflow_spmm import _C, _lib, synth
    cfg = synth.CONFIGS["products"]
    m, nnz = cfg["m"] // args.scale, cfg["nnz"] // args.scale
    dev = torch.device("cuda", 0)
    rp_n = synth.row_ptr(m, m, nnz)
    ci_n = synth.columns(m, m, rp_n, threads=CPU_THREADS)
    rp_h, ci_h = torch.from_numpy(rp_n).to(torch.int32), torch.from_numpy(ci_n).to(torch.int32)
    val_h = torch.randn(nnz, generator=torch.Generator().manual_seed(0))
    rp, ci, val = rp_h.to(dev), ci_h.to(dev), val_h.to(dev)
    idt, vdt = _C.dtype_code(torch.int32), _C.dtype_code(torch.float32)
    deg = np.diff(rp_n)
    row_id = torch.repeat_interleave(torch.arange(m, device=dev), (rp[1:] - rp[:-1]).long())
    first = rp.long()[row_id]  # the first entry of every entry's row
    position = torch.arange(nnz, device=dev)

    def torch_route(k):
        by_value = torch.argsort(val, descending=True, stable=True)
        by_row = torch.argsort(row_id[by_value], stable=True)
        return by_value[by_row][torch.nonzero(position - first < k).squeeze(1)]

    ws_bytes = ctypes.c_size_t(0)
    _lib.check(_lib.LIB.ofx_row_topk_workspace_size(idt, m, nnz, ctypes.byref(ws_bytes)))
    ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8, device=dev)
    scalars = torch.zeros(2, dtype=torch.int64, device=dev)

    def device_entry(k):
        out = [torch.empty(n, dtype=torch.int32, device=dev) for n in (m + 1, min(nnz, m * k), min(nnz, m * k))]

        def run():
            _lib.check(_lib.LIB.ofx_row_topk(
                _C.current_stream_handle(rp), idt, vdt, m, nnz, rp.data_ptr(), ci.data_ptr(),
                val.data_ptr(), k, 1, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                scalars.data_ptr(), scalars.data_ptr() + 8, ws.data_ptr(), ws_bytes.value))
        return run, out

    rows = []
    for k in KS:
        ref = flow_spmm.row_topk(rp_h, ci_h, val_h, k, num_threads=CPU_THREADS)
        got = flow_spmm.row_topk(rp, ci, val, k)
        assert all(torch.equal(g.cpu(), r) for g, r in zip(got, ref)), "GPU != kCPU"
        device, out = device_entry(k)
        device()
        n_out, bad = scalars.tolist()
        assert bad == 0 and torch.equal(out[0].cpu(), ref[0]) and torch.equal(out[2][:n_out].cpu(), ref[2])
        assert torch.equal(torch.sort(torch_route(k)).values.cpu(), ref[2].long()), "torch route != kCPU"
        t = timed({"call": lambda: flow_spmm.row_topk(rp, ci, val, k), "device": device,
                   "torch": lambda: torch_route(k), "copy": lambda: val.clone()}, args.reps)
        ts = []
        for _ in range(args.cpu_reps):
            t0 = time.perf_counter()
            flow_spmm.row_topk(rp_h, ci_h, val_h, k, num_threads=CPU_THREADS)
            ts.append((time.perf_counter() - t0) * 1e3)
        t["cpu"] = (float(np.median(ts)), float(np.min(ts)))
        rows.append({"k": k, "nnz_s": n_out, "rows_selecting": int((deg > k).sum()),
                     "timings": {n: {"median_ms": round(v[0], 4), "min_ms": round(v[1], 4)}
                                 for n, v in t.items()},
                     "ratios": {f"{a}_over_{b}": round(t[a][0] / t[b][0], 3) for a, b in
                                (("call", "torch"), ("device", "torch"), ("call", "copy"),
                                 ("device", "copy"), ("cpu", "call"))}})
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
        del device, out

    res = {"graph": "products", "device": torch.cuda.get_device_name(0), "m": m, "nnz": nnz,
           "values": "float32", "idx": "int32", "reps": args.reps, "cpu_threads": CPU_THREADS,
           "rows_over_64": int((deg > 64).sum()), "rows_over_512": int((deg > 512).sum()),
           "max_degree": int(deg.max()), "by_k": rows,
           "call_below_torch_at_every_k": all(r["ratios"]["call_over_torch"] < 1 for r in rows)}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Times the max / mean aggregation of spmm and its gradients beside the sum op on the same inputs
in one process: the products-shaped config (f32, N = 128) and the Reddit-shaped one (bf16,
N = 256).  HIP events around each call on the launch stream, median of 20 after warm-up (the
protocol of scripts/bench_backward.py).  Writes profiles/reduce_bench.json with the times, the
byte model and the resulting TB/s.

Byte model: the sum op's gather model (row_ptr + col_idx + values + one B row per nonzero + the
output) plus M * N * sizeof(index) for the arg write of the forward, or for the arg
read of a gradient."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "of-spmm_amd"), ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, reps=20, warmup=3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def run_config(name, reps):
    import oneflow_spmm as fs
    from oneflow_spmm import _C, synth
    from oneflow_spmm import autograd as ag
    cfg = synth.CONFIGS[name]
    m, k, nnz, n, dt = cfg["m"], cfg["k"], cfg["nnz"], cfg["n"], cfg["dtype"]
    dev = torch.device("cuda", 0)
    rp, ci, v = synth.csr(m, k, nnz, val_dtype=dt, threads=16)
    rp, ci, v = rp.to(dev), ci.to(dev), v.to(dev)
    b = synth.dense(0, k, n, dt, device=dev)
    g = synth.dense(0, m, n, dt, device=dev, seed=7)
    sv, si = b.element_size(), rp.element_size()
    fwd_bytes = si * (m + 1) + (si + sv) * nnz + sv * nnz * n + sv * m * n
    db_bytes = si * (k + 1) + (2 * si + sv) * nnz + sv * nnz * n + sv * k * n
    dv_bytes = si * (m + 1) + si * nnz + sv * nnz * n + sv * m * n + sv * nnz
    arg_bytes = si * m * n
    rt, ct, perm = fs.csr_transpose(rp, ci, k)
    vt = ag.gather_values(perm, v)
    out, arg = _C.spmm_csr_reduce(rp, ci, v, m, k, b, "max")
    res = {"config": name, "m": m, "nnz": nnz, "n": n, "dtype": str(dt).split(".")[-1]}

    def rec(key, ms, nbytes):
        res[key] = {"ms": round(ms, 4), "model_bytes": nbytes,
                    "model_tbs": round(nbytes / (ms * 1e-3) / 1e12, 3)}

    rec("sum_forward", timed(lambda: fs.spmm_csr(rp, ci, v, m, k, b), reps), fwd_bytes)
    rec("max_forward", timed(lambda: _C.spmm_csr_reduce(rp, ci, v, m, k, b, "max"), reps),
        fwd_bytes + arg_bytes)
    rec("mean_forward", timed(lambda: _C.spmm_csr_reduce(rp, ci, v, m, k, b, "mean"), reps),
        fwd_bytes + 2 * sv * m * n)
    rec("sum_grad_b", timed(lambda: fs.spmm_csr(rt, ct, vt, k, m, g), reps), db_bytes - si * nnz)
    rec("max_grad_b", timed(lambda: _C.spmm_csr_reduce_grad_b(rt, ct, perm, v, arg, g, m, k), reps),
        db_bytes + arg_bytes)
    rec("sum_grad_values", timed(lambda: fs.sddmm(rp, ci, g, b), reps), dv_bytes)
    rec("max_grad_values",
        timed(lambda: _C.spmm_csr_reduce_grad_values(rp, ci, arg, g, b, m, k), reps),
        dv_bytes + arg_bytes)
    for a, s in (("max_forward", "sum_forward"), ("max_grad_b", "sum_grad_b"),
                 ("max_grad_values", "sum_grad_values"), ("mean_forward", "sum_forward")):
        res[f"{a}_over_{s}"] = {"measured": round(res[a]["ms"] / res[s]["ms"], 3),
                                "model": round(res[a]["model_bytes"] / res[s]["model_bytes"], 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="products,reddit")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduce_bench.json"))
    args = ap.parse_args()
    results = []
    for name in args.configs.split(","):
        results.append(run_config(name, args.reps))
        print(json.dumps(results[-1]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps,
                   "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

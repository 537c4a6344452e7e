#!/usr/bin/env python3
"""Times `segment_matmul` (ops "segment_matmul" / "segment_matmul_grad_w") against the route that
serves a typed linear transform today, on shapes fixed here before any measurement:

  * edge-typed messages x[col[j]] @ w[etype[j]]: the 1M-node power-law graph of the bench (20M
    edges, oneflow_spmm.synth), edges sorted by one of T = 16 or 64 types with skewed sizes,
    idx = col_idx in that order; bf16 128 -> 128 and f32 64 -> 64;
  * HeteroLinear: 2,449,029 nodes in T = 4 uneven types, no idx, bf16 128 -> 256 (recorded, not
    barred: a few torch.mm on large contiguous segments is a vendor GEMM at its best);
  * many small segments: 2M rows in T = 1024 segments of power-law lengths, bf16 128 -> 128.

Candidates, alternating round by round in one process on the same tensors:
  * "call": flow_spmm.segment_matmul;
  * "torch": the Python loop of torch.mm(x[idx[s:e]], w[t]) over the types, with its read-back of
    seg_ptr inside the timed window (a user's code reads it every call);
  * "step_call" / "step_torch": forward and backward with gradients in x and w.

Share of the bound: the call's least time, the larger of bytes / 8 TB/s (x rows read, out written,
w once) and flops / peak (2.5 PF/s dense bf16, 157 TF/s f32 matrix), over its median.

Bar (checked after the JSON is written): on every shape with a gather or T >= 16 the call's and
the step's medians are below torch's by more than the spread (max - min over the reps of either).

Protocol (scripts/heads_bench.py): HIP events around each call, 3 warm-up rounds, median and
minimum of --reps runs.  Run without --step the script is the driver: every step is a child process
of its own under `timeout -k 10`, and the first step that fails ends the run.
Results: one JSON line per step, and profiles/segment_matmul_bench.json (--out)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "of-spmm_amd"), ROOT, os.path.join(ROOT, "scripts")]

# step -> (rows source, T, dtype, F_in, F_out, gather, barred)
STEPS = {"edges_t16_bf16_128": ("plaw1m", 16, "bf16", 128, 128, True, True),
         "edges_t64_bf16_128": ("plaw1m", 64, "bf16", 128, 128, True, True),
         "edges_t16_f32_64": ("plaw1m", 16, "f32", 64, 64, True, True),
         "hetero_t4_bf16_128_256": (2449029, 4, "bf16", 128, 256, False, False),
         "small_t1024_bf16_128": (2000000, 1024, "bf16", 128, 128, False, True)}
STEP_SECONDS = 420
PEAK_BYTES = 8e12
PEAK_FLOPS = {"bf16": 2.5e15, "f32": 157.3e12}


def skewed_lengths(total, t):
    """t segment lengths that sum to `total`, proportional to 1 / (rank + 1) (power-law sizes)."""
    import numpy as np
    wts = 1.0 / np.arange(1, t + 1)
    lens = np.floor(wts / wts.sum() * total).astype(np.int64)
    lens[0] += total - lens.sum()
    return lens


def run_step(name, reps, scale):
    import numpy as np
    import torch

    import oneflow_spmm as flow_spmm
    from heads_bench import timed
    from oneflow_spmm import synth
    src, t, dtn, f_in, f_out, gather, barred = STEPS[name]
    dt = {"f32": torch.float32, "bf16": torch.bfloat16}[dtn]
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    idx = None
    if gather:
        cfg = synth.CONFIGS[src]
        r, s = cfg["m"] // scale, cfg["nnz"] // scale
        rp_h = synth.row_ptr(r, r, s)
        idx = torch.from_numpy(synth.columns(r, r, rp_h, threads=16)).to(torch.int32).to(dev)
        s = idx.numel()
    else:
        r = s = src // scale
    seg_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(skewed_lengths(s, t))])).to(
        torch.int32).to(dev)
    x = torch.randn(r, f_in, device=dev, generator=gen).to(dt)
    w = (torch.randn(t, f_in, f_out, device=dev, generator=gen) / f_in ** 0.5).to(dt)
    lidx = idx.long() if idx is not None else None

    def torch_route(xx, ww):
        bounds = seg_ptr.tolist()  # the read-back of the route
        return torch.cat([torch.mm(xx[lidx[a:b]] if lidx is not None else xx[a:b], ww[i])
                          for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:]))])

    def call(xx, ww):
        return flow_spmm.segment_matmul(xx, ww, seg_ptr, idx)

    got, want = call(x, w).float(), torch_route(x, w).float()
    max_diff = float((got - want).abs().max())
    assert max_diff <= 2.0 ** -(7 if dtn == "bf16" else 18) * float(want.abs().max()), max_diff
    del got, want
    tm = timed({"call": lambda: call(x, w), "torch": lambda: torch_route(x, w)}, reps)
    dy = torch.randn(s, f_out, device=dev, generator=gen).to(dt)
    px, pw = x.clone().requires_grad_(True), w.clone().requires_grad_(True)

    def step(f):
        px.grad = pw.grad = None
        f(px, pw).backward(dy)

    tm.update(timed({"step_call": lambda: step(call), "step_torch": lambda: step(torch_route)},
                    reps))
    es = 2 if dtn == "bf16" else 4
    bytes_ = (s * f_in + s * f_out + t * f_in * f_out) * es + (s * 4 if gather else 0)
    flops = 2.0 * s * f_in * f_out
    t_bytes, t_flops = bytes_ / PEAK_BYTES * 1e3, flops / PEAK_FLOPS[dtn] * 1e3
    res = {"step": name, "device": torch.cuda.get_device_name(0), "dtype": dtn, "r": r, "s": s,
           "t": t, "f_in": f_in, "f_out": f_out, "gather": gather, "barred": barred, "reps": reps,
           "max_abs_diff_vs_torch": max_diff,
           "timings": {key: {"median_ms": round(v[0], 4), "min_ms": round(v[1], 4)}
                       for key, v in tm.items()},
           "bound": {"bytes_ms": round(t_bytes, 4), "flops_ms": round(t_flops, 4),
                     "bound_by": "bytes" if t_bytes >= t_flops else "flops",
                     "call_share": round(max(t_bytes, t_flops) / tm["call"][0], 3)}}
    res["ratios"] = {"call_over_torch": round(tm["call"][0] / tm["torch"][0], 3),
                     "step_call_over_torch": round(tm["step_call"][0] / tm["step_torch"][0], 3)}
    # "below": the call's median under torch's fastest run (torch's median - its spread downwards)
    res["accepted"] = (not barred) or (tm["call"][0] < tm["torch"][1]
                                       and tm["step_call"][0] < tm["step_torch"][1])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=list(STEPS), help="run one step in this process (the driver's child)")
    ap.add_argument("--steps", default=",".join(STEPS), help="the driver's steps, comma-separated")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scale", type=int, default=1, help="divide the problem's rows (rehearsal)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_matmul_bench.json"))
    args = ap.parse_args()
    if args.step:
        print(json.dumps(run_step(args.step, args.reps, args.scale)), flush=True)
        return 0
    results = []
    for step in args.steps.split(","):  # one step a process; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__),
               "--step", step, "--reps", str(args.reps), "--scale", str(args.scale)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            print(f"step {step} failed with exit status {r.returncode}: the run ends here",
                  file=sys.stderr)
            return r.returncode
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        results.append(json.loads(line))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"results": results}, f, indent=1)
        f.write("\n")
    if not all(r["accepted"] for r in results):
        print("BAR MISSED: a median of segment_matmul is not below the torch route's", file=sys.stderr)
        return 3
    return 0


if __name__ == "__main__":
    sys.exit(main())

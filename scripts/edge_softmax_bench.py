#!/usr/bin/env python3
"""Times op "edge_softmax_csr" and its gradient against the torch composition a user would write
without it, on the same GPU and tensors, at the bench's products-shaped CSR (2.45M rows, 123.7M
nonzeros), f32 and bf16.

The composition (forward): scatter_reduce(amax) over a materialised row-id vector, gather, exp,
index_add_, gather, divide; (backward): multiply, index_add_, gather, subtract, multiply.  Its
row-id vector (int64 [nnz], which the CSR does not have) is built once outside the timed window;
the time to build it is reported beside the others.

Protocol (scripts/bench_backward.py): HIP events around each call on the launch stream, warm-up,
median (and minimum) of --reps runs, the two contenders alternating in one process.  Achieved
bytes/s are against the algorithmic minimum 2 * nnz * sizeof(T) + (m + 1) * sizeof(I) of the
forward (read e, write y, read row_ptr); the backward reads y and g and writes de:
3 * nnz * sizeof(T) + (m + 1) * sizeof(I).

Run without --step, the script is the driver: every GPU step is a child process of its own under
`timeout -k 10`, and the first step that fails ends the run.  Results: one JSON line per step, and
profiles/edge_softmax_bench.json."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "of-spmm_amd"), ROOT]

STEPS = ("f32", "bf16")
STEP_SECONDS = 420


def timed_pair(fns, reps, warmup=3):
    """Median and minimum ms of each callable, the callables alternating round by round."""
    import numpy as np
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[i].append(e0.elapsed_time(e1))
    return [(float(np.median(t)), float(np.min(t))) for t in ts]


def run_step(name, reps, scale):
    import time

    import torch
    from oneflow_spmm import _C, synth
    cfg = synth.CONFIGS["products"]
    m, nnz = cfg["m"] // scale, cfg["nnz"] // scale
    dt = {"f32": torch.float32, "bf16": torch.bfloat16}[name]
    dev = torch.device("cuda", 0)
    rp = torch.from_numpy(synth.row_ptr(m, m, nnz).astype("int32")).to(dev)
    ci = torch.empty(nnz, dtype=torch.int32, device=dev)  # taken for its shape only
    gen = torch.Generator(device=dev).manual_seed(1)
    e = (4 * torch.randn(nnz, device=dev, generator=gen)).to(dt)
    g = torch.randn(nnz, device=dev, generator=gen).to(dt)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rows = torch.repeat_interleave(torch.arange(m, device=dev), torch.diff(rp.long()))
    torch.cuda.synchronize()
    rows_ms = (time.perf_counter() - t0) * 1e3

    def comp_fwd():
        mx = torch.full((m,), float("-inf"), dtype=dt, device=dev)
        mx.scatter_reduce_(0, rows, e, "amax", include_self=True)
        x = torch.exp(e - mx[rows])
        s = torch.zeros(m, dtype=dt, device=dev).index_add_(0, rows, x)
        return x / s[rows]

    y = _C.edge_softmax_csr(rp, ci, e)
    out = torch.empty_like(e)

    def comp_bwd():
        d = torch.zeros(m, dtype=dt, device=dev).index_add_(0, rows, y * g)
        return y * (g - d[rows])

    # both forwards against the composition in float64 (its atomic sums are then exact enough to
    # be the reference); the op must be within 1e-5 of it in f32
    e_lo = e
    e = e_lo.double()
    dt_lo, dt = dt, torch.float64
    ref = comp_fwd()
    e, dt = e_lo, dt_lo
    err = float((y.double() - ref).abs().max())
    comp_err = float((comp_fwd().double() - ref).abs().max())
    j = int((y.double() - ref).abs().argmax())
    r = int(rows[j])
    print(f"{name}: max |error| against float64: op {err:.3e} (nonzero {j}, a row of "
          f"{int(rp[r + 1] - rp[r])}), composition {comp_err:.3e}", file=sys.stderr, flush=True)
    assert dt != torch.float32 or err <= 1e-5, f"op against float64: max |diff| {err}"
    del ref
    (op_f, comp_f) = timed_pair([lambda: _C.edge_softmax_csr(rp, ci, e, out=out), comp_fwd], reps)
    (op_b, comp_b) = timed_pair([lambda: _C.edge_softmax_csr_grad(rp, ci, y, g), comp_bwd], reps)
    sv, si = e.element_size(), rp.element_size()
    fwd_bytes = 2 * nnz * sv + (m + 1) * si
    bwd_bytes = 3 * nnz * sv + (m + 1) * si

    def rec(t, nbytes):
        return {"median_ms": round(t[0], 4), "min_ms": round(t[1], 4),
                "algorithmic_bytes": nbytes,
                "achieved_tbs": round(nbytes / (t[0] * 1e-3) / 1e12, 3)}

    return {"step": name, "device": torch.cuda.get_device_name(0), "m": m, "nnz": nnz,
            "reps": reps, "forward_op": rec(op_f, fwd_bytes),
            "forward_composition": rec(comp_f, fwd_bytes), "backward_op": rec(op_b, bwd_bytes),
            "backward_composition": rec(comp_b, bwd_bytes),
            "forward_speedup": round(comp_f[0] / op_f[0], 2),
            "backward_speedup": round(comp_b[0] / op_b[0], 2),
            "row_id_vector_ms": round(rows_ms, 3), "forward_op_max_abs_err_vs_f64": err,
            "forward_composition_max_abs_err_vs_f64": comp_err}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS, help="run one step in this process (the driver's child)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scale", type=int, default=1, help="divide the problem's m and nnz (rehearsal)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_softmax_bench.json"))
    args = ap.parse_args()
    if args.step:
        print(json.dumps(run_step(args.step, args.reps, args.scale)), flush=True)
        return 0
    results = []
    for step in STEPS:
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
    return 0


if __name__ == "__main__":
    sys.exit(main())

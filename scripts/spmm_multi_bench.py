#!/usr/bin/env python3
"""Times the multi-aggregator SpMM (`spmm_multi`, op "spmm_csr_multi") with aggrs = (mean, max, min,
std) on the bench's synthetic CSRs (oneflow_spmm.synth, int32): the products-shaped one (2,449,029
rows, 123,718,280 nonzeros) at f32 N=64 and bf16 N=128 and the 1M x 1M / 20M-nonzero power-law one
at f32 N=64.  Candidates, on the same GPU and tensors:

  * "multi": `spmm_multi`, one walk of the CSR and one gather of b;
  * "composed": the route that serves it today on the same tree: `spmm(reduce="mean")`,
    `spmm_reduce("max")`, `spmm_reduce("min")`, and std from two `spmm` calls over b and b * b with
    the values and their squares plus torch arithmetic (five walks, five gathers; b * b and the
    squared values are formed inside the timed window, as a user's code forms them);
  * "max": a single `spmm_reduce("max")` call, for scale (recorded, not gated);
  * "step_multi" / "step_composed": forward and backward with gradients in values and b.

Bar (checked after the measurement, once the JSON is written): in every step the forward and the
training-step medians of spmm_multi are below the composition's.

Protocol (scripts/heads_bench.py): HIP events around each call, 3 warm-up rounds, median (and
minimum) of --reps runs, the candidates alternating round by round in one process.  Run without
--step the script is the driver: every step is a child process of its own under `timeout -k 10`,
and the first step that fails ends the run.
Results: one JSON line per step, and profiles/spmm_multi_bench.json (--out)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "of-spmm_amd"), ROOT, os.path.join(ROOT, "scripts")]

# step -> (graph, dtype, N)
STEPS = {"plaw1m_f32_n64": ("plaw1m", "f32", 64),
         "products_f32_n64": ("products", "f32", 64),
         "products_bf16_n128": ("products", "bf16", 128)}
STEP_SECONDS = 420
AGGRS = ("mean", "max", "min", "std")
EPS = 1e-5


def run_step(name, reps, scale):
    import torch

    import oneflow_spmm as flow_spmm
    from heads_bench import timed
    from oneflow_spmm import synth
    graph, dtn, n = STEPS[name]
    cfg = synth.CONFIGS[graph]
    m, nnz = cfg["m"] // scale, cfg["nnz"] // scale
    k = m
    dt = {"f32": torch.float32, "bf16": torch.bfloat16}[dtn]
    dev = torch.device("cuda", 0)
    rp_h = synth.row_ptr(m, k, nnz)
    ci = torch.from_numpy(synth.columns(m, k, rp_h, threads=16)).to(dev)
    rp = torch.from_numpy(rp_h).to(torch.int32).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    b = torch.randn(k, n, device=dev, generator=gen).to(dt)
    values = torch.randn(nnz, device=dev, generator=gen).to(dt)
    deg = (rp[1:] - rp[:-1]).float().clamp(min=1).unsqueeze(1)

    def composed(v, x):
        mean = flow_spmm.spmm(rp, ci, v, m, k, x, reduce="mean")
        mx = flow_spmm.spmm_reduce(rp, ci, v, m, k, x, "max")[0]
        mn = flow_spmm.spmm_reduce(rp, ci, v, m, k, x, "min")[0]
        s1 = flow_spmm.spmm(rp, ci, v, m, k, x).float()
        s2 = flow_spmm.spmm(rp, ci, v * v, m, k, x * x).float()
        var = (s2 / deg - (s1 / deg) ** 2).clamp(min=0)
        return torch.stack((mean, mx, mn, (var + EPS).sqrt().to(dt)), 1)

    def multi(v, x):
        return flow_spmm.spmm_multi(rp, ci, v, m, k, x, AGGRS, EPS)

    got, want = multi(values, b), composed(values, b)
    for i in range(3):  # mean / max / min: the same operations in the same order
        assert torch.equal(got[:, i], want[:, i]), f"spmm_multi != the composition ({AGGRS[i]})"
    std_diff = float((got[:, 3].float() - want[:, 3].float()).abs().max())
    del got, want
    t = timed({"fwd_multi": lambda: multi(values, b), "fwd_composed": lambda: composed(values, b),
               "fwd_max": lambda: flow_spmm.spmm_reduce(rp, ci, values, m, k, b, "max")}, reps)

    w = torch.randn(m, len(AGGRS), n, device=dev, generator=gen).to(dt)
    pv, pb = values.clone().requires_grad_(True), b.clone().requires_grad_(True)

    def step(f):
        pv.grad = pb.grad = None
        f(pv, pb).backward(w)

    t.update(timed({"step_multi": lambda: step(multi), "step_composed": lambda: step(composed)},
                   reps))
    res = {"step": name, "device": torch.cuda.get_device_name(0), "graph": graph, "dtype": dtn,
           "n": n, "m": m, "k": k, "nnz": nnz, "reps": reps, "aggrs": AGGRS,
           "std_max_abs_diff": std_diff,
           "timings": {key: {"median_ms": round(v[0], 4), "min_ms": round(v[1], 4)}
                       for key, v in t.items()}}
    res["ratios"] = {
        "fwd_multi_over_composed": round(t["fwd_multi"][0] / t["fwd_composed"][0], 3),
        "fwd_multi_over_max": round(t["fwd_multi"][0] / t["fwd_max"][0], 3),
        "step_multi_over_composed": round(t["step_multi"][0] / t["step_composed"][0], 3)}
    res["accepted"] = res["ratios"]["fwd_multi_over_composed"] < 1 and \
        res["ratios"]["step_multi_over_composed"] < 1
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=list(STEPS), help="run one step in this process (the driver's child)")
    ap.add_argument("--steps", default=",".join(STEPS), help="the driver's steps, comma-separated")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scale", type=int, default=1, help="divide the problem's m and nnz (rehearsal)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spmm_multi_bench.json"))
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
        print("BAR MISSED: a median of spmm_multi is not below the composition's", file=sys.stderr)
        return 3
    return 0


if __name__ == "__main__":
    sys.exit(main())

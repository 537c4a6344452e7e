#!/usr/bin/env python3
"""Times the multi-head edge softmax (ops "edge_softmax_csr_heads" / "_grad") at the bench's
products-shaped CSR (2,449,029 rows, 123,718,280 nonzeros, int32), f32 H=4, f32 H=8 and bf16 H=8,
forward and backward, against three things on the same GPU and tensors:

  * "composed": the per-head composition starting from the packed [nnz, H] tensor (what the 2-D
    `edge_softmax` was before the native op: e[:, h].contiguous() per head, H launches of the
    single-head op and a stack; the backward through autograd);
  * "hoisted": the same H single-head launches on per-head contiguous columns prepared outside the
    timed window, writing per-head results (the composition's best case);
  * "single": the single-head op on a 1-D tensor of nnz*H elements over a CSR whose rows are H
    times as long: the same bytes in one launch.  Its ratio is recorded, not gated.

Acceptance (asserted after the measurement): in every configuration the native op's median is not
above the hoisted composition's, forward and backward.

Protocol (scripts/heads_bench.py): HIP events around each call, 3 warm-up rounds, median (and
minimum) of --reps runs, the candidates alternating round by round in one process.  Achieved
bytes/s are over the algorithmic bytes: forward 2*nnz*H*sizeof(T) + (m+1)*sizeof(I), backward three
such nnz terms.  The kernels do not read col_idx, so it is a zero tensor of the right length.  Run
without --step the script is the driver: every configuration is a child process of its own under
`timeout -k 10`, and the first step that fails ends the run.
Results: one JSON line per step, and profiles/edge_softmax_heads_bench.json."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "of-spmm_amd"), ROOT, os.path.join(ROOT, "scripts")]

STEPS = {"f32_h4": ("f32", 4), "f32_h8": ("f32", 8), "bf16_h8": ("bf16", 8)}
STEP_SECONDS = 300


def run_step(name, reps, scale):
    import torch

    from heads_bench import timed
    from oneflow_spmm import _C, autograd, synth
    dtn, h = STEPS[name]
    cfg = synth.CONFIGS["products"]
    m, nnz = cfg["m"] // scale, cfg["nnz"] // scale
    dt = {"f32": torch.float32, "bf16": torch.bfloat16}[dtn]
    bits = torch.int16 if dtn == "bf16" else torch.int32
    dev = torch.device("cuda", 0)
    rp_h = torch.from_numpy(synth.row_ptr(m, m, nnz).astype("int64"))
    rp = rp_h.to(torch.int32).to(dev)
    rp_long = (rp_h * h).to(torch.int32).to(dev)  # the same rows, H times as long (nnz*H < 2^31)
    ci = torch.zeros(nnz, dtype=torch.int32, device=dev)
    ci_long = torch.zeros(nnz * h, dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    e = torch.randn(nnz, h, device=dev, generator=gen).mul_(4).to(dt)
    g = torch.randn(nnz, h, device=dev, generator=gen).to(dt)
    y = torch.empty_like(e)
    eh = [e[:, i].contiguous() for i in range(h)]
    gh = [g[:, i].contiguous() for i in range(h)]
    yh = [torch.empty_like(eh[0]) for _ in range(h)]

    # ---- the candidates compute the same thing ---------------------------------------------------
    _C.edge_softmax_csr_heads(rp, ci, e, out=y)
    with torch.no_grad():
        want = autograd._edge_softmax_heads_composed(rp, ci, e)
    assert torch.equal(y.view(bits), want.view(bits)), "native forward != composition"
    de = _C.edge_softmax_csr_heads_grad(rp, ci, y, g)
    for i in range(h):
        _C.edge_softmax_csr(rp, ci, eh[i], out=yh[i])
        assert torch.equal(de[:, i].contiguous().view(bits),
                           _C.edge_softmax_csr_grad(rp, ci, yh[i], gh[i]).view(bits)), \
            "native backward != composition"
    del want, de

    def composed():
        with torch.no_grad():
            return autograd._edge_softmax_heads_composed(rp, ci, e)

    t = timed({
        "fwd_native": lambda: _C.edge_softmax_csr_heads(rp, ci, e, out=y),
        "fwd_composed": composed,
        "fwd_hoisted": lambda: [_C.edge_softmax_csr(rp, ci, eh[i], out=yh[i]) for i in range(h)],
        "fwd_single": lambda: _C.edge_softmax_csr(rp_long, ci_long, e.view(-1), out=y.view(-1)),
    }, reps)

    e_l = e.detach().clone().requires_grad_(True)
    y_c = autograd._edge_softmax_heads_composed(rp, ci, e_l)
    t.update(timed({
        "bwd_native": lambda: _C.edge_softmax_csr_heads_grad(rp, ci, y, g),
        "bwd_composed": lambda: torch.autograd.grad(y_c, e_l, g, retain_graph=True),
        "bwd_hoisted": lambda: [_C.edge_softmax_csr_grad(rp, ci, yh[i], gh[i]) for i in range(h)],
        "bwd_single": lambda: _C.edge_softmax_csr_grad(rp_long, ci_long, y.view(-1), g.view(-1)),
    }, reps))

    sv, si = e.element_size(), rp.element_size()
    model = {"fwd": 2 * nnz * h * sv + (m + 1) * si, "bwd": 3 * nnz * h * sv + (m + 1) * si}

    def rec(key):
        return {"median_ms": round(t[key][0], 4), "min_ms": round(t[key][1], 4),
                "achieved_tbs": round(model[key[:3]] / (t[key][0] * 1e-3) / 1e12, 3)}

    res = {"step": name, "device": torch.cuda.get_device_name(0), "dtype": dtn, "heads": h, "m": m,
           "nnz": nnz, "reps": reps, "algorithmic_bytes": model,
           "timings": {key: rec(key) for key in t}}
    res["ratios"] = {
        d: {"native_over_hoisted": round(t[f"{d}_native"][0] / t[f"{d}_hoisted"][0], 3),
            "native_over_composed": round(t[f"{d}_native"][0] / t[f"{d}_composed"][0], 3),
            "native_over_single": round(t[f"{d}_native"][0] / t[f"{d}_single"][0], 3)}
        for d in ("fwd", "bwd")}
    res["accepted"] = all(r["native_over_hoisted"] <= 1.0 for r in res["ratios"].values())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=list(STEPS), help="run one step in this process (the driver's child)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scale", type=int, default=1, help="divide the problem's m and nnz (rehearsal)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_softmax_heads_bench.json"))
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
    if not all(r["accepted"] for r in results):
        print("ACCEPTANCE FAILED: the native op's median is above the hoisted composition's",
              file=sys.stderr)
        return 3
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Times the fused multi-head graph attention (op "graph_attention_csr_heads",
`oneflow_spmm.graph_attention`) at the bench's products-shaped CSR (2,449,029 rows, 123,718,280
nonzeros, int32) for f32 H=8 D=16, f32 H=4 D=32 and bf16 H=8 D=32, against the composition it
replaces, on the same GPU and tensors and with the same library:

  (a) "fwd_fused":    graph_attention(q, k, v), no grad: the plan, one fused kernel for the rows of
                      at most 512 nonzeros, three small launches for the hub rows;
  (b) "fwd_composed": spmm(edge_softmax(sddmm(q, k)), v) through the public API, no grad: three
                      launches and two [nnz, H] tensors;
  (c) "step_fused" / "step_composed": a training step, the forward with autograd and its backward
      for d(q), d(k), d(v).  The two backwards are the same ops, so their difference should be the
      forwards'.

Bar (asserted after the measurement): in every configuration the fused forward's median is below
the composition's median from the same run.

Protocol (scripts/heads_bench.py): HIP events around each call, 3 warm-up rounds, median (and
minimum) of --reps runs, the candidates alternating round by round in one process.  Achieved
bytes/s are over the algorithmic bytes of the forward: two gathers of nnz*H*D*sizeof(T), col_idx
and row_ptr once, q once, out once, attn written once.  Run without --step the script is the
driver: every configuration is a child process of its own under `timeout -k 10`, and the first
step that fails ends the run.
Results: one JSON line per step, and profiles/graph_attention_bench.json, written before the bar
is judged: a file whose records say "bar_met": false comes from a run that ended with status 3.
The committed file is such a run (the bar is missed in all three configurations)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "of-spmm_amd"), ROOT, os.path.join(ROOT, "scripts")]

STEPS = {"f32_h8_d16": ("f32", 8, 16), "f32_h4_d32": ("f32", 4, 32), "bf16_h8_d32": ("bf16", 8, 32)}
STEP_SECONDS = 300


def run_step(name, reps, scale, cols_path):
    import numpy as np
    import torch

    import oneflow_spmm as fs
    from heads_bench import timed
    from oneflow_spmm import synth
    dtn, h, d = STEPS[name]
    cfg = synth.CONFIGS["products"]
    m, nnz = cfg["m"] // scale, cfg["nnz"] // scale
    k, n = m, h * d
    dt = {"f32": torch.float32, "bf16": torch.bfloat16}[dtn]
    bits = torch.int16 if dtn == "bf16" else torch.int32
    dev = torch.device("cuda", 0)
    rp_h = synth.row_ptr(m, k, nnz)
    ci_h = np.load(cols_path) if cols_path else synth.columns(m, k, rp_h, threads=16)
    rp = torch.from_numpy(rp_h.astype("int32")).to(dev)
    ci = torch.from_numpy(ci_h).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.rand(*s, device=dev, generator=gen).mul_(2).sub_(1).to(dt)  # noqa: E731
    q, kk, v, g = rnd(m, h, d), rnd(k, h, d), rnd(k, h, d), rnd(m, h, d)

    def composed(a, b, c):
        return fs.spmm(rp, ci, fs.edge_softmax(rp, ci, fs.sddmm(rp, ci, a, b)), m, k, c)

    # ---- the candidates compute the same thing ---------------------------------------------------
    with torch.no_grad():
        out, attn = fs.graph_attention(rp, ci, q, kk, v, return_attention=True)
        y = fs.edge_softmax(rp, ci, fs.sddmm(rp, ci, q, kk))
        assert torch.equal(attn.view(bits), y.view(bits)), "fused attn != composition"
        ref = fs.spmm(rp, ci, y, m, k, v)
        assert torch.equal(out.view(bits), ref.view(bits)), "fused out != composition"
    del out, attn, y, ref

    def fwd_fused():
        with torch.no_grad():
            return fs.graph_attention(rp, ci, q, kk, v)

    def fwd_composed():
        with torch.no_grad():
            return composed(q, kk, v)

    t = timed({"fwd_fused": fwd_fused, "fwd_composed": fwd_composed}, reps)

    leaves = tuple(x.detach().clone().requires_grad_(True) for x in (q, kk, v))

    def new_step():
        # the weights are new every step in training: the cache of values gathered for A^T never
        # hits (scripts/heads_bench.py new_step); A^T itself stays cached (the graph is static)
        fs.autograd.TRANSPOSE_CACHE.value_entries.clear()
        fs.autograd.TRANSPOSE_CACHE.seen.clear()

    t.update(timed({
        "step_fused": lambda: torch.autograd.grad(fs.graph_attention(rp, ci, *leaves), leaves, g),
        "step_composed": lambda: torch.autograd.grad(composed(*leaves), leaves, g),
    }, reps, prep=new_step))

    sv, si = q.element_size(), rp.element_size()
    model = 2 * nnz * n * sv + nnz * si + (m + 1) * si + 2 * m * n * sv + nnz * h * sv

    def rec(key):
        r = {"median_ms": round(t[key][0], 4), "min_ms": round(t[key][1], 4)}
        if key.startswith("fwd"):
            r["achieved_tbs"] = round(model / (t[key][0] * 1e-3) / 1e12, 3)
        return r

    res = {"step": name, "device": torch.cuda.get_device_name(0), "dtype": dtn, "heads": h, "d": d,
           "m": m, "nnz": nnz, "max_degree": int(np.diff(rp_h).max()), "reps": reps,
           "forward_algorithmic_bytes": model, "timings": {key: rec(key) for key in t}}
    res["ratios"] = {
        "fwd_fused_over_composed": round(t["fwd_fused"][0] / t["fwd_composed"][0], 3),
        "step_fused_over_composed": round(t["step_fused"][0] / t["step_composed"][0], 3)}
    res["forward_saving_ms"] = round(t["fwd_composed"][0] - t["fwd_fused"][0], 4)
    res["step_saving_ms"] = round(t["step_composed"][0] - t["step_fused"][0], 4)
    res["bar_met"] = t["fwd_fused"][0] < t["fwd_composed"][0]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=list(STEPS), help="run one step in this process (the driver's child)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scale", type=int, default=1, help="divide the problem's m and nnz (rehearsal)")
    ap.add_argument("--cols", default="", help="a .npy of the graph's columns (the driver's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_attention_bench.json"))
    args = ap.parse_args()
    if args.step:
        print(json.dumps(run_step(args.step, args.reps, args.scale, args.cols)), flush=True)
        return 0
    import numpy as np

    from oneflow_spmm import synth
    cfg = synth.CONFIGS["products"]
    m, nnz = cfg["m"] // args.scale, cfg["nnz"] // args.scale
    results = []
    with tempfile.TemporaryDirectory() as tmp:
        cols = os.path.join(tmp, "cols.npy")
        np.save(cols, synth.columns(m, m, synth.row_ptr(m, m, nnz), threads=16))
        print("columns generated", file=sys.stderr, flush=True)
        for step in STEPS:
            cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable,
                   os.path.abspath(__file__), "--step", step, "--reps", str(args.reps), "--scale",
                   str(args.scale), "--cols", cols]
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stderr.write(r.stderr[-2000:])
            if r.returncode != 0:
                print(f"step {step} failed with exit status {r.returncode}: the run ends here",
                      file=sys.stderr)
                return r.returncode
            line = r.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            results.append(json.loads(line))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"results": results}, f, indent=1)
        f.write("\n")
    if not all(r["bar_met"] for r in results):
        print("BAR MISSED: a fused forward's median is not below the composition's", file=sys.stderr)
        return 3
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Times the GAT attention weights (ops "gat_softmax_csr_heads" / "_grad") at the bench's
products-shaped CSR (2,449,029 rows and columns, 123,718,280 nonzeros, int32, the synthetic
columns of oneflow_spmm.synth), f32 H=8, f32 H=4 and bf16 H=8, against two things on the same GPU
and tensors:

  * "torch": today's route on this library, leaky_relu(s_row[row_ids] + s_col[col_idx]) in torch
    followed by `edge_softmax`.  The row-id vector and the int64 column indices are built outside
    the timed window, which favours this baseline;
  * "floor": `edge_softmax` alone on a precomputed e [nnz, H], the floor the fused launch
    approaches.  Its ratio is recorded, not gated.

Also recorded without a bar: the training step (forward and backward through autograd) of
`gat_softmax` and of the torch route, each with gradients in s_row and s_col.

Bar (checked after the measurement, once the JSON is written): in every configuration the forward
median of gat_softmax is below the torch route's.

Protocol (scripts/heads_bench.py): HIP events around each call, 3 warm-up rounds, median (and
minimum) of --reps runs, the candidates alternating round by round in one process.  Run without
--step the script is the driver: every configuration is a child process of its own under
`timeout -k 10`, and the first step that fails ends the run.
Results: one JSON line per step, and profiles/gat_softmax_bench.json."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "of-spmm_amd"), ROOT, os.path.join(ROOT, "scripts")]

STEPS = {"f32_h8": ("f32", 8), "f32_h4": ("f32", 4), "bf16_h8": ("bf16", 8)}
STEP_SECONDS = 420
SLOPE = 0.2


def run_step(name, reps, scale):
    import torch

    import oneflow_spmm as flow_spmm
    from heads_bench import timed
    from oneflow_spmm import _C, synth
    dtn, h = STEPS[name]
    cfg = synth.CONFIGS["products"]
    m, nnz = cfg["m"] // scale, cfg["nnz"] // scale
    k = m
    dt = {"f32": torch.float32, "bf16": torch.bfloat16}[dtn]
    bits = torch.int16 if dtn == "bf16" else torch.int32
    dev = torch.device("cuda", 0)
    rp_h = synth.row_ptr(m, k, nnz)
    ci = torch.from_numpy(synth.columns(m, k, rp_h, threads=16)).to(dev)
    rp = torch.from_numpy(rp_h).to(torch.int32).to(dev)
    # outside every timed window: the row-id vector and int64 columns of the torch route
    row_ids = torch.repeat_interleave(torch.arange(m, device=dev), torch.diff(rp.long()))
    cols = ci.long()
    gen = torch.Generator(device=dev).manual_seed(1)
    s_row = torch.randn(m, h, device=dev, generator=gen).mul_(2).to(dt)
    s_col = torch.randn(k, h, device=dev, generator=gen).mul_(2).to(dt)
    g = torch.randn(nnz, h, device=dev, generator=gen).to(dt)
    attn, attn_t, attn_f = (torch.empty(nnz, h, dtype=dt, device=dev) for _ in range(3))

    def gather(s, idx):
        """s[idx].  Rows of 16 bytes (f32 H=4, bf16 H=8) are gathered in pieces of 2^25 indices:
        with torch 2.10.0+rocm7.0 a single call on this many indices returned zeros for the last
        2^26 rows (s[idx], index_select and embedding alike; 32-byte rows are gathered correctly)."""
        if s.shape[1] * s.element_size() >= 32:
            return s[idx]
        piece = 1 << 25
        if s.requires_grad:
            return torch.cat([s[idx[i:i + piece]] for i in range(0, idx.numel(), piece)])
        out = torch.empty((idx.numel(), s.shape[1]), dtype=s.dtype, device=s.device)
        for i in range(0, idx.numel(), piece):
            torch.index_select(s, 0, idx[i:i + piece], out=out[i:i + piece])
        return out

    def torch_scores(sr, sc):
        return torch.nn.functional.leaky_relu(gather(sr, row_ids) + gather(sc, cols), SLOPE)

    # ---- the candidates compute the same thing ---------------------------------------------------
    e = torch_scores(s_row, s_col)
    _C.gat_softmax_csr_heads(rp, ci, s_row, s_col, SLOPE, out=attn)
    _C.edge_softmax_csr_heads(rp, ci, e, out=attn_t)
    if dtn == "f32":  # torch's f32 add, select and multiply are the contract's: the same bits
        assert torch.equal(attn.view(bits), attn_t.view(bits)), "gat_softmax != the torch route"
    else:  # torch rounds the sum to bf16 before the activation: one more rounding
        assert torch.allclose(attn.float(), attn_t.float(), rtol=0, atol=2e-2)

    t = timed({
        "fwd_gat": lambda: _C.gat_softmax_csr_heads(rp, ci, s_row, s_col, SLOPE, out=attn),
        "fwd_torch": lambda: _C.edge_softmax_csr_heads(rp, ci, torch_scores(s_row, s_col),
                                                       out=attn_t),
        "fwd_floor": lambda: _C.edge_softmax_csr_heads(rp, ci, e, out=attn_f),
    }, reps)

    a_row, a_col = (x.clone().requires_grad_(True) for x in (s_row, s_col))
    b_row, b_col = (x.clone().requires_grad_(True) for x in (s_row, s_col))

    def step_gat():
        a_row.grad = a_col.grad = None
        flow_spmm.gat_softmax(rp, ci, a_row, a_col, SLOPE).backward(g)

    def step_torch():
        b_row.grad = b_col.grad = None
        flow_spmm.edge_softmax(rp, ci, torch_scores(b_row, b_col)).backward(g)

    t.update(timed({
        "bwd_gat": lambda: _C.gat_softmax_csr_heads_grad(rp, ci, s_row, s_col, attn, g, SLOPE),
        "bwd_floor": lambda: _C.edge_softmax_csr_heads_grad(rp, ci, attn, g),
        "step_gat": step_gat,
        "step_torch": step_torch,
    }, reps))
    # the torch route sums with atomics in T: recorded, and checked where T is f32
    grad_diff = {"d_s_row": float((a_row.grad.float() - b_row.grad.float()).abs().max()),
                 "d_s_col": float((a_col.grad.float() - b_col.grad.float()).abs().max())}
    assert dtn != "f32" or max(grad_diff.values()) < 1e-2, grad_diff

    def rec(key):
        return {"median_ms": round(t[key][0], 4), "min_ms": round(t[key][1], 4)}

    res = {"step": name, "device": torch.cuda.get_device_name(0), "dtype": dtn, "heads": h, "m": m,
           "k": k, "nnz": nnz, "reps": reps, "negative_slope": SLOPE,
           "timings": {key: rec(key) for key in t}, "step_grad_max_abs_diff": grad_diff}
    res["ratios"] = {
        "fwd_gat_over_torch": round(t["fwd_gat"][0] / t["fwd_torch"][0], 3),
        "fwd_gat_over_floor": round(t["fwd_gat"][0] / t["fwd_floor"][0], 3),
        "bwd_gat_over_floor": round(t["bwd_gat"][0] / t["bwd_floor"][0], 3),
        "step_gat_over_torch": round(t["step_gat"][0] / t["step_torch"][0], 3)}
    res["accepted"] = t["fwd_gat"][0] < t["fwd_torch"][0]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=list(STEPS), help="run one step in this process (the driver's child)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scale", type=int, default=1, help="divide the problem's m and nnz (rehearsal)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gat_softmax_bench.json"))
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
        print("BAR MISSED: gat_softmax's forward median is not below the torch route's",
              file=sys.stderr)
        return 3
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Times the GATv2 attention scores (ops "gatv2_scores_csr_heads" / "_grad") at f32 H=4 D=16,
f32 H=8 D=16 and bf16 H=8 D=32 on the bench's synthetic CSRs (oneflow_spmm.synth, int32): the
products-shaped one (2,449,029 rows, 123,718,280 nonzeros) where the baseline's [nnz, H*D] tensors
fit in memory (f32 H=4 D=16: 31.7 GB each), and the 1M x 1M / 20M-nonzero power-law one for every
configuration.  Candidates, on the same GPU and tensors:

  * "gatv2": `gatv2_scores`, one launch;
  * "torch": today's route through existing code only: U = leaky_relu(x_row[row_ids] +
    x_col[col_idx]) in torch (gathered in pieces of 2^25 indices into one buffer, added and
    activated in place, which favours this baseline), then `sddmm_csr_heads` on (row_ptr,
    arange(nnz)) with att repeated per row.  The row-id vector, the int64 columns, arange and the
    repeated att are built outside the timed window;
  * "floor": `sddmm_csr_heads(rp, ci, x_row, x_col)` at the same shapes, which gathers the same
    bytes.  Its ratio is recorded, not gated.

Also recorded without a bar: the gradient launch (with p) against `spmm_csr_heads` at N = H*D, and,
on the 1M graph, a training step of `gatv2_attention` against the same layer over the torch route's
scores, with gradients in x_row, x_col and att.

Bar (checked after the measurement, once the JSON is written): in every step the forward median of
gatv2_scores is below the torch route's.

Protocol (scripts/heads_bench.py): HIP events around each call, 3 warm-up rounds, median (and
minimum) of --reps runs, the candidates alternating round by round in one process.  Run without
--step the script is the driver: every step is a child process of its own under `timeout -k 10`,
and the first step that fails ends the run.
Results: one JSON line per step, and profiles/gatv2_bench.json."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "of-spmm_amd"), ROOT, os.path.join(ROOT, "scripts")]

# step -> (graph, dtype, H, D, with the training step)
STEPS = {"plaw1m_f32_h4_d16": ("plaw1m", "f32", 4, 16, True),
         "plaw1m_f32_h8_d16": ("plaw1m", "f32", 8, 16, True),
         "plaw1m_bf16_h8_d32": ("plaw1m", "bf16", 8, 32, True),
         "products_f32_h4_d16": ("products", "f32", 4, 16, False)}
STEP_SECONDS = 420
SLOPE = 0.2
PIECE = 1 << 25  # indices per torch gather (one call over 2^26+ rows went wrong)


def run_step(name, reps, scale):
    import torch

    import oneflow_spmm as flow_spmm
    from heads_bench import timed
    from oneflow_spmm import _C, synth
    graph, dtn, h, d, train = STEPS[name]
    cfg = synth.CONFIGS[graph]
    m, nnz = cfg["m"] // scale, cfg["nnz"] // scale
    k, n = m, h * d
    dt = {"f32": torch.float32, "bf16": torch.bfloat16}[dtn]
    bits = torch.int16 if dtn == "bf16" else torch.int32
    dev = torch.device("cuda", 0)
    rp_h = synth.row_ptr(m, k, nnz)
    ci = torch.from_numpy(synth.columns(m, k, rp_h, threads=16)).to(dev)
    rp = torch.from_numpy(rp_h).to(torch.int32).to(dev)
    # outside every timed window: what the torch route needs besides the CSR
    row_ids = torch.repeat_interleave(torch.arange(m, device=dev), torch.diff(rp.long()))
    cols = ci.long()
    ident = torch.arange(nnz, dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    x_row = torch.randn(m, n, device=dev, generator=gen).to(dt)
    x_col = torch.randn(k, n, device=dev, generator=gen).to(dt)
    att = torch.randn(n, device=dev, generator=gen).to(dt)
    att_rows = att[None, :].repeat(m, 1)
    de = torch.randn(nnz, h, device=dev, generator=gen).to(dt)
    ones = torch.ones(nnz, h, dtype=dt, device=dev)
    e, e_t, e_f = (torch.empty(nnz, h, dtype=dt, device=dev) for _ in range(3))
    u_buf = torch.empty(nnz, n, dtype=dt, device=dev)
    g_buf = torch.empty(PIECE, n, dtype=dt, device=dev)

    def torch_u():
        """U into u_buf: both gathers in pieces, the add and the activation in place."""
        for i in range(0, nnz, PIECE):
            j = min(nnz, i + PIECE)
            torch.index_select(x_row, 0, row_ids[i:j], out=u_buf[i:j])
            torch.index_select(x_col, 0, cols[i:j], out=g_buf[:j - i])
            u_buf[i:j].add_(g_buf[:j - i])
        return torch.nn.functional.leaky_relu_(u_buf, SLOPE)

    def torch_scores(out):
        return _C.sddmm_csr_heads(rp, ident, att_rows, torch_u(), h, out=out)

    # ---- the candidates compute the same thing ---------------------------------------------------
    _C.gatv2_scores_csr_heads(rp, ci, x_row, x_col, att, h, SLOPE, out=e)
    torch_scores(e_t)
    if dtn == "f32":  # torch's f32 add, select and multiply are the contract's: the same bits
        assert torch.equal(e.view(bits), e_t.view(bits)), "gatv2_scores != the torch route"
    else:  # torch rounds the sum to bf16 before the activation: one more rounding per element
        assert torch.allclose(e.float(), e_t.float(), rtol=2e-2, atol=0.25)

    t = timed({
        "fwd_gatv2": lambda: _C.gatv2_scores_csr_heads(rp, ci, x_row, x_col, att, h, SLOPE, out=e),
        "fwd_torch": lambda: torch_scores(e_t),
        "fwd_floor": lambda: _C.sddmm_csr_heads(rp, ci, x_row, x_col, h, out=e_f),
    }, reps)
    # the gradient launch against the multi-head SpMM at N = H * D (u_buf: any [nnz, N] operand)
    sp_out = torch.empty(m, n, dtype=dt, device=dev)
    t.update(timed({
        "bwd_gatv2": lambda: _C.gatv2_scores_csr_heads_grad(rp, ci, x_row, x_col, att, de, h, SLOPE,
                                                            True),
        "bwd_gatv2_no_p": lambda: _C.gatv2_scores_csr_heads_grad(rp, ci, x_row, x_col, att, de, h,
                                                                 SLOPE, False),
        "bwd_spmm": lambda: _C.spmm_csr_heads(rp, ci, ones, m, k, x_col, out=sp_out),
    }, reps))
    del u_buf, g_buf

    grad_diff = None
    if train:
        a = [x.clone().view(s).requires_grad_(True)
             for x, s in ((x_row, (m, h, d)), (x_col, (k, h, d)), (att, (h, d)))]
        b = [x.clone().requires_grad_(True) for x in (x_row, x_col, att)]
        w = torch.randn(m, h, d, device=dev, generator=gen).to(dt)

        def step_gatv2():
            for x in a:
                x.grad = None
            flow_spmm.gatv2_attention(rp, ci, *a, SLOPE).backward(w)

        def step_torch():
            for x in b:
                x.grad = None
            u = torch.nn.functional.leaky_relu(b[0][row_ids] + b[1][cols], SLOPE)
            s = flow_spmm.sddmm(rp, ident, b[2][None, :].expand(m, n).reshape(m, h, d),
                                u.view(nnz, h, d))
            attn = flow_spmm.edge_softmax(rp, ci, s)
            flow_spmm.spmm(rp, ci, attn, m, k, b[1].view(k, h, d)).backward(w)

        t.update(timed({"step_gatv2": step_gatv2, "step_torch": step_torch}, reps))
        # the torch route sums with atomics in T: recorded, and checked where T is f32
        grad_diff = {nm: float((x.grad.float().reshape(-1) - y.grad.float().reshape(-1)).abs().max())
                     for nm, x, y in zip(("d_x_row", "d_x_col", "d_att"), a, b)}
        scale_of = max(float(x.grad.float().abs().max()) for x in a[:2])
        assert dtn != "f32" or max(grad_diff["d_x_row"], grad_diff["d_x_col"]) < 1e-3 * (1 + scale_of), \
            grad_diff

    def rec(key):
        return {"median_ms": round(t[key][0], 4), "min_ms": round(t[key][1], 4)}

    res = {"step": name, "device": torch.cuda.get_device_name(0), "graph": graph, "dtype": dtn,
           "heads": h, "d": d, "m": m, "k": k, "nnz": nnz, "reps": reps, "negative_slope": SLOPE,
           "timings": {key: rec(key) for key in t}, "step_grad_max_abs_diff": grad_diff}
    res["ratios"] = {
        "fwd_gatv2_over_torch": round(t["fwd_gatv2"][0] / t["fwd_torch"][0], 3),
        "fwd_gatv2_over_floor": round(t["fwd_gatv2"][0] / t["fwd_floor"][0], 3),
        "bwd_gatv2_over_spmm": round(t["bwd_gatv2"][0] / t["bwd_spmm"][0], 3),
        "bwd_gatv2_no_p_over_spmm": round(t["bwd_gatv2_no_p"][0] / t["bwd_spmm"][0], 3)}
    if train:
        res["ratios"]["step_gatv2_over_torch"] = round(t["step_gatv2"][0] / t["step_torch"][0], 3)
    res["accepted"] = t["fwd_gatv2"][0] < t["fwd_torch"][0]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=list(STEPS), help="run one step in this process (the driver's child)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scale", type=int, default=1, help="divide the problem's m and nnz (rehearsal)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gatv2_bench.json"))
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
        print("BAR MISSED: gatv2_scores's forward median is not below the torch route's",
              file=sys.stderr)
        return 3
    return 0


if __name__ == "__main__":
    sys.exit(main())

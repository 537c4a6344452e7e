#!/usr/bin/env python3
"""Times the multi-head ops "spmm_csr_heads" / "sddmm_csr_heads" and their gradients at the
bench's products-shaped CSR (2,449,029 rows, 123,718,280 nonzeros, int32), f32 H=8 D=16, f32 H=4
D=32 and bf16 H=8 D=32, each against two things on the same GPU and tensors:

  * the per-head loop through the existing public API (spmm / sddmm per head on b[:, h, :] views),
    reported twice: "packed" starts from the packed tensors a user of the multi-head layout holds
    (the values[:, h].contiguous() copies, and for the SDDMM the stack of the H results, inside the
    timed window; in the gradients also autograd's scatter back into the packed gradients), and
    "hoisted" has every per-head operand contiguous beforehand and writes / returns per-head
    results (the loop's best case: it still makes H launches, re-reads row_ptr and col_idx per
    head and gathers D-wide pieces of the B rows);
  * the single-head op at N = H*D with [nnz] values: the same gather bytes, (H-1)*nnz*sizeof(T)
    fewer value bytes.  Its ratio is recorded with the byte model, not gated.

Acceptance (asserted after the measurement): in every configuration the multi-head op's median is
not above the hoisted loop's median, for the two forwards and the two gradients.

The gradients run as in a training step: the cache of values gathered for A^T is emptied before
every timed call (new_step below).

Protocol (scripts/edge_softmax_bench.py): HIP events around each call, 3 warm-up rounds, median
(and minimum) of --reps runs, the candidates alternating round by round in one process.
Achieved bytes/s are over the algorithmic bytes (bytes_model below).  Run without --step the
script is the driver: the graph's columns are generated once on the host, every configuration is a
child process of its own under `timeout -k 10`, and the first step that fails ends the run.
Results: one JSON line per step, and profiles/heads_bench.json."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "of-spmm_amd"), ROOT]

STEPS = {"f32_h8_d16": ("f32", 8, 16), "f32_h4_d32": ("f32", 4, 32), "bf16_h8_d32": ("bf16", 8, 32)}
STEP_SECONDS = 420


def timed(fns, reps, warmup=3, prep=None):
    """{name: (median ms, min ms)} of the callables, alternating round by round; `prep` runs
    before every call, outside its timed window."""
    import numpy as np
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    prep = prep or (lambda: None)
    for _ in range(warmup):
        for fn in fns.values():
            prep()
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            prep()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return {k: (float(np.median(t)), float(np.min(t))) for k, t in ts.items()}


def bytes_model(m, k, nnz, h, d, sv, si):
    """Algorithmic bytes of one launch (every operand once; gathered B rows once per nonzero)."""
    n = h * d
    csr = nnz * si + (m + 1) * si
    gather = nnz * n * sv
    spmm = lambda hv, launches: gather + launches * csr + nnz * hv * sv + m * n * sv  # noqa: E731
    sddmm = lambda hv, launches: gather + launches * csr + nnz * hv * sv + m * n * sv  # noqa: E731
    fwd = {"spmm_heads": spmm(h, 1), "spmm_loop": spmm(h, h), "spmm_single": spmm(1, 1),
           "sddmm_heads": sddmm(h, 1), "sddmm_loop": sddmm(h, h), "sddmm_single": sddmm(1, 1)}
    # a gradient pair = one SDDMM + one SpMM on the transpose (k rows), plus the values gathered
    # through perm (read + write + perm) for the multi-head op
    perm = lambda hv: 2 * nnz * hv * sv + nnz * si  # noqa: E731
    tr = lambda hv, launches: gather + launches * csr + nnz * hv * sv + k * n * sv  # noqa: E731
    out = dict(fwd)
    for name, hv, launches in (("heads", h, 1), ("loop", h, h), ("single", 1, 1)):
        out[f"spmm_grad_{name}"] = sddmm(hv, launches) + tr(hv, launches) + perm(hv)
        out[f"sddmm_grad_{name}"] = spmm(hv, launches) + tr(hv, launches) + perm(hv)
    return out


def run_step(name, reps, scale, cols_path):
    import numpy as np
    import torch

    import oneflow_spmm as fs
    from oneflow_spmm import _C, synth
    dtn, h, d = STEPS[name]
    cfg = synth.CONFIGS["products"]
    m, nnz = cfg["m"] // scale, cfg["nnz"] // scale
    k, n = m, h * d
    dt = {"f32": torch.float32, "bf16": torch.bfloat16}[dtn]
    dev = torch.device("cuda", 0)
    rp_h = synth.row_ptr(m, k, nnz)
    ci_h = np.load(cols_path) if cols_path else synth.columns(m, k, rp_h, threads=16)
    rp = torch.from_numpy(rp_h.astype("int32")).to(dev)
    ci = torch.from_numpy(ci_h).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.rand(*s, device=dev, generator=gen).mul_(2).sub_(1).to(dt)  # noqa: E731
    vals, b2, a2, g2, ge = rnd(nnz, h), rnd(k, n), rnd(m, n), rnd(m, n), rnd(nnz, h)
    b3, a3, g3 = b2.view(k, h, d), a2.view(m, h, d), g2.view(m, h, d)
    vals1 = vals[:, 0].contiguous()
    vh = [vals[:, i].contiguous() for i in range(h)]
    geh = [ge[:, i].contiguous() for i in range(h)]
    out2 = torch.empty((m, n), dtype=dt, device=dev)
    out3 = out2.view(m, h, d)
    sd = torch.empty((nnz, h), dtype=dt, device=dev)

    # ---- the candidates compute the same thing ---------------------------------------------------
    ref = _C.spmm_csr_heads(rp, ci, vals, m, k, b2).clone()
    for i in range(h):
        fs.spmm(rp, ci, vh[i], m, k, b3[:, i, :], out=out3[:, i, :])
    assert torch.equal(ref.view(torch.int16 if dtn == "bf16" else torch.int32),
                       out2.view(torch.int16 if dtn == "bf16" else torch.int32)), "spmm heads != loop"
    ref_sd = _C.sddmm_csr_heads(rp, ci, a2, b2, h)
    loop_sd = torch.stack([fs.sddmm(rp, ci, a3[:, i, :], b3[:, i, :]) for i in range(h)], 1)
    assert torch.equal(ref_sd.view(torch.int16 if dtn == "bf16" else torch.int32),
                       loop_sd.view(torch.int16 if dtn == "bf16" else torch.int32)), "sddmm heads != loop"
    del ref, ref_sd, loop_sd

    # ---- forwards -------------------------------------------------------------------------------
    def spmm_loop_packed():
        for i in range(h):
            fs.spmm(rp, ci, vals[:, i].contiguous(), m, k, b3[:, i, :], out=out3[:, i, :])

    def spmm_loop_hoisted():
        for i in range(h):
            fs.spmm(rp, ci, vh[i], m, k, b3[:, i, :], out=out3[:, i, :])

    t = timed({
        "spmm_heads": lambda: _C.spmm_csr_heads(rp, ci, vals, m, k, b2, out=out2),
        "spmm_loop_packed": spmm_loop_packed, "spmm_loop_hoisted": spmm_loop_hoisted,
        "spmm_single": lambda: fs.spmm(rp, ci, vals1, m, k, b2, out=out2),
        "sddmm_heads": lambda: _C.sddmm_csr_heads(rp, ci, a2, b2, h, out=sd),
        "sddmm_loop_packed": lambda: torch.stack(
            [fs.sddmm(rp, ci, a3[:, i, :], b3[:, i, :]) for i in range(h)], 1),
        "sddmm_loop_hoisted": lambda: [fs.sddmm(rp, ci, a3[:, i, :], b3[:, i, :]) for i in range(h)],
        "sddmm_single": lambda: fs.sddmm(rp, ci, a2, b2),
    }, reps)

    # ---- gradients (autograd through the public entry points) -----------------------------------
    def leaf(x):
        return x.detach().clone().requires_grad_(True)

    v_l, b_l, a_l = leaf(vals), leaf(b3), leaf(a3)
    o_heads = fs.spmm(rp, ci, v_l, m, k, b_l)
    e_heads = fs.sddmm(rp, ci, a_l, b_l)
    vp, bp, ap = leaf(vals), leaf(b3), leaf(a3)  # the loop from packed leaves
    o_packed = [fs.spmm(rp, ci, vp[:, i].contiguous(), m, k, bp[:, i, :]) for i in range(h)]
    e_packed = [fs.sddmm(rp, ci, ap[:, i, :], bp[:, i, :]) for i in range(h)]
    vhl = [leaf(x) for x in vh]                  # the loop from per-head contiguous leaves
    bhl = [leaf(b3[:, i, :].contiguous()) for i in range(h)]
    ahl = [leaf(a3[:, i, :].contiguous()) for i in range(h)]
    g3h = [g3[:, i, :].contiguous() for i in range(h)]
    o_hoist = [fs.spmm(rp, ci, vhl[i], m, k, bhl[i]) for i in range(h)]
    e_hoist = [fs.sddmm(rp, ci, ahl[i], bhl[i]) for i in range(h)]
    v1, b1, a1 = leaf(vals1), leaf(b2), leaf(a2)
    o_single, e_single = fs.spmm(rp, ci, v1, m, k, b1), fs.sddmm(rp, ci, a1, b1)
    grad = torch.autograd.grad

    def new_step():
        # In training the attention weights and the upstream gradients are new every step, so the
        # autograd's cache of values gathered for A^T (autograd.py _TransposeCache: a copy kept
        # for values met twice) never hits.  Repeating one backward would hit it, for whichever
        # candidates fit its four entries: it is emptied before every timed call, so the loop's
        # d(b) reads its values through perm inside the SpMM (ofx_spmm_csr_gathered) and the
        # multi-head op gathers its [nnz, H] rows, as both do in a real step.  A^T itself stays
        # cached (the graph is static).
        fs.autograd.TRANSPOSE_CACHE.value_entries.clear()
        fs.autograd.TRANSPOSE_CACHE.seen.clear()

    t.update(timed({
        "spmm_grad_heads": lambda: grad(o_heads, (v_l, b_l), g3, retain_graph=True),
        "spmm_grad_loop_packed": lambda: grad(o_packed, (vp, bp), g3h, retain_graph=True),
        "spmm_grad_loop_hoisted": lambda: grad(o_hoist, vhl + bhl, g3h, retain_graph=True),
        "spmm_grad_single": lambda: grad(o_single, (v1, b1), g2, retain_graph=True),
        "sddmm_grad_heads": lambda: grad(e_heads, (a_l, b_l), ge, retain_graph=True),
        "sddmm_grad_loop_packed": lambda: grad(e_packed, (ap, bp), geh, retain_graph=True),
        "sddmm_grad_loop_hoisted": lambda: grad(e_hoist, ahl + bhl, geh, retain_graph=True),
        "sddmm_grad_single": lambda: grad(e_single, (a1, b1), geh[0], retain_graph=True),
    }, reps, prep=new_step))

    model = bytes_model(m, k, nnz, h, d, vals.element_size(), rp.element_size())

    def rec(key):
        base = key.replace("_packed", "").replace("_hoisted", "")
        return {"median_ms": round(t[key][0], 4), "min_ms": round(t[key][1], 4),
                "algorithmic_bytes": model[base],
                "achieved_tbs": round(model[base] / (t[key][0] * 1e-3) / 1e12, 3)}

    res = {"step": name, "device": torch.cuda.get_device_name(0), "dtype": dtn, "heads": h, "d": d,
           "m": m, "nnz": nnz, "reps": reps, "timings": {key: rec(key) for key in t}}
    ratios = {}
    for op in ("spmm", "sddmm", "spmm_grad", "sddmm_grad"):
        hd = t[f"{op}_heads"][0]
        ratios[op] = {"heads_over_loop_hoisted": round(hd / t[f"{op}_loop_hoisted"][0], 3),
                      "heads_over_loop_packed": round(hd / t[f"{op}_loop_packed"][0], 3),
                      "heads_over_single": round(hd / t[f"{op}_single"][0], 3),
                      "bytes_heads_over_single": round(model[f"{op}_heads"] / model[f"{op}_single"], 3)}
    res["ratios"] = ratios
    res["accepted"] = all(r["heads_over_loop_hoisted"] <= 1.0 for r in ratios.values())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=list(STEPS), help="run one step in this process (the driver's child)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scale", type=int, default=1, help="divide the problem's m and nnz (rehearsal)")
    ap.add_argument("--cols", default="", help="a .npy of the graph's columns (the driver's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heads_bench.json"))
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
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"results": results}, f, indent=1)
        f.write("\n")
    if not all(r["accepted"] for r in results):
        print("ACCEPTANCE FAILED: a multi-head op's median is above the hoisted loop's",
              file=sys.stderr)
        return 3
    return 0


if __name__ == "__main__":
    sys.exit(main())

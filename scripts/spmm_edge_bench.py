#!/usr/bin/env python3
"""Times the SpMM over per-edge feature vectors (`spmm_edge`; ops "spmm_csr_edge" / "_grad_e" /
"_grad_b") at f32 N=64 and bf16 N=128 on the bench's synthetic CSRs (oneflow_spmm.synth, int32):
the products-shaped one (2,449,029 rows, 123,718,280 nonzeros; e is 31.7 GB) and the 1M x 1M /
20M-nonzero power-law one.  Candidates, on the same GPU and tensors, for mul and for add + relu:

  * "edge": `spmm_edge`, one launch; "step_edge": forward and backward with gradients in e and b;
  * "torch": today's route through existing code only: msg = act(b[col_idx] op e) in torch
    (gathered in pieces of 2^25 indices into one buffer, combined and activated in place, which
    favours this baseline), summed by `spmm` on (row_ptr, arange(nnz), ones).  The int64 columns,
    arange and the ones are built outside the timed window; "step_torch" is its autograd;
  * "spmm": plain `spmm` with scalar values on the same graph, for scale.  Its ratio is recorded,
    not gated (the bytes predict about 2x).

The training step is tried on every graph; where the torch route's autograd (about eight [nnz, N]
tensors beside e) runs out of device memory, that is recorded and spmm_edge's step is timed alone.

--ab LIB also runs the A/B of the e loads on the products-shaped graph: LIB is the library of
`make edge-ab` (plain instead of non-temporal loads).  Two libraries cannot share a process, so
whole processes alternate, three rounds each, the forwards alone; the medians of the rounds'
medians go under "ab_e_loads".

Bar (checked after the measurement, once the JSON is written): in every step the forward and the
training-step medians of spmm_edge are below the torch route's.

Protocol (scripts/heads_bench.py): HIP events around each call, 3 warm-up rounds, median (and
minimum) of --reps runs, the candidates alternating round by round in one process.  Run without
--step the script is the driver: every step is a child process of its own under `timeout -k 10`,
and the first step that fails ends the run.
Results: one JSON line per step, and profiles/spmm_edge_bench.json (--out)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "of-spmm_amd"), ROOT, os.path.join(ROOT, "scripts")]

# step -> (graph, dtype, N, with the training step)
STEPS = {"plaw1m_f32_n64": ("plaw1m", "f32", 64, True),
         "plaw1m_bf16_n128": ("plaw1m", "bf16", 128, True),
         "products_f32_n64": ("products", "f32", 64, True),
         "products_bf16_n128": ("products", "bf16", 128, True)}
AB_STEPS = ("products_f32_n64", "products_bf16_n128")
AB_ROUNDS = 3
STEP_SECONDS = 420
PIECE = 1 << 25  # indices per torch gather (one call over 2^26+ rows went wrong)
PAIRS = {"mul": ("mul", None), "add_relu": ("add", "relu")}


def run_step(name, reps, scale, fwd_only=False):
    """fwd_only: the two `spmm_edge` forwards alone (a round of the load A/B)."""
    import torch

    import oneflow_spmm as flow_spmm
    from heads_bench import timed
    from oneflow_spmm import _C, synth
    graph, dtn, n, train = STEPS[name]
    cfg = synth.CONFIGS[graph]
    m, nnz = cfg["m"] // scale, cfg["nnz"] // scale
    k = m
    dt = {"f32": torch.float32, "bf16": torch.bfloat16}[dtn]
    dev = torch.device("cuda", 0)
    rp_h = synth.row_ptr(m, k, nnz)
    ci = torch.from_numpy(synth.columns(m, k, rp_h, threads=16)).to(dev)
    rp = torch.from_numpy(rp_h).to(torch.int32).to(dev)
    cols = ci.long()
    ident = torch.arange(nnz, dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    b = torch.randn(k, n, device=dev, generator=gen).to(dt)
    e = torch.empty(nnz, n, dtype=dt, device=dev)
    for i in range(0, nnz, PIECE):  # in pieces: no f32 copy of the whole of a bf16 e
        e[i:i + PIECE] = torch.randn(min(PIECE, nnz - i), n, device=dev, generator=gen).to(dt)
    values = torch.randn(nnz, device=dev, generator=gen).to(dt)
    ones = torch.ones(nnz, dtype=dt, device=dev)
    out, out_t, out_s = (torch.empty(m, n, dtype=dt, device=dev) for _ in range(3))
    if fwd_only:
        t = timed({f"fwd_edge_{tag}": (lambda op=op, act=act: _C.spmm_csr_edge(rp, ci, e, m, k, b, op, act, out=out))
                   for tag, (op, act) in PAIRS.items()}, reps)
        return {"step": name, "lib": os.environ.get("OFX_SPMM_LIB") or "release",
                "timings": {key: round(v[0], 4) for key, v in t.items()}}
    msg = torch.empty(nnz, n, dtype=dt, device=dev)

    def torch_route(op, act, dst):
        for i in range(0, nnz, PIECE):
            j = min(nnz, i + PIECE)
            torch.index_select(b, 0, cols[i:j], out=msg[i:j])
            msg[i:j].mul_(e[i:j]) if op == "mul" else msg[i:j].add_(e[i:j])
        if act == "relu":
            torch.relu_(msg)
        return flow_spmm.spmm(rp, ident, ones, m, nnz, msg, out=dst)

    t, diffs = {}, {}
    for tag, (op, act) in PAIRS.items():
        _C.spmm_csr_edge(rp, ci, e, m, k, b, op, act, out=out)
        torch_route(op, act, out_t)
        # f32: the same operations in the same order (spmm's own sum); bf16: torch rounds alike
        diffs[tag] = float((out.float() - out_t.float()).abs().max())
        assert torch.equal(out, out_t), f"spmm_edge != the torch route ({tag}: {diffs[tag]})"
        t.update(timed({
            f"fwd_edge_{tag}": lambda: _C.spmm_csr_edge(rp, ci, e, m, k, b, op, act, out=out),
            f"fwd_torch_{tag}": lambda: torch_route(op, act, out_t),
            **({} if "fwd_spmm" in t else
               {"fwd_spmm": lambda: flow_spmm.spmm(rp, ci, values, m, k, b, out=out_s)}),
        }, reps))
    del msg

    torch_step_oom = False
    if train:
        w = torch.randn(m, n, device=dev, generator=gen).to(dt)
        pe, pb = e.requires_grad_(True), b.clone().requires_grad_(True)
        for tag, (op, act) in PAIRS.items():
            def step_edge():
                pe.grad = pb.grad = None
                flow_spmm.spmm_edge(rp, ci, pe, m, k, pb, op, act).backward(w)

            def step_torch():
                pe.grad = pb.grad = None
                x = pb[cols] * pe if op == "mul" else pb[cols] + pe
                x = torch.relu(x) if act == "relu" else x
                flow_spmm.spmm(rp, ident, ones, m, nnz, x).backward(w)

            cands = {f"step_edge_{tag}": step_edge, f"step_torch_{tag}": step_torch}
            if not torch_step_oom:
                # the torch route's autograd keeps about eight [nnz, N] tensors beside e: on the
                # products-shaped graph that may not fit, and then only spmm_edge's step is timed
                try:
                    step_torch()
                    torch.cuda.synchronize()
                except torch.OutOfMemoryError:
                    torch_step_oom = True
                pe.grad = pb.grad = None
                torch.cuda.empty_cache()
            if torch_step_oom:
                del cands[f"step_torch_{tag}"]
            t.update(timed(cands, reps))

    res = {"step": name, "device": torch.cuda.get_device_name(0), "graph": graph, "dtype": dtn,
           "n": n, "m": m, "k": k, "nnz": nnz, "reps": reps, "fwd_max_abs_diff": diffs,
           "torch_step_out_of_memory": torch_step_oom,
           "timings": {key: {"median_ms": round(v[0], 4), "min_ms": round(v[1], 4)}
                       for key, v in t.items()}}
    res["ratios"], res["accepted"] = {}, True
    for tag in PAIRS:
        for kind in ("fwd", "step") if train and not torch_step_oom else ("fwd",):
            r = t[f"{kind}_edge_{tag}"][0] / t[f"{kind}_torch_{tag}"][0]
            res["ratios"][f"{kind}_edge_over_torch_{tag}"] = round(r, 3)
            res["accepted"] = res["accepted"] and r < 1
        res["ratios"][f"fwd_edge_over_spmm_{tag}"] = round(t[f"fwd_edge_{tag}"][0] / t["fwd_spmm"][0], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=list(STEPS), help="run one step in this process (the driver's child)")
    ap.add_argument("--steps", default=",".join(STEPS), help="the driver's steps, comma-separated")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scale", type=int, default=1, help="divide the problem's m and nnz (rehearsal)")
    ap.add_argument("--fwd-only", action="store_true", help="with --step: a round of the load A/B")
    ap.add_argument("--ab", metavar="LIB", help="the driver also runs the A/B of the e loads against "
                    "this library (`make edge-ab`: plain instead of non-temporal loads)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spmm_edge_bench.json"))
    args = ap.parse_args()
    if args.step:
        print(json.dumps(run_step(args.step, args.reps, args.scale, args.fwd_only)), flush=True)
        return 0

    def child(step, extra=(), lib=None):
        """One step in a process of its own; None after a failure (which ends the run)."""
        cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__),
               "--step", step, "--reps", str(args.reps), "--scale", str(args.scale), *extra]
        env = dict(os.environ, **({"OFX_SPMM_LIB": os.path.abspath(lib)} if lib else {}))
        r = subprocess.run(cmd, capture_output=True, text=True, env=env)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            print(f"step {step} failed with exit status {r.returncode}: the run ends here",
                  file=sys.stderr)
            return None, r.returncode
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        return json.loads(line), 0

    results, ab = [], []
    for step in args.steps.split(","):
        res, rc = child(step)
        if res is None:
            return rc
        results.append(res)
    # The A/B of the e loads: the two libraries cannot share a process, so whole processes
    # alternate, AB_ROUNDS each; the median of the rounds' medians is compared.
    for step in AB_STEPS if args.ab else ():
        rounds = {"non_temporal": [], "plain": []}
        for _ in range(AB_ROUNDS):
            for form, lib in (("non_temporal", None), ("plain", args.ab)):
                res, rc = child(step, ("--fwd-only",), lib)
                if res is None:
                    return rc
                rounds[form].append(res["timings"])
        med = {form: {key: sorted(r[key] for r in rs)[len(rs) // 2] for key in rs[0]}
               for form, rs in rounds.items()}
        ab.append({"step": step, "rounds": rounds, "median_ms": med})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"results": results, "ab_e_loads": ab}, f, indent=1)
        f.write("\n")
    if not all(r["accepted"] for r in results):
        print("BAR MISSED: a median of spmm_edge is not below the torch route's", file=sys.stderr)
        return 3
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Times the multi-head SpMM over an FP8 feature table (op "spmm_csr_heads_fp8") against the
existing multi-head SpMM at H x D in {1x64, 1x128, 4x32, 8x16, 1x256} on the bench's synthetic CSRs
(oneflow_spmm.synth, int32): the products-shaped one (2,449,029 rows, 123,718,280 nonzeros) and the
1M x 1M / 20M-nonzero power-law one.  Candidates, on the same GPU, CSR and values:

  * "fp8_scaled":  (a)  `spmm_csr_heads_fp8` with b_scale, e4m3fn table, bf16 values and output;
  * "fp8":         (a') the same without b_scale;
  * "bf16":        (b)  `spmm_csr_heads` on the table converted to bf16, the same bf16 values;
  * "f32":         (c)  `spmm_csr_heads` on the table converted to f32, the same values in f32.

Each candidate is checked before it is timed: (a') has the bits of (b) (the table converts to bf16
exactly), (a) those of `spmm_csr_heads` on the scaled values rounded to bf16, (c) those of the FP8
op run in f32.

Bar (checked after the measurement, once the JSON is written): on the products-shaped graph at
1x128 the median of (a') is below the median of (b).  The cost of the scale gather, (a) over (a'),
and the narrow rows are recorded as measured.

Protocol (scripts/heads_bench.py): HIP events around each call, 3 warm-up rounds, median (and
minimum) of --reps runs, the candidates alternating round by round in one process.  Run without
--graph the script is the driver: each graph is a child process of its own under `timeout -k 10`,
and the first one that fails ends the run.
Results: one JSON line per graph and shape, and profiles/spmm_fp8_bench.json."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "of-spmm_amd"), ROOT, os.path.join(ROOT, "scripts")]

GRAPHS = ("products", "plaw1m")
SHAPES = ((1, 64), (1, 128), (4, 32), (8, 16), (1, 256))
GRAPH_SECONDS = 540


def run_graph(graph, reps, scale):
    import torch

    import oneflow_spmm as flow_spmm
    from heads_bench import timed
    from oneflow_spmm import _C, synth
    cfg = synth.CONFIGS[graph]
    m, nnz = cfg["m"] // scale, cfg["nnz"] // scale
    k = m
    dev = torch.device("cuda", 0)
    rp_h = synth.row_ptr(m, k, nnz)
    ci = torch.from_numpy(synth.columns(m, k, rp_h, threads=16)).to(dev)
    rp = torch.from_numpy(rp_h).to(torch.int32).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    results = []
    for h, d in SHAPES:
        n = h * d
        b_q, b_scale = flow_spmm.quantize_rows_fp8(torch.randn(k, n, device=dev, generator=gen))
        b16, b32 = b_q.to(torch.bfloat16), b_q.to(torch.float32)
        v16 = torch.randn(nnz, h, device=dev, generator=gen).to(torch.bfloat16)
        v32 = v16.float()
        out_a, out_a1, out_b = (torch.empty(m, n, dtype=torch.bfloat16, device=dev) for _ in range(3))
        out_c = torch.empty(m, n, dtype=torch.float32, device=dev)

        def a():
            return _C.spmm_csr_heads_fp8(rp, ci, v16, m, k, b_q, b_scale, out=out_a)

        def a1():
            return _C.spmm_csr_heads_fp8(rp, ci, v16, m, k, b_q, out=out_a1)

        def b():
            return _C.spmm_csr_heads(rp, ci, v16, m, k, b16, out=out_b)

        def c():
            return _C.spmm_csr_heads(rp, ci, v32, m, k, b32, out=out_c)

        # ---- every candidate against its reference ------------------------------------------------
        a(), a1(), b(), c()
        assert torch.equal(out_a1.view(torch.int16), out_b.view(torch.int16)), "(a') != (b)"
        v_scaled = (v32 * b_scale[ci.long()][:, None]).to(torch.bfloat16)
        ref_a = _C.spmm_csr_heads(rp, ci, v_scaled, m, k, b16)
        assert torch.equal(out_a.view(torch.int16), ref_a.view(torch.int16)), "(a) != its composition"
        ref_c = _C.spmm_csr_heads_fp8(rp, ci, v32, m, k, b_q)
        assert torch.equal(out_c.view(torch.int32), ref_c.view(torch.int32)), "(c) != the FP8 op in f32"
        del v_scaled, ref_a, ref_c

        t = timed({"fp8_scaled": a, "fp8": a1, "bf16": b, "f32": c}, reps)
        res = {"graph": graph, "device": torch.cuda.get_device_name(0), "heads": h, "d": d, "m": m,
               "k": k, "nnz": nnz, "reps": reps, "format": "e4m3fn",
               "timings": {key: {"median_ms": round(t[key][0], 4), "min_ms": round(t[key][1], 4)}
                           for key in t},
               "ratios": {"fp8_over_bf16": round(t["fp8"][0] / t["bf16"][0], 3),
                          "fp8_over_f32": round(t["fp8"][0] / t["f32"][0], 3),
                          "fp8_scaled_over_fp8": round(t["fp8_scaled"][0] / t["fp8"][0], 3)}}
        print(json.dumps(res), flush=True)
        results.append(res)
        del b_q, b_scale, b16, b32, v16, v32, out_a, out_a1, out_b, out_c
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", choices=GRAPHS, help="run one graph in this process (the driver's child)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scale", type=int, default=1, help="divide the problem's m and nnz (rehearsal)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spmm_fp8_bench.json"))
    args = ap.parse_args()
    if args.graph:
        run_graph(args.graph, args.reps, args.scale)
        return 0
    results = []
    for graph in GRAPHS:
        cmd = ["timeout", "-k", "10", str(GRAPH_SECONDS), sys.executable, os.path.abspath(__file__),
               "--graph", graph, "--reps", str(args.reps), "--scale", str(args.scale)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            print(f"graph {graph} failed with exit status {r.returncode}: the run ends here",
                  file=sys.stderr)
            return r.returncode
        for line in r.stdout.strip().splitlines():
            print(line, flush=True)
            results.append(json.loads(line))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"results": results}, f, indent=1)
        f.write("\n")
    gate = [r for r in results if r["graph"] == "products" and (r["heads"], r["d"]) == (1, 128)]
    if not gate or gate[0]["timings"]["fp8"]["median_ms"] >= gate[0]["timings"]["bf16"]["median_ms"]:
        print("BAR MISSED: spmm_fp8 without a scale is not below the bf16 multi-head SpMM on the "
              "products-shaped graph at N = 128", file=sys.stderr)
        return 3
    return 0


if __name__ == "__main__":
    sys.exit(main())

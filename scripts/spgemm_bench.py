#!/usr/bin/env python3
"""Times the CSR x CSR product (`spgemm`, csrc/spgemm.hip) in float32 with int32 indices on three
shapes built from the synthetic graphs of oneflow_spmm.synth:
  * "arxiv_sq":   A @ A on the arxiv-shaped graph (169,343 rows, 1,166,243 nonzeros);
  * "blocks":     block_2 @ block_1 of a two-layer `sample_blocks` mini-batch on the products-shaped
                  graph, 100,000 seeds, fanouts 10 and 10 (block_1 through `coo_to_csr` first);
  * "coarsen":    S^T @ (A @ S) on plaw1m with S the assignment of row i to cluster i mod (M / 16),
                  as its two calls, "coarsen_as" and "coarsen_st".
Per shape: sum ub (the partial products) and nnz_c from the kCPU kernel, the rows of each device
class, and the timings
  * "call":    `spgemm` on the GPU as a user calls it: allocations, both entries, the one read-back;
  * "count", "fill": the two C-ABI entries alone on preallocated buffers;
  * "pattern": the call without values;
  * "torch":   the route without this op: every partial product expanded with repeat_interleave,
               a gather and a multiply, then `coo_to_csr(merge_duplicates=True)`; checked against
               the kCPU kernel's arrays like the GPU call; left out above --max-products products;
  * "sparse_mm": torch.sparse.mm on two sparse_csr tensors, if this torch build runs it;
  * "cpu":     the kCPU kernel at 16 threads (wall clock).
Protocol (scripts/row_topk_bench.py): HIP events around each call, 3 warm-up rounds, median (and
minimum) of --reps runs, the GPU candidates alternating round by round in one process.  Results:
one JSON line, and profiles/spgemm_bench.json."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "of-spmm_amd"), ROOT, os.path.join(ROOT, "scripts")]

CPU_THREADS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=int, default=1, help="divide the problems' sizes (rehearsal)")
    ap.add_argument("--shapes", default="arxiv_sq,blocks,coarsen")
    ap.add_argument("--max-products", type=int, default=400_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spgemm_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import oneflow_spmm as fs
    from heads_bench import timed
    from oneflow_spmm import _C, _lib, synth
    dev = torch.device("cuda", 0)
    i32 = torch.int32
    idt, vdt = _C.dtype_code(i32), _C.dtype_code(torch.float32)

    def graph(m, nnz):
        rp = synth.row_ptr(m, m, nnz)
        ci = synth.columns(m, m, rp, threads=CPU_THREADS)
        rp, ci = torch.from_numpy(rp).to(i32), torch.from_numpy(ci).to(i32)
        # canonical rows: ascending, no duplicates (a valid B)
        row = torch.repeat_interleave(torch.arange(m, dtype=i32), (rp[1:] - rp[:-1]).long())
        rp, ci, _ = fs.coo_to_csr(row, ci, None, m, m)
        return rp, ci, values(ci.numel(), 1)

    def values(count, seed):
        return torch.randn(count, generator=torch.Generator().manual_seed(seed))

    def torch_route(a, b, m, n):
        rp_a, ci_a, va = a
        rp_b, ci_b, vb = b
        rp_bl, ci_al = rp_b.long(), ci_a.long()
        inside = ci_al < rp_b.numel() - 1
        row_a = torch.repeat_interleave(torch.arange(m, device=dev), (rp_a[1:] - rp_a[:-1]).long())[inside]
        ci_al, va = ci_al[inside], va[inside]
        cnt = rp_bl[ci_al + 1] - rp_bl[ci_al]
        ends = torch.cumsum(cnt, 0)
        q = torch.arange(int(ends[-1]), device=dev) + torch.repeat_interleave(rp_bl[ci_al] - (ends - cnt), cnt)
        return fs.coo_to_csr(torch.repeat_interleave(row_a, cnt).to(i32), ci_b[q],
                             torch.repeat_interleave(va, cnt) * vb[q], m, n, merge_duplicates=True)

    def measure(name, a_h, b_h, n):
        m, k = a_h[0].numel() - 1, b_h[0].numel() - 1
        deg_b = (b_h[0][1:] - b_h[0][:-1]).long()
        inside = a_h[1].long() < k
        products = int(deg_b[a_h[1].long()[inside]].sum())
        t0 = time.perf_counter()
        ref = fs.spgemm(*a_h, *b_h, n, num_threads=CPU_THREADS)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        a, b = [t.to(dev) for t in a_h], [t.to(dev) for t in b_h]
        got = fs.spgemm(*a, *b, n)
        assert all(torch.equal(g.cpu().view(i32), r.view(i32)) for g, r in zip(got, ref)), "GPU != kCPU"
        nnz_c = ref[1].numel()
        sizes = (m, k, n, a[1].numel(), b[1].numel())
        ws_bytes = ctypes.c_size_t(0)
        _lib.check(_lib.LIB.ofx_spgemm_workspace_size(idt, vdt, *sizes, ctypes.byref(ws_bytes)))
        ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8, device=dev)
        scalars = torch.zeros(2, dtype=torch.int64, device=dev)
        out_rp = torch.empty(m + 1, dtype=i32, device=dev)
        out_ci, out_v = torch.empty(nnz_c, dtype=i32, device=dev), torch.empty(nnz_c, device=dev)
        ptrs = [t.data_ptr() for t in (*a, *b)]

        def count():
            _lib.check(_lib.LIB.ofx_spgemm_count(
                _C.current_stream_handle(out_rp), idt, *sizes, ptrs[0], ptrs[1], ptrs[3], ptrs[4],
                out_rp.data_ptr(), scalars.data_ptr(), scalars.data_ptr() + 8, ws.data_ptr(), ws_bytes.value))

        def fill():
            _lib.check(_lib.LIB.ofx_spgemm_fill(
                _C.current_stream_handle(out_rp), idt, vdt, *sizes, nnz_c, *ptrs, out_rp.data_ptr(),
                out_ci.data_ptr(), out_v.data_ptr(), ws.data_ptr(), ws_bytes.value))

        count()
        fill()
        assert scalars.tolist() == [nnz_c, 0] and torch.equal(out_v.cpu().view(i32), ref[2].view(i32))
        classes = ws[12:28].view(i32).tolist()  # the list lengths in the head of the workspace
        fns = {"call": lambda: fs.spgemm(*a, *b, n), "count": count, "fill": fill,
               "pattern": lambda: fs.spgemm(a[0], a[1], None, b[0], b[1], None, n)}
        notes = {}
        if products <= args.max_products:
            route = torch_route(a, b, m, n)
            assert torch.equal(route[0].cpu(), ref[0]) and torch.equal(route[1].cpu(), ref[1])
            notes["torch_values_bit_equal"] = bool(torch.equal(route[2].cpu().view(i32), ref[2].view(i32)))
            assert torch.allclose(route[2].cpu(), ref[2], rtol=1e-4, atol=1e-4), "torch route != kCPU"
            del route
            fns["torch"] = lambda: torch_route(a, b, m, n)
        else:
            notes["torch"] = f"left out: {products} products above --max-products"
        try:
            sa, sb = (torch.sparse_csr_tensor(x[0], x[1], x[2], size=s) for x, s in ((a, (m, k)), (b, (k, n))))
            torch.sparse.mm(sa, sb)
            torch.cuda.synchronize()
            fns["sparse_mm"] = lambda: torch.sparse.mm(sa, sb)
        except Exception as err:  # noqa: BLE001
            notes["sparse_mm"] = f"not run by this torch build: {type(err).__name__}: {str(err)[:120]}"
        t = timed(fns, args.reps)
        t["cpu"] = (cpu_ms, cpu_ms)
        row = {"shape": name, "m": m, "k": k, "n": n, "nnz_a": sizes[3], "nnz_b": sizes[4],
               "products": products, "nnz_c": nnz_c, "nnz_c_over_products": round(nnz_c / max(products, 1), 4),
               "rows_narrow_wave_block_hub": classes,
               "products_per_s_call": round(products / (t["call"][0] * 1e-3), 0),
               "timings": {x: {"median_ms": round(v[0], 4), "min_ms": round(v[1], 4)} for x, v in t.items()},
               "call_over_torch": round(t["call"][0] / t["torch"][0], 3) if "torch" in t else None,
               "pattern_over_call": round(t["pattern"][0] / t["call"][0], 3), **notes}
        print(json.dumps(row), file=sys.stderr, flush=True)
        return row, ref

    rows = []
    shapes = args.shapes.split(",")
    if "arxiv_sq" in shapes:
        g = graph(169_343 // args.scale, 1_166_243 // args.scale)
        rows.append(measure("arxiv_sq", g, g, g[0].numel() - 1)[0])
    if "blocks" in shapes:
        cfg = synth.CONFIGS["products"]
        m = cfg["m"] // args.scale
        rp = synth.row_ptr(m, m, cfg["nnz"] // args.scale)
        ci = torch.from_numpy(synth.columns(m, m, rp, threads=CPU_THREADS)).to(i32).to(dev)
        rp = torch.from_numpy(rp).to(i32).to(dev)
        seeds = torch.randperm(m, generator=torch.Generator().manual_seed(0))[:100_000 // args.scale]
        b1, b2 = fs.sample_blocks(rp, ci, seeds.to(i32).to(dev), [10, 10])
        del rp, ci
        n1 = b1[3].numel()
        row1 = torch.repeat_interleave(torch.arange(b1[0].numel() - 1, device=dev), (b1[0][1:] - b1[0][:-1]).long())
        blk1 = fs.coo_to_csr(row1.to(i32), b1[1], None, b1[0].numel() - 1, n1)[:2]
        a_h = (b2[0].cpu(), b2[1].cpu(), values(b2[1].numel(), 2))
        b_h = (blk1[0].cpu(), blk1[1].cpu(), values(blk1[1].numel(), 3))
        rows.append(measure("blocks", a_h, b_h, n1)[0])
    if "coarsen" in shapes:
        cfg = synth.CONFIGS["plaw1m"]
        m = cfg["m"] // args.scale
        g = graph(m, cfg["nnz"] // args.scale)
        c = m // 16
        s = (torch.arange(m + 1, dtype=i32), (torch.arange(m) % c).to(i32), values(m, 4))
        row, a_s = measure("coarsen_as", g, s, c)
        rows.append(row)
        st = fs.coo_to_csr(s[1], torch.arange(m, dtype=i32), s[2], c, m)
        rows.append(measure("coarsen_st", st, a_s, c)[0])

    res = {"device": torch.cuda.get_device_name(0), "values": "float32", "idx": "int32",
           "reps": args.reps, "cpu_threads": CPU_THREADS, "scale": args.scale, "shapes": rows,
           "b_check_share": "not measured (needs a kernel trace)",
           "call_below_torch_on_every_shape": all(r["call_over_torch"] is None or r["call_over_torch"] < 1
                                                  for r in rows)}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""The C-ABI entries each public call invokes, and what bad inputs raise, as JSON: the record a
refactor of the Python layer (oneflow_spmm/_C.py, autograd.py, ops.py) must leave unchanged.

    python scripts/abi_call_trace.py --out new.json
    git worktree add /tmp/parent HEAD~1
    OFX_SPMM_LIB=$PWD/of-spmm_amd/oneflow_spmm/libofx_spmm.so \\
        python scripts/abi_call_trace.py --pkg /tmp/parent/of-spmm_amd --out old.json
    cmp old.json new.json

Every attribute of _lib.LIB is wrapped after import (the wrappers keep __name__, which the
two-phase call uses in its messages).  The problem is the smallest with empty rows: a 5-row CSR
with row lengths [0, 3, 1, 0, 2], K = 4, N = 8, H = 2, D = 4, f32 / int32.  Bad inputs to the
Python layer always use CPU tensors (they must raise before any kernel runs; a GPU is no place to
find out).  What the multi-head C-ABI entries themselves refuse (entry_errors) is asked on the
traced device, where the HIP entries and their workspace queries answer: the record a refactor of
those entries' host side must leave unchanged.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, K, N, H, D = 5, 4, 8, 2, 4


def problem(torch, dev):
    g = torch.Generator().manual_seed(5)
    r = lambda *s: (torch.rand(*s, generator=g) - 0.5).to(dev)  # noqa: E731
    rp = torch.tensor([0, 0, 3, 4, 4, 6], dtype=torch.int32, device=dev)
    ci = torch.tensor([0, 1, 3, 2, 1, 3], dtype=torch.int32, device=dev)
    return dict(rp=rp, ci=ci, v=r(6), b=r(K, N), a=r(M, N), g=r(M, N), bias=r(N), vh=r(6, H),
                bh=r(K, H, D), ah=r(M, H, D), gh=r(M, H, D), sr=r(M, H), sc=r(K, H), e=r(6),
                eh=r(6, H))


def good_calls(fs, torch, p):
    """[(label, thunk)] in a fixed order; the autograd steps repeat on unchanged values (second and
    third sight of the transpose cache) and once more after an in-place update."""
    rp, ci = p["rp"], p["ci"]
    leaf = lambda t: t.clone().requires_grad_(True)  # noqa: E731
    out = []
    add = lambda label, fn: out.append((label, fn))  # noqa: E731

    def steps(label, values, fn):
        """fn(values_leaf) runs forward + backward; 3 times, then once after values.mul_(2)."""
        vv = leaf(values)
        for i in (1, 2, 3):
            add(f"{label} step {i}", lambda: fn(vv))

        def updated():
            with torch.no_grad():
                vv.mul_(2)
            fn(vv)
        add(f"{label} after in-place update", updated)

    add("spmm", lambda: fs.spmm(rp, ci, p["v"], M, K, p["b"]))
    add("spmm again", lambda: fs.spmm(rp, ci, p["v"], M, K, p["b"]))
    add("spmm out=", lambda: fs.spmm(rp, ci, p["v"], M, K, p["b"], out=torch.empty_like(p["g"])))
    add("spmm static_csr", lambda: fs.spmm(rp, ci, p["v"], M, K, p["b"], static_csr=7))
    add("spmm strided b", lambda: fs.spmm(rp, ci, p["v"], M, K, p["b"][:, :5]))
    add("spmm_csr _parallel rows", lambda: fs.spmm_csr(rp, ci, p["v"], M, K, p["b"],
                                                       _parallel=(1, 2, 0)))
    steps("spmm backward", p["v"],
          lambda vv: fs.spmm(rp, ci, vv, M, K, leaf(p["b"])).backward(p["g"]))
    steps("spmm backward static_csr", p["v"],
          lambda vv: fs.spmm(rp, ci, vv, M, K, leaf(p["b"]), static_csr=9).backward(p["g"]))
    for red in ("sum", "mean", "max", "min"):
        add(f"spmm reduce={red}", lambda red=red: fs.spmm(rp, ci, p["v"], M, K, p["b"], reduce=red))
        add(f"spmm_reduce {red}", lambda red=red: fs.spmm_reduce(rp, ci, p["v"], M, K, p["b"], red))
        steps(f"spmm_reduce {red} backward", p["v"], lambda vv, red=red: fs.spmm_reduce(
            rp, ci, vv, M, K, leaf(p["b"]), red)[0].backward(p["g"]))
    add("spmm_csr_reduce _parallel", lambda: fs.spmm_csr_reduce(rp, ci, p["v"], M, K, p["b"], "max",
                                                                _parallel=(0, 2, 0)))
    for relu in (False, True):
        add(f"fused_spmm relu={relu}", lambda relu=relu: fs.fused_spmm(
            rp, ci, p["v"], M, K, p["b"], p["bias"], relu=relu))
        steps(f"fused_spmm relu={relu} backward", p["v"], lambda vv, relu=relu: fs.fused_spmm(
            rp, ci, vv, M, K, leaf(p["b"]), leaf(p["bias"]), relu=relu).backward(p["g"]))
    add("fused_spmm no bias", lambda: fs.fused_spmm(rp, ci, p["v"], M, K, p["b"]))
    add("sddmm", lambda: fs.sddmm(rp, ci, p["a"], p["b"]))
    steps("sddmm backward", p["a"], lambda aa: fs.sddmm(rp, ci, aa, leaf(p["b"])).backward(p["e"]))
    add("sddmm heads", lambda: fs.sddmm(rp, ci, p["ah"], p["bh"]))
    steps("sddmm heads backward", p["ah"],
          lambda aa: fs.sddmm(rp, ci, aa, leaf(p["bh"])).backward(p["eh"]))
    add("csr_transpose", lambda: fs.csr_transpose(rp, ci, K))
    add("spmm heads", lambda: fs.spmm(rp, ci, p["vh"], M, K, p["bh"]))
    add("spmm heads out=", lambda: fs.spmm(rp, ci, p["vh"], M, K, p["bh"],
                                           out=torch.empty_like(p["gh"])))
    steps("spmm heads backward", p["vh"],
          lambda vv: fs.spmm(rp, ci, vv, M, K, leaf(p["bh"])).backward(p["gh"]))
    for name, e in (("edge_softmax", p["e"]), ("edge_softmax heads", p["eh"])):
        add(name, lambda e=e: fs.edge_softmax(rp, ci, e))
        add(f"{name} out=", lambda e=e: fs.edge_softmax(rp, ci, e, out=torch.empty_like(e)))
        steps(f"{name} backward", e, lambda ee, e=e: fs.edge_softmax(rp, ci, ee).backward(e))
    add("graph_attention", lambda: fs.graph_attention(rp, ci, p["ah"], p["bh"], p["bh"]))
    add("graph_attention 2-D", lambda: fs.graph_attention(rp, ci, p["a"], p["b"], p["b"],
                                                          return_attention=True))
    steps("graph_attention backward", p["ah"], lambda qq: fs.graph_attention(
        rp, ci, qq, leaf(p["bh"]), leaf(p["bh"])).backward(p["gh"]))

    def attention_weights_only(qq):
        o, w = fs.graph_attention(rp, ci, qq, leaf(p["bh"]), leaf(p["bh"]), return_attention=True)
        w.backward(p["eh"])
    steps("graph_attention weights-only backward", p["ah"], attention_weights_only)
    add("gat_softmax", lambda: fs.gat_softmax(rp, ci, p["sr"], p["sc"]))
    add("gat_softmax 1-D out=", lambda: fs.gat_softmax(rp, ci, p["sr"][:, 0], p["sc"][:, 0],
                                                       out=torch.empty_like(p["e"])))
    steps("gat_softmax backward", p["sr"],
          lambda ss: fs.gat_softmax(rp, ci, ss, leaf(p["sc"])).backward(p["eh"]))
    add("gat_attention", lambda: fs.gat_attention(rp, ci, p["sr"], p["sc"], p["bh"]))
    steps("gat_attention backward", p["sr"], lambda ss: fs.gat_attention(
        rp, ci, ss, leaf(p["sc"]), leaf(p["bh"])).backward(p["gh"]))
    # the direct C-ABI forms of ops.py
    rt, ct, perm = fs.csr_transpose(rp, ci, K)
    ops, b2 = fs.ops, p["bh"].reshape(K, H * D)
    add("ops.spmm_csr_gathered", lambda: ops.spmm_csr_gathered(rt, ct, p["v"], perm, p["g"], K, M))
    add("ops.relu_bias_grad", lambda: ops.relu_bias_grad(p["g"], p["a"], relu=True, bias_grad=True))
    add("ops.spmm_csr_heads", lambda: ops.spmm_csr_heads(rp, ci, p["vh"], b2, M, K, H))
    add("ops.sddmm_csr_heads", lambda: ops.sddmm_csr_heads(rp, ci, p["ah"].reshape(M, H * D), b2,
                                                           M, K, H))
    add("ops.graph_attention_csr_heads", lambda: ops.graph_attention_csr_heads(
        rp, ci, p["ah"].reshape(M, H * D), b2, b2, M, K, H))
    add("_C.spmm_csr_gathered", lambda: fs._C.spmm_csr_gathered(rt, ct, p["v"], perm, K, M, p["g"]))
    # the GATv2 scores: the public entries, then ops.py's
    att = p["bias"].reshape(H, D)
    add("gatv2_scores", lambda: fs.gatv2_scores(rp, ci, p["ah"], p["bh"], att))
    steps("gatv2_scores backward", p["ah"], lambda xx: fs.gatv2_scores(
        rp, ci, xx, leaf(p["bh"]), leaf(att)).backward(p["eh"]))
    add("gatv2_attention", lambda: fs.gatv2_attention(rp, ci, p["ah"], p["bh"], att))
    a2 = p["ah"].reshape(M, H * D)
    add("ops.gatv2_scores_csr_heads", lambda: ops.gatv2_scores_csr_heads(
        rp, ci, a2, b2, p["bias"], M, K, H))
    for with_att in (True, False):
        add(f"ops.gatv2_scores_csr_heads_grad with_att={with_att}",
            lambda with_att=with_att: ops.gatv2_scores_csr_heads_grad(
                rp, ci, a2, b2, p["bias"], p["eh"], M, K, H, with_att=with_att))
    return out


def entry_errors(fs, torch, p):
    """[(label, thunk)]: what the multi-head entries of ops.py refuse, on the traced device's
    tensors (the HIP entry and its workspace query there, the kCPU entry on host tensors): bad
    heads / d, a workspace of one byte (ignored by the kCPU entries, which take none), planned /
    variant options, a leading dimension below n.
    Every refusal returns before a launch.  The rows here are long enough to need a workspace:
    row lengths [300, 1] (the per-nonzero ops cut their items at 256 nonzeros)."""
    ops, _lib, dev = fs.ops, fs._lib, p["rp"].device
    n, nnz = H * D, 301
    rp = torch.tensor([0, 300, 301], dtype=torch.int32, device=dev)
    ci = (torch.arange(nnz, dtype=torch.int32) % K).to(dev)
    g = torch.Generator().manual_seed(6)
    r = lambda *s: (torch.rand(*s, generator=g) - 0.5).to(dev)  # noqa: E731
    a, b, att, vh, eh = r(2, n), r(K, n), r(n), r(nnz, H), r(nnz, H)
    e_out, o_out = torch.empty_like(eh), torch.empty_like(a)
    split8 = ops.make_options(split=8, chunk=8)
    # op -> call(heads, a, b, **kw): kw are options= / workspace_bytes= where the op takes them
    entries = {
        "spmm_csr_heads": lambda heads, a, b, **kw: ops.spmm_csr_heads(
            rp, ci, vh, b, 2, K, heads, out=o_out, **kw),
        "sddmm_csr_heads": lambda heads, a, b, **kw: ops.sddmm_csr_heads(
            rp, ci, a, b, 2, K, heads, out=e_out, **kw),
        "graph_attention_csr_heads": lambda heads, a, b, **kw: ops.graph_attention_csr_heads(
            rp, ci, a, b, b, 2, K, heads, out=o_out, attn=e_out, **kw),
        "gatv2_scores_csr_heads": lambda heads, a, b, **kw: ops.gatv2_scores_csr_heads(
            rp, ci, a, b, att, 2, K, heads, out=e_out, **kw),
        "gatv2_scores_csr_heads_grad": lambda heads, a, b, **kw: ops.gatv2_scores_csr_heads_grad(
            rp, ci, a, b, att, eh, 2, K, heads, d_x=o_out, p=torch.empty_like(a), **kw),
        "gatv2_scores_csr_heads_grad no p": lambda heads, a, b, **kw:
            ops.gatv2_scores_csr_heads_grad(rp, ci, a, b, att, eh, 2, K, heads, with_att=False,
                                            d_x=o_out, **kw),
    }
    takes_options = lambda op: "sddmm" not in op and op != "gatv2_scores_csr_heads"  # noqa: E731
    out = []
    add = lambda label, fn: out.append((label, fn))  # noqa: E731
    for op, call in entries.items():
        add(f"{op}: good", lambda call=call: call(H, a, b))
        add(f"{op}: heads < 0", lambda call=call: call(-1, a, b))
        short = dict(workspace_bytes=1, **(dict(options=split8) if takes_options(op) else {}))
        add(f"{op}: workspace of one byte", lambda call=call, short=short: call(H, a, b, **short))
        add(f"{op}: ld < n", lambda call=call: call(H, a.as_strided((2, n), (n - 1, 1)),
                                                    b.as_strided((K, n), (n - 1, 1))))
        if takes_options(op):
            add(f"{op}: good, split 8", lambda call=call: call(H, a, b, options=split8))
            add(f"{op}: planned", lambda call=call: call(H, a, b, options=ops.make_options(planned=True)))
            add(f"{op}: variant", lambda call=call: call(H, a, b, options=ops.make_options(variant=1)))
    # the HIP entries' own refusal of heads * d (their workspace queries answer first above): no
    # pointer is read and nothing is launched, on any machine
    I, F, LIB = _lib.DT_INT32, _lib.DT_FLOAT, _lib.LIB
    big = 1 << 62
    direct = {
        "ofx_spmm_csr_heads": lambda: LIB.ofx_spmm_csr_heads(
            None, I, F, 2, K, big, 4, nnz, None, None, None, None, n, None, n, 0, 2, None, 0, None),
        "ofx_sddmm_csr_heads": lambda: LIB.ofx_sddmm_csr_heads(
            None, I, F, 2, K, big, 4, nnz, None, None, None, n, None, n, None, 0, 2, None, 0),
        "ofx_graph_attention_csr_heads": lambda: LIB.ofx_graph_attention_csr_heads(
            None, I, F, 2, K, big, 4, nnz, None, None, None, n, None, n, None, n, None, n, None, 0,
            2, None, 0, None),
        "ofx_gatv2_scores_csr_heads": lambda: LIB.ofx_gatv2_scores_csr_heads(
            None, I, F, 2, K, big, 4, nnz, None, None, None, n, None, n, None, 0.2, None, 0, 2,
            None, 0),
        "ofx_gatv2_scores_csr_heads_grad": lambda: LIB.ofx_gatv2_scores_csr_heads_grad(
            None, I, F, 2, K, big, 4, nnz, None, None, None, n, None, n, None, 0.2, None, None, n,
            None, n, 0, 2, None, 0, None),
    }
    for name, fn in direct.items():
        add(f"{name}: heads * d overflows", lambda fn=fn, name=name: _lib.check(fn(), name))
    size = ctypes.c_size_t(0)
    add("ofx_gatv2_scores_csr_heads_grad_workspace_size: 2 * heads * d overflows",
        lambda: _lib.check(LIB.ofx_gatv2_scores_csr_heads_grad_workspace_size(
            I, F, 2, K, 1 << 61, 3, nnz, 1, None, ctypes.byref(size)), "grad workspace_size"))
    return out


def bad_calls(fs, torch, p):
    """[(label, thunk)]: one call per raise of _C.py's check functions (for the shared
    _check_inputs: per op that calls it, every tensor it names) and of the autograd wrappers."""
    _C, rp, ci = fs._C, p["rp"], p["ci"]
    q2, k2 = p["ah"].reshape(M, H * D), p["bh"].reshape(K, H * D)
    y, yh = fs.edge_softmax(rp, ci, p["e"]), fs.edge_softmax(rp, ci, p["eh"])
    # op -> (call(rp, ci, **tensors), the tensors _check_inputs names, those with nnz rows)
    checked = {
        "edge_softmax_csr": (lambda r, c, e: _C.edge_softmax_csr(r, c, e), dict(e=p["e"]), "e"),
        "edge_softmax_csr_grad": (lambda r, c, y, dy: _C.edge_softmax_csr_grad(r, c, y, dy),
                                  dict(y=y, dy=p["e"]), "y dy"),
        "spmm_csr_heads": (lambda r, c, a_csr_values, b: _C.spmm_csr_heads(r, c, a_csr_values, M, K, b),
                           dict(a_csr_values=p["vh"], b=k2), "a_csr_values"),
        "sddmm_csr_heads": (lambda r, c, a, b: _C.sddmm_csr_heads(r, c, a, b, H),
                            dict(a=q2, b=k2), ""),
        "graph_attention_csr_heads": (lambda r, c, q, k, v: _C.graph_attention_csr_heads(r, c, q, k, v, H),
                                      dict(q=q2, k=k2, v=k2), ""),
        "edge_softmax_csr_heads": (lambda r, c, e: _C.edge_softmax_csr_heads(r, c, e),
                                   dict(e=p["eh"]), "e"),
        "edge_softmax_csr_heads_grad": (lambda r, c, y, dy: _C.edge_softmax_csr_heads_grad(r, c, y, dy),
                                        dict(y=yh, dy=p["eh"]), "y dy"),
        "gat_softmax_csr_heads": (lambda r, c, s_row, s_col: _C.gat_softmax_csr_heads(r, c, s_row, s_col),
                                  dict(s_row=p["sr"], s_col=p["sc"]), ""),
        "gat_softmax_csr_heads_grad": (
            lambda r, c, s_row, s_col, y, dy: _C.gat_softmax_csr_heads_grad(r, c, s_row, s_col, y, dy),
            dict(s_row=p["sr"], s_col=p["sc"], y=yh, dy=p["eh"]), "y dy"),
    }
    out = []
    add = lambda label, fn: out.append((label, fn))  # noqa: E731
    for op, (call, tensors, nnz_names) in checked.items():
        def variant(label, r=rp, c=ci, call=call, tensors=tensors, op=op, **changed):
            add(f"{op}: {label}", lambda: call(r, c, **{**tensors, **changed}))
        for name, t in tensors.items():
            variant(f"{name} rank", **{name: t.unsqueeze(-1)})
            variant(f"{name} dtype", **{name: t.double()})
            if name in nnz_names.split() or name == "s_row":
                variant(f"{name} rows", **{name: t[:-1]})
            if t.dim() == 2:
                variant(f"{name} heads", **{name: t[:, :1]})
        variant("not float", **{name: t.int() for name, t in tensors.items()})
        variant("index dtypes differ", c=ci.long())
        variant("index dtype unsupported", r=rp.short(), c=ci.short())
    good = torch.empty((6, H))
    add("_check_out: not contiguous", lambda: _C.edge_softmax_csr_heads(rp, ci, p["eh"], out=good.t().contiguous().t()))
    add("_check_out: shape", lambda: _C.edge_softmax_csr_heads(rp, ci, p["eh"], out=good[:-1]))
    add("_check_out: dtype", lambda: _C.spmm_csr_heads(rp, ci, p["vh"], M, K, k2, out=torch.empty((M, H * D)).double()))
    add("_prep: not a tensor", lambda: fs.spmm_csr(rp, ci, p["v"], M, K, None))
    add("dtype_code: unsupported", lambda: fs.spmm_csr(rp, ci, p["v"].to(torch.int8), M, K, p["b"]))
    add("desc: 3-D", lambda: fs.spmm_csr(rp, ci, p["v"], M, K, p["bh"]))
    add("reduce_code", lambda: fs.spmm_reduce(rp, ci, p["v"], M, K, p["b"], "prod"))
    add("graph_attention_csr_heads: q rows", lambda: _C.graph_attention_csr_heads(rp, ci, q2[:-1], k2, k2, H))
    add("graph_attention_csr_heads: v rows", lambda: _C.graph_attention_csr_heads(rp, ci, q2, k2, k2[:-1], H))
    # the autograd wrappers
    leaf = lambda t: t.clone().requires_grad_(True)  # noqa: E731
    add("sddmm: heads differ", lambda: fs.sddmm(rp, ci, p["ah"], p["bh"][:, :1]))
    add("_heads_2d", lambda: fs.autograd._heads_2d(p["b"], "b"))
    add("spmm heads: reduce", lambda: fs.spmm(rp, ci, p["vh"], M, K, p["bh"], reduce="max"))
    add("spmm heads: values", lambda: fs.spmm(rp, ci, p["v"], M, K, p["bh"]))
    add("spmm heads: out= with grad", lambda: fs.spmm(rp, ci, leaf(p["vh"]), M, K, p["bh"], out=torch.empty_like(p["gh"])))
    add("spmm heads: out shape", lambda: fs.spmm(rp, ci, p["vh"], M, K, p["bh"], out=torch.empty((M, H * D))))
    add("spmm: out= with grad", lambda: fs.spmm(rp, ci, leaf(p["v"]), M, K, p["b"], out=torch.empty_like(p["g"])))
    add("spmm_reduce: out= with grad", lambda: fs.spmm_reduce(rp, ci, p["v"], M, K, leaf(p["b"]), "max", out=torch.empty_like(p["g"])))
    add("fused_spmm: out= with grad", lambda: fs.fused_spmm(rp, ci, p["v"], M, K, p["b"], leaf(p["bias"]), out=torch.empty_like(p["g"])))
    add("edge_softmax: out= with grad", lambda: fs.edge_softmax(rp, ci, leaf(p["e"]), out=torch.empty_like(p["e"])))
    add("edge_softmax heads: out= with grad", lambda: fs.edge_softmax(rp, ci, leaf(p["eh"]), out=torch.empty_like(p["eh"])))
    add("graph_attention: ranks", lambda: fs.graph_attention(rp, ci, p["ah"], p["b"], p["b"]))
    add("graph_attention: shapes", lambda: fs.graph_attention(rp, ci, p["ah"], p["bh"], p["bh"][:, :1]))
    add("graph_attention: dtypes", lambda: fs.graph_attention(rp, ci, p["ah"].double(), p["bh"], p["bh"]))
    add("gat_softmax: ranks", lambda: fs.gat_softmax(rp, ci, p["sr"], p["sc"][:, 0]))
    add("gat_softmax: out= with grad", lambda: fs.gat_softmax(rp, ci, leaf(p["sr"]), p["sc"], out=torch.empty_like(p["eh"])))
    add("gat_softmax: 1-D out", lambda: fs.gat_softmax(rp, ci, p["sr"][:, 0], p["sc"][:, 0], out=torch.empty_like(p["eh"])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(ROOT, "of-spmm_amd"),
                    help="the directory that holds the oneflow_spmm package to trace")
    ap.add_argument("--device", default="cpu", choices=["cpu", "cuda"])
    ap.add_argument("--out", default="-")
    args = ap.parse_args()
    sys.path.insert(0, args.pkg)
    import torch
    import oneflow_spmm as fs
    from oneflow_spmm import _lib

    log: list = []
    for name in _lib.EXPORTED:
        def wrapper(*a, _raw=getattr(_lib.LIB, name), _name=name):
            log.append(_name)
            return _raw(*a)
        wrapper.__name__ = name
        setattr(_lib.LIB, name, wrapper)

    record = {"device": args.device, "calls": [], "errors": []}
    fs.autograd.TRANSPOSE_CACHE.__init__()
    for label, fn in good_calls(fs, torch, problem(torch, torch.device(args.device))):
        del log[:]
        fn()
        record["calls"].append([label, list(log)])
    fs.autograd.TRANSPOSE_CACHE.__init__()
    bad = bad_calls(fs, torch, problem(torch, torch.device("cpu"))) + \
        entry_errors(fs, torch, problem(torch, torch.device(args.device)))
    for label, fn in bad:
        del log[:]
        try:
            fn()
            what = ["no error", ""]
        except Exception as e:  # noqa: BLE001  (the type is the record)
            what = [type(e).__name__, str(e)]
        record["errors"].append([label, *what, list(log)])
    text = json.dumps(record, indent=1)
    if args.out == "-":
        print(text)
    else:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(f"{os.path.dirname(fs.__file__)}: {len(record['calls'])} calls,{len(record['errors'])} bad inputs "
          f"({sum(e[1] == 'no error' for e in record['errors'])} did not raise)", file=sys.stderr)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The data gradient for a block of cotangent rows per QP (ipmz_batch_data_vjp_multi) against the way without it: a
host loop of ipmz_batch_data_vjp over the rows.

    python tools/data_vjp_multi_bench.py [--shape 256:48:16] [--reps 15] [--out profiles/data_vjp_multi/bench.json]

C4's shape (n 256, m 48, p 16), the default formulation, the iterate after two steps, standard-normal cotangent rows;
ncot in 2, 4, 16, 64; blocks shared by the batch at batch 1024 and per-QP blocks at batch 128 (the output of 64 rows
stays within a few GB).  Two legs, alternated in one process after a warm-up of both, timed with device events:

  multi  Optimizer.data_grad_tensors_multi: nine fresh tensors and one ipmz_batch_data_vjp_multi
  loop   ncot times Optimizer.data_grad_tensors on W[:, r]: nine fresh tensors and one ipmz_batch_data_vjp each

Before any time is reported the two legs' results are compared bitwise (the row contract).  Medians over the
repetitions and max - min as the spread.  --layer adds the layer's figure: layer.solution_vjp (one factor) against
ncot backward passes of layer.solve_qp (one factor each) at batch 128, ncot 16.  Kernel times come from a rocprofv3
--kernel-trace run of this tool with --trace-only (shared blocks, batch 1024, ncot 16: the new call twice, then the
loop), added to the document with --summarize.  There is no CPU fallback.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ipm-zoo_amd"))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))

KERNELS = ("k_grad_matrix<", "k_grad_vectors(", "k_grad_vectors_shared(", "k_grad_shared_part<", "k_grad_shared_sum(")
NAMES = ("Q", "c", "l_x", "u_x", "A_ineq", "l_A_ineq", "u_A_ineq", "A_eq", "b_eq")
NCOTS = (2, 4, 16, 64)
SLAB = 16  # csrc/kernels.h IPMZ_VJP_SLAB
TRACE_B, TRACE_NCOT = 1024, 16
LAYER_B, LAYER_NCOT = 128, 16


def summarize_trace(path):
    """A --trace-only run: the launches in time order are those of the new call (warm-up), of the new call again
    (read) and of the loop's TRACE_NCOT single-row calls (all read, the first of them included)."""
    import csv
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if any(k in r["Kernel_Name"] for k in KERNELS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    multi = 3 * 2 * -(-TRACE_NCOT // SLAB) + 1  # (part, sum) per matrix block and slab, one shared-vector launch
    single = 3 * 2 + 1
    assert len(rows) == 2 * multi + TRACE_NCOT * single, (len(rows), multi, single)

    def total(rs):
        out = {}
        for r in rs:
            k = next(k for k in KERNELS if k in r["Kernel_Name"]).rstrip("<(")
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            out.setdefault(k, {"launches": 0, "us": 0.0})
            out[k]["launches"] += 1
            out[k]["us"] += us
        out["sum_us"] = sum(v["us"] for v in out.values())
        return out

    return {"batch": TRACE_B, "ncot": TRACE_NCOT, "layout": "shared", "multi": total(rows[multi:2 * multi]),
            "loop": total(rows[2 * multi:])}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", default="256:48:16", help="n:m:p (C4)")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--layer", action="store_true", help="also time layer.solution_vjp against backward passes of solve_qp")
    ap.add_argument("--trace-only", action="store_true", help="the new call twice, then the loop, and nothing else")
    ap.add_argument("--out", default=None, help="write one JSON document here")
    ap.add_argument("--summarize", default=None, metavar="KERNEL_TRACE_CSV",
                    help="no GPU work: add the kernel times of a --trace-only profiler run to the document at --out")
    a = ap.parse_args()
    n, m, p = (int(x) for x in a.shape.split(":"))
    if a.summarize:
        with open(a.out) as f:
            doc = json.load(f)
        doc["kernel_trace"] = {"source": "rocprofv3 --kernel-trace of this tool with --trace-only, a run of its own",
                               "results": summarize_trace(a.summarize)}
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(json.dumps(doc["kernel_trace"]["results"]))
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("data_vjp_multi_bench: no GPU visible (there is no CPU fallback)")
    import ipmz_amd as I

    ctx = I.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(99)

    def solver(batch):
        g = I.Batch(n, m, p, batch, ctx)
        g.generate(1234)
        g.step()
        g.step()
        return g

    def legs_of(g, W, shared):
        ncot = W.shape[1]
        return {"multi": lambda: g.data_grad_tensors_multi(W, shared=shared),
                "loop": lambda: [g.data_grad_tensors(W[:, r], shared=shared) for r in range(ncot)]}

    if a.trace_only:
        g = solver(TRACE_B)
        W = torch.randn((TRACE_B, TRACE_NCOT, g.state_len), generator=gen, dtype=torch.float64, device="cuda")
        legs = legs_of(g, W, NAMES)
        legs["multi"]()
        legs["multi"]()
        legs["loop"]()
        torch.cuda.synchronize()
        g.close()
        return

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out = f()
        e1.record(stream)
        e1.synchronize()
        del out
        return e0.elapsed_time(e1)

    def race(legs):
        for f in legs.values():
            f()
        ms = {k: [] for k in legs}
        for _ in range(a.reps):
            for name, f in legs.items():
                ms[name].append(timed(f))
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        return med, {k: max(v) - min(v) for k, v in ms.items()}

    doc = {"tool": "tools/data_vjp_multi_bench.py", "device": torch.cuda.get_device_name(0),
           "method": "median of device-event times around each leg, the two legs alternated in one process after a "
                     "warm-up of both; results compared bitwise before any time is taken",
           "legs": {"multi": "Optimizer.data_grad_tensors_multi (one ipmz_batch_data_vjp_multi)",
                    "loop": "ncot times Optimizer.data_grad_tensors on W[:, r] (ipmz_batch_data_vjp)"},
           "results": []}
    for layout, shared, batch in (("shared", NAMES, 1024), ("per_qp", (), 128)):
        g = solver(batch)
        L = g.state_len
        for ncot in NCOTS:
            W = torch.randn((batch, ncot, L), generator=gen, dtype=torch.float64, device="cuda")
            legs = legs_of(g, W, shared)
            ra, rb = legs["multi"](), legs["loop"]()
            torch.cuda.synchronize()
            for k in NAMES:
                for r in range(ncot):
                    row = ra[k][r] if shared else ra[k][:, r]
                    if not torch.equal(row.contiguous().view(torch.int64), rb[r][k].contiguous().view(torch.int64)):
                        sys.exit(f"data_vjp_multi_bench: {layout} ncot {ncot}: row {r} of {k} differs from the loop's")
            del ra, rb
            med, spread = race(legs)
            rec = {"n": n, "m": m, "p": p, "batch": batch, "L": L, "layout": layout, "ncot": ncot, "reps": a.reps,
                   "ms_median": med, "ms_spread_max_minus_min": spread, "multi_over_loop": med["multi"] / med["loop"],
                   "rows_bitwise_equal": True}
            doc["results"].append(rec)
            print(json.dumps(rec), flush=True)
            del W, legs
            torch.cuda.empty_cache()
        g.close()
    if a.layer:
        import oracle
        from ipmz_amd import layer
        import numpy as np
        keys = dict(Q="Q", c="c", l_x="lx", u_x="ux", A_ineq="A", l_A_ineq="lA", u_A_ineq="uA", A_eq="C", b_eq="d")
        qs = [oracle.gen_qp(n, m, p, 1000 + i) for i in range(LAYER_B)]
        leaves = {k: torch.from_numpy(np.stack([q[v] for q in qs])).cuda().requires_grad_(True) for k, v in keys.items()}
        bt = I.Batch(n, m, p, LAYER_B, ctx)
        x = layer.solve_qp(bt, strict=False, **leaves)
        converged = int(bt.batch_scalars()[:, I.SC["converged"]].sum()) if hasattr(I, "SC") else None
        G = torch.randn((LAYER_B, LAYER_NCOT, n), generator=gen, dtype=torch.float64, device="cuda")
        inputs = list(leaves.values())
        legs = {"solution_vjp": lambda: layer.solution_vjp(bt, G)[0],
                "backward_loop": lambda: [torch.autograd.grad((G[:, r] * x).sum(), inputs, retain_graph=True)
                                          for r in range(LAYER_NCOT)]}
        ra, rb = legs["solution_vjp"](), legs["backward_loop"]()
        torch.cuda.synchronize()
        worst = max(((ra[k][:, r] - rb[r][i]).abs().max() / rb[r][i].abs().max().clamp(min=1.0)).item()
                    for i, k in enumerate(leaves) for r in range(LAYER_NCOT))
        del ra, rb  # (the two adjoint solves differ in nrhs: the distance is reported, not judged here)
        med, spread = race(legs)
        rec = {"what": "layer", "n": n, "m": m, "p": p, "batch": LAYER_B, "ncot": LAYER_NCOT, "reps": a.reps,
               "ms_median": med, "ms_spread_max_minus_min": spread,
               "solution_vjp_over_backward_loop": med["solution_vjp"] / med["backward_loop"], "legs_differ_by": worst, "converged": converged}
        doc["layer"] = rec
        print(json.dumps(rec), flush=True)
        bt.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

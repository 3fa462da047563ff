#!/usr/bin/env python3
"""The gradient with respect to the problem data (ipmz_batch_data_vjp) against what a user writes without it.

    python tools/data_vjp_bench.py [--shape 256:48:16:1024] [--reps 15] [--out profiles/data_vjp/bench.json]

One configuration (default C4: n 256, m 48, p 16, batch 1024, the default formulation, the iterate after two
steps, standard-normal cotangent rows), two block layouts -- per-QP blocks and blocks shared by the batch -- and for
each two legs alternated in one process after a warm-up of both, timed with device events:

  vjp    (a) the new call, Optimizer.data_grad_tensors: nine fresh tensors and one ipmz_batch_data_vjp
  torch  (b) torch.einsum / slicing over state_tensor(0) and W producing the same nine gradients (the state is read
         once before the timed region, which favours this leg)

Before any time is reported the two legs' results are compared (1e-10 relative to max(1, |b|inf) per block).
Medians over the repetitions and max - min as the spread.  The per-QP blocks are pure stores: the bytes model is
batch (n^2 + m n + p n + 3 n + 2 m + p) 8.  Kernel times come from a rocprofv3 --kernel-trace --stats run of this
tool with --trace-only (two calls per layout, the second one read), added to the document with --summarize.
There is no CPU fallback.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ipm-zoo_amd"))

HBM_PEAK_TBS = 8.0  # bench.py / BASELINE.md "Peaks"
KERNELS = ("k_grad_matrix<", "k_grad_vectors(", "k_grad_vectors_shared(", "k_grad_shared_part<", "k_grad_shared_sum(")
NAMES = ("Q", "c", "l_x", "u_x", "A_ineq", "l_A_ineq", "u_A_ineq", "A_eq", "b_eq")


def bytes_model(n, m, p, batch):
    return batch * (n * n + m * n + p * n + 3 * n + 2 * m + p) * 8


def torch_leg(torch, S, W, n, m, p, shared):
    """The nine gradients of the default form (SlackedSlacks, both bounds, Regularization) by hand: the Newton order
    x, lambda_A, lambda_C, s, p, lambda_g, lambda_h, lambda_y, lambda_z, g, h, y, z."""
    off, o = {}, 0
    for name, k in (("x", n), ("lambda_A", m), ("lambda_C", p), ("s", m), ("p", p), ("lambda_g", m), ("lambda_h", m),
                    ("lambda_y", n), ("lambda_z", n)):
        off[name] = slice(o, o + k)
        o += k
    x, wx = S[:, off["x"]], W[:, off["x"]]
    outer = "bi,bj->ij" if shared else "bi,bj->bij"
    g = {"Q": torch.einsum(outer, wx, x), "c": wx, "l_x": W[:, off["lambda_y"]], "u_x": -W[:, off["lambda_z"]],
         "A_ineq": torch.einsum(outer, W[:, off["lambda_A"]], x) + torch.einsum(outer, S[:, off["lambda_A"]], wx),
         "l_A_ineq": W[:, off["lambda_g"]], "u_A_ineq": -W[:, off["lambda_h"]],
         "A_eq": torch.einsum(outer, W[:, off["lambda_C"]], x) + torch.einsum(outer, S[:, off["lambda_C"]], wx),
         "b_eq": -W[:, off["lambda_C"]]}
    for k in ("c", "l_x", "u_x", "l_A_ineq", "u_A_ineq", "b_eq"):
        g[k] = g[k].sum(dim=0) if shared else g[k].clone()
    return g


def summarize_trace(path, n, m, p, batch):
    """The second call of each layout of a --trace-only run, from the profiler's kernel trace CSV."""
    import csv
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if any(k in r["Kernel_Name"] for k in KERNELS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = {k: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if k in r["Kernel_Name"]]
          for k in KERNELS}
    # per-QP calls: 3 matrix launches + 1 vector launch each; shared calls: 3 (part, sum) pairs + 1 shared-vector launch
    # (names as the trace prints them, up to the template or argument list)
    per = {"k_grad_matrix": us["k_grad_matrix<"][3:6], "k_grad_vectors": us["k_grad_vectors("][1]}
    sh = {"k_grad_shared_part": us["k_grad_shared_part<"][3:6], "k_grad_shared_sum": us["k_grad_shared_sum("][3:6],
          "k_grad_vectors_shared": us["k_grad_vectors_shared("][1]}
    per_us = sum(per["k_grad_matrix"]) + per["k_grad_vectors"]
    model = bytes_model(n, m, p, batch)
    return {"per_qp": {"kernel_us": per, "sum_us": per_us, "bytes_model": model,
                       "TBps": model / (per_us * 1e-6) / 1e12,
                       "fraction_of_hbm_peak": model / (per_us * 1e-6) / 1e12 / HBM_PEAK_TBS},
            "shared": {"kernel_us": sh, "sum_us": sum(sh["k_grad_shared_part"]) + sum(sh["k_grad_shared_sum"]) +
                       sh["k_grad_vectors_shared"],
                       "mfma_flops": 2 * batch * n * (n + 2 * m + 2 * p)}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", default="256:48:16:1024", help="n:m:p:batch (C4)")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--trace-only", action="store_true", help="two calls of the new call per layout and nothing else")
    ap.add_argument("--out", default=None, help="write one JSON document here")
    ap.add_argument("--summarize", default=None, metavar="KERNEL_TRACE_CSV",
                    help="no GPU work: add the kernel times of a --trace-only profiler run to the document at --out")
    a = ap.parse_args()
    n, m, p, batch = (int(x) for x in a.shape.split(":"))
    if a.summarize:
        with open(a.out) as f:
            doc = json.load(f)
        doc["kernel_trace"] = {"source": "rocprofv3 --kernel-trace --stats of this tool with --trace-only, a run of its "
                                         "own; the second call of each layout",
                               "results": summarize_trace(a.summarize, n, m, p, batch)}
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(json.dumps(doc["kernel_trace"]["results"]))
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("data_vjp_bench: no GPU visible (there is no CPU fallback)")
    import ipmz_amd as I

    ctx = I.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    g = I.Batch(n, m, p, batch, ctx)
    g.generate(1234)
    g.step()
    g.step()
    L = g.state_len
    gen = torch.Generator(device="cuda")
    gen.manual_seed(99)
    W = torch.randn((batch, L), generator=gen, dtype=torch.float64, device="cuda")
    if a.trace_only:
        for shared in ((), NAMES):
            g.data_grad_tensors(W, shared=shared)
            g.data_grad_tensors(W, shared=shared)
        torch.cuda.synchronize()
        g.close()
        return
    S = g.state_tensor(0)

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out = f()
        e1.record(stream)
        e1.synchronize()
        del out
        return e0.elapsed_time(e1)

    doc = {"tool": "tools/data_vjp_bench.py", "device": torch.cuda.get_device_name(0),
           "method": "median of device-event times around each leg, the two legs alternated in one process after a "
                     "warm-up of both; results compared before any time is taken",
           "legs": {"vjp": "Optimizer.data_grad_tensors (ipmz_batch_data_vjp)",
                    "torch": "torch.einsum / slicing over state_tensor(0) and W, the state read before the timed region"},
           "peaks": {"hbm_TBps": HBM_PEAK_TBS}, "results": []}
    for layout, shared in (("per_qp", ()), ("shared", NAMES)):
        legs = {"vjp": lambda: g.data_grad_tensors(W, shared=shared),
                "torch": lambda: torch_leg(torch, S, W, n, m, p, bool(shared))}
        ra, rb = legs["vjp"](), legs["torch"]()
        torch.cuda.synchronize()
        worst = max(((ra[k] - rb[k]).abs().max() / rb[k].abs().max().clamp(min=1.0)).item() for k in NAMES)
        if not worst <= 1e-10:
            sys.exit(f"data_vjp_bench: {layout}: the two legs differ by {worst:.3e} relative")
        del ra, rb
        for f in legs.values():
            f()
        ms = {k: [] for k in legs}
        for _ in range(a.reps):
            for name, f in legs.items():
                ms[name].append(timed(f))
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        rec = {"n": n, "m": m, "p": p, "batch": batch, "L": L, "layout": layout, "reps": a.reps,
               "ms_median": med, "ms_spread_max_minus_min": {k: max(v) - min(v) for k, v in ms.items()},
               "vjp_over_torch": med["vjp"] / med["torch"], "legs_differ_by": worst}
        if layout == "per_qp":
            rec["bytes_model"] = bytes_model(n, m, p, batch)
            rec["vjp_call_fraction_of_hbm_peak"] = rec["bytes_model"] / (med["vjp"] * 1e-3) / 1e12 / HBM_PEAK_TBS
        doc["results"].append(rec)
        print(json.dumps(rec), flush=True)
    g.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

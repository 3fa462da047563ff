#!/usr/bin/env python3
"""The adjoint Newton solve for a block of cotangents (ipmz_qp_newton_adjoint_multi /
ipmz_batch_newton_adjoint_multi) against the forward call it transposes.

    python tools/newton_adjoint_bench.py [--batch 256:48:16:1024] [--batch-nrhs 1,4,16,32]
                                         [--single 8192:2048:1024] [--single-nrhs 1,4,16,32] [--out FILE]

For every configuration (QP i = the generator's seed + i, the initial iterate)
and every nrhs, two legs alternated in one process after a warm-up of both and
timed with device events around the call:

  adjoint  (a) the new call: E^T g, assembly, factor, blocked solve, expansion,
           one synchronize
  forward  (b) ipmz_*_newton_solve_multi with alpha = NULL and the same nrhs:
           the same assembly, factor and solve between its own two
           element-wise kernels

Medians over the repetitions, and max - min as the spread.  Both element-wise
pairs move about 3 L 8 bytes per row (the block read twice and written once)
plus the workspace row; the kernels' own times come from a rocprofv3
--kernel-trace --stats run of this tool with --trace-only (two calls of each
leg per configuration and count, the second one read; no timing legs), added
to the document with --summarize.  Before any time is reported the two calls
are checked against each other: <g, Dir(r)> = <Adj(g), r> on the device's own
outputs.  There is no CPU fallback.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ipm-zoo_amd"))

HBM_PEAK_TBS = 8.0  # bench.py / BASELINE.md "Peaks"
PAIRS = {"adjoint": ("k_adj_reduce_multi", "k_adj_expand_multi"), "forward": ("k_rhs_multi", "k_backsub_multi")}


def run(torch, I, ctx, stream, n, m, p, batch, nrhs_list, reps, trace_only):
    g = I.Batch(n, m, p, batch, ctx) if batch > 1 else I.Optimizer(n, m, p, ctx)
    g.generate(1234)
    N, L = g.N, g.state_len
    ld = L + (L & 1)
    nmax = max(nrhs_list)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(99)
    R = torch.randn((batch, nmax, ld), generator=gen, dtype=torch.float64, device="cuda")
    G = torch.randn((batch, nmax, ld), generator=gen, dtype=torch.float64, device="cuda")
    D = torch.empty_like(R)
    W = torch.empty_like(R)

    def adjoint(nrhs):
        if batch > 1:
            return g.newton_adjoint_all(G.data_ptr(), W.data_ptr(), nrhs, ld, nmax * ld, ld, nmax * ld)
        return g.newton_adjoint(G.data_ptr(), W.data_ptr(), nrhs, ld, ld)

    def forward(nrhs):
        if batch > 1:
            return g.newton_solve_all(R.data_ptr(), D.data_ptr(), nrhs, ld, nmax * ld, ld, nmax * ld, None)
        return g.newton_solve(R.data_ptr(), D.data_ptr(), nrhs, ld, ld, None)

    def timed(f, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        info = f(*a)
        e1.record(stream)
        e1.synchronize()
        if info != 0:
            sys.exit(f"newton_adjoint_bench: factor info {info}")
        return e0.elapsed_time(e1)

    legs = {"adjoint": adjoint, "forward": forward}
    if trace_only:
        for nrhs in nrhs_list:  # twice each: the second launch of a count is the warm one
            for f in legs.values():
                f(nrhs)
                f(nrhs)
        g.close()
        return []
    # warm-up of both legs, and the two against each other before any time is reported
    adjoint(nmax)
    forward(nmax)
    gd = torch.einsum("bal,bcl->bac", G[:, :, :L], D[:, :, :L])
    wr = torch.einsum("bal,bcl->bac", W[:, :, :L], R[:, :, :L])
    bound = 1e-10 * (G[:, :, :L].abs().sum(dim=2)[:, :, None] * D[:, :, :L].abs().amax(dim=2).clamp(min=1.0)[:, None, :] +
                     R[:, :, :L].abs().sum(dim=2)[:, None, :] * W[:, :, :L].abs().amax(dim=2).clamp(min=1.0)[:, :, None])
    gap = ((gd - wr).abs() / bound).max().item()
    if not gap <= 1.0:
        sys.exit(f"newton_adjoint_bench: N={N} batch={batch}: |<g, Dir r> - <Adj g, r>| / bound = {gap:.3e}")
    for nrhs in nrhs_list:
        for f in legs.values():
            f(nrhs)
    out = []
    for nrhs in nrhs_list:
        ms = {k: [] for k in legs}
        for _ in range(reps):
            for name, f in legs.items():
                ms[name].append(timed(f, nrhs))
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        rec = {"n": n, "m": m, "p": p, "N": N, "L": L, "batch": batch, "nrhs": nrhs, "reps": reps,
               "call_ms_median": med, "call_ms_spread_max_minus_min": {k: max(v) - min(v) for k, v in ms.items()},
               "adjoint_over_forward": med["adjoint"] / med["forward"],
               "adjoint_minus_forward_ms": med["adjoint"] - med["forward"],
               "dot_identity_gap_over_bound": gap,
               "elementwise_bytes_model": 3 * L * 8 * nrhs * batch}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    g.close()
    return out


def summarize_trace(path, configs):
    """The warm (second) launch of every (configuration, nrhs, leg) of a --trace-only run, from the
    profiler's kernel trace CSV: the two element-wise kernels of each direction, their sum, the
    adjoint / forward ratio and the achieved rate against the 3 L 8 nrhs batch byte model."""
    import csv
    names = [k for pair in PAIRS.values() for k in pair]
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if any(k in r["Kernel_Name"] for k in names)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = {k: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if k in r["Kernel_Name"]]
          for k in names}
    out = []
    for i, (n, m, p, batch, L, nrhs) in enumerate(configs):
        t = {k: us[k][2 * i + 1] for k in names}  # (one launch of each per call at these counts)
        model = 3 * L * 8 * nrhs * batch
        pair = {leg: sum(t[k] for k in ks) for leg, ks in PAIRS.items()}
        out.append({"n": n, "m": m, "p": p, "batch": batch, "L": L, "nrhs": nrhs, "kernel_us": t, "pair_us": pair,
                    "adjoint_pair_over_forward_pair": pair["adjoint"] / pair["forward"],
                    "elementwise_bytes_model": model,
                    "elementwise_TBps": {leg: model / (v * 1e-6) / 1e12 for leg, v in pair.items()},
                    "fraction_of_hbm_peak": {leg: model / (v * 1e-6) / 1e12 / HBM_PEAK_TBS for leg, v in pair.items()}})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", default="256:48:16:1024", help="n:m:p:batch (C4's batch); empty: skip")
    ap.add_argument("--batch-nrhs", default="1,4,16,32")
    ap.add_argument("--single", default="8192:2048:1024", help="n:m:p (C3's size); empty: skip")
    ap.add_argument("--single-nrhs", default="1,4,16,32")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--single-reps", type=int, default=5)
    ap.add_argument("--trace-only", action="store_true",
                    help="two calls of each leg per (configuration, nrhs) and nothing else, for a profiler run")
    ap.add_argument("--out", default=None, help="write one JSON document here")
    ap.add_argument("--summarize", default=None, metavar="KERNEL_TRACE_CSV",
                    help="no GPU work: add the kernel times of a --trace-only profiler run (same --batch / --single "
                         "arguments) to the document at --out")
    a = ap.parse_args()
    if a.summarize:
        def state_len(n, m, p):  # SlackedSlacks, both bounds, Regularization
            return 5 * n + 6 * m + 2 * p
        cfg = []
        if a.batch:
            n, m, p, batch = (int(x) for x in a.batch.split(":"))
            cfg += [(n, m, p, batch, state_len(n, m, p), int(k)) for k in a.batch_nrhs.split(",")]
        if a.single:
            n, m, p = (int(x) for x in a.single.split(":"))
            cfg += [(n, m, p, 1, state_len(n, m, p), int(k)) for k in a.single_nrhs.split(",")]
        with open(a.out) as f:
            doc = json.load(f)
        doc["kernel_trace"] = {"source": "rocprofv3 --kernel-trace --stats of this tool with --trace-only, a run of its "
                                         "own; the second launch of every count and leg",
                               "results": summarize_trace(a.summarize, cfg)}
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        for r in doc["kernel_trace"]["results"]:
            print(json.dumps(r))
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("newton_adjoint_bench: no GPU visible (there is no CPU fallback)")
    import ipmz_amd as I

    ctx = I.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    doc = {"tool": "tools/newton_adjoint_bench.py", "device": torch.cuda.get_device_name(0),
           "method": "median of device-event times around each call, the two legs alternated in one process after a "
                     "warm-up of both; every call ends with one synchronize and the info read",
           "legs": {"adjoint": "the new call", "forward": "ipmz_*_newton_solve_multi, alpha = NULL, same nrhs"},
           "peaks": {"hbm_TBps": HBM_PEAK_TBS}, "results": []}

    def dump():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")

    if a.batch:
        n, m, p, batch = (int(x) for x in a.batch.split(":"))
        doc["results"] += run(torch, I, ctx, stream, n, m, p, batch, [int(x) for x in a.batch_nrhs.split(",")], a.reps,
                              a.trace_only)
        dump()
    if a.single:
        n, m, p = (int(x) for x in a.single.split(":"))
        doc["results"] += run(torch, I, ctx, stream, n, m, p, 1, [int(x) for x in a.single_nrhs.split(",")],
                              a.single_reps, a.trace_only)
        dump()


if __name__ == "__main__":
    main()

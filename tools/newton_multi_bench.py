#!/usr/bin/env python3
"""Newton directions for a block of residuals (ipmz_qp_newton_solve_multi /
ipmz_batch_newton_solve_multi): what the top layer costs and what blocking buys.

    python tools/newton_multi_bench.py [--batch 256:48:16:1024] [--batch-nrhs 1,4,16,32]
                                       [--single 8192:2048:1024] [--single-nrhs 1,8,32] [--out FILE]

For every configuration (QP i = the generator's seed + i, the initial iterate)
and every nrhs, legs alternated in one process after a warm-up of every leg
and timed with device events around the call:

  newton   (a) the new call: reduction, assembly, factor, blocked solve,
           back-substitution, step lengths, one synchronize
  kkt      (b) the matching *_kkt_solve* call with the same nrhs: (a) - (b) is
           what the three element-wise launches cost
  rows     (c) nrhs calls of one row each: what reusing one factor buys
  rpg1 / rpg2 / rpg8   (a) with 1 / 2 / 8 rows per thread in the two
           element-wise kernels instead of IPMZ_NEWTON_MULTI_RPG = 4 (debug bits)

Medians over the repetitions, and max - min as the spread.  The element-wise
kernels move about 3 L 8 bytes per row (R read twice, Dir written once); their
own times come from a rocprofv3 --kernel-trace --stats run of this tool with
--trace-only (two calls per configuration and count, the second one read;
no timing legs).  One JSON object per
(configuration, nrhs) on stdout and, with --out, one JSON document.  There is
no CPU fallback.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ipm-zoo_amd"))

HBM_PEAK_TBS = 8.0  # bench.py / BASELINE.md "Peaks"
RPG1, RPG8 = 2097152, 4194304  # kernels.h IPMZ_DEBUG_NEWTON_RPG*


def run(torch, I, ctx, stream, n, m, p, batch, nrhs_list, reps, trace_only):
    g = I.Batch(n, m, p, batch, ctx) if batch > 1 else I.Optimizer(n, m, p, ctx)
    g.generate(1234)
    N, L = g.N, g.state_len
    ld, ldb = L + (L & 1), N + (N & 1)
    nmax = max(nrhs_list)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(99)
    R = torch.randn((batch, nmax, ld), generator=gen, dtype=torch.float64, device="cuda")
    D = torch.empty_like(R)
    A = torch.empty((batch, nmax), dtype=torch.float64, device="cuda")
    K0 = torch.rand((batch, nmax, ldb), generator=gen, dtype=torch.float64, device="cuda") * 2 - 1
    K = torch.empty_like(K0)

    def newton(nrhs, bits=0):
        I.debug_inject(bits)
        try:
            if batch > 1:
                return g.newton_solve_all(R.data_ptr(), D.data_ptr(), nrhs, ld, nmax * ld, ld, nmax * ld, A.data_ptr())
            return g.newton_solve(R.data_ptr(), D.data_ptr(), nrhs, ld, ld, A.data_ptr())
        finally:
            I.debug_inject(0)

    def kkt(nrhs):
        K.copy_(K0)
        if batch > 1:
            return g.kkt_solve_all(K.data_ptr(), nrhs, ldb, nmax * ldb)
        return g.kkt_solve(K.data_ptr(), nrhs, ldb)

    def rows(nrhs):
        for r in range(nrhs):
            if batch > 1:
                g.newton_solve_all(R.data_ptr() + 8 * ld * r, D.data_ptr() + 8 * ld * r, 1, ld, nmax * ld, ld, nmax * ld,
                                   A.data_ptr() + 8 * r)
            else:
                g.newton_solve(R.data_ptr() + 8 * ld * r, D.data_ptr() + 8 * ld * r, 1, ld, ld, A.data_ptr() + 8 * r)
        return 0

    def timed(f, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        info = f(*a)
        e1.record(stream)
        e1.synchronize()
        if info != 0:
            sys.exit(f"newton_multi_bench: factor info {info}")
        return e0.elapsed_time(e1)

    if trace_only:
        for nrhs in nrhs_list:  # twice each: the second launch of a count is the warm one
            newton(nrhs)
            newton(nrhs)
        g.close()
        return []
    # warm-up of every leg, and the looped rows against the blocked call before any time is reported
    newton(nmax)
    Dref = D.clone()
    rows(nmax)
    scale = Dref[:, :, :L].abs().amax(dim=2).clamp(min=1.0)
    err = ((D[:, :, :L] - Dref[:, :, :L]).abs().amax(dim=2) / scale).max().item()
    if not err < 1e-10:
        sys.exit(f"newton_multi_bench: N={N} batch={batch}: blocked call vs looped rows {err:.3e}")
    legs = {"newton": lambda k: newton(k), "kkt": kkt, "rows": rows, "rpg1": lambda k: newton(k, RPG1),
            "rpg2": lambda k: newton(k, RPG1 | RPG8), "rpg8": lambda k: newton(k, RPG8)}
    for nrhs in nrhs_list:
        for f in legs.values():
            f(nrhs)
    out = []
    for nrhs in nrhs_list:
        ms = {k: [] for k in ["base", *legs]}
        for _ in range(reps):
            ms["base"].append(timed(newton, 0))
            for name, f in legs.items():
                ms[name].append(timed(f, nrhs))
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        rec = {"n": n, "m": m, "p": p, "N": N, "L": L, "batch": batch, "nrhs": nrhs, "reps": reps,
               "call_ms_median": med, "call_ms_spread_max_minus_min": {k: max(v) - min(v) for k, v in ms.items()},
               "elementwise_ms_newton_minus_kkt": med["newton"] - med["kkt"],
               "rows_over_newton": med["rows"] / med["newton"],
               "blocked_vs_looped_rows_max_rel_err": err,
               "elementwise_bytes_model": 3 * L * 8 * nrhs * batch}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    g.close()
    return out


def summarize_trace(path, configs):
    """The warm (second) launch of every (configuration, nrhs) of a --trace-only run, from the
    profiler's kernel trace CSV: the three kernels' times and the achieved rate of the two
    element-wise ones against their 3 L 8 nrhs batch byte model."""
    import csv
    names = ("k_rhs_multi", "k_backsub_multi", "k_ratio_multi")
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if any(k in r["Kernel_Name"] for k in names)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = {k: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if k in r["Kernel_Name"]]
          for k in names}
    out = []
    for i, (n, m, p, batch, L, nrhs) in enumerate(configs):
        t = {k: us[k][2 * i + 1] for k in names}  # (one launch of each per call at these counts)
        model = 3 * L * 8 * nrhs * batch
        ew = t["k_rhs_multi"] + t["k_backsub_multi"]
        out.append({"n": n, "m": m, "p": p, "batch": batch, "L": L, "nrhs": nrhs, "kernel_us": t,
                    "elementwise_bytes_model": model, "elementwise_TBps": model / (ew * 1e-6) / 1e12,
                    "fraction_of_hbm_peak": model / (ew * 1e-6) / 1e12 / HBM_PEAK_TBS})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", default="256:48:16:1024", help="n:m:p:batch (C4's batch); empty: skip")
    ap.add_argument("--batch-nrhs", default="1,4,16,32")
    ap.add_argument("--single", default="8192:2048:1024", help="n:m:p (C3's size); empty: skip")
    ap.add_argument("--single-nrhs", default="1,8,32")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--single-reps", type=int, default=5)
    ap.add_argument("--trace-only", action="store_true", help="two calls per (configuration, nrhs) and nothing else, for a profiler run")
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
                                         "own; the second launch of every count",
                               "results": summarize_trace(a.summarize, cfg)}
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        for r in doc["kernel_trace"]["results"]:
            print(json.dumps(r))
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("newton_multi_bench: no GPU visible (there is no CPU fallback)")
    import ipmz_amd as I

    ctx = I.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    doc = {"tool": "tools/newton_multi_bench.py", "device": torch.cuda.get_device_name(0),
           "method": "median of device-event times around each call, legs alternated in one process after a warm-up "
                     "of every leg; every call ends with one synchronize and the info read",
           "legs": {"newton": "the new call", "kkt": "the matching *_kkt_solve* call, same nrhs",
                    "rows": "nrhs calls of one row each", "base": "the new call with nrhs = 0",
                    "rpg1/rpg2/rpg8": "the new call with 1 / 2 / 8 rows per thread (default 4)"},
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

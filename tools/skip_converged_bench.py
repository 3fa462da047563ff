#!/usr/bin/env python3
"""IPMZ_STEP_SKIP_CONVERGED (Batch.solve_all(skip_converged=True)), measured against the flag-off path of the same
run -- which is the step and the solve loop as they were before the flag existed.

    python tools/skip_converged_bench.py [--shape 256:48:16] [--batches 1024,128] [--reps 9] [--out FILE]

One process, device events around the timed work, every leg warmed up, legs alternated; median and max - min.

(a) One step with a fraction f of the QPs converged, f in {0, 0.5, 0.9, 1}, flag off against flag on.  The batch is
    solved; before every timed step every QP is put at its solution and the first (1 - f) B QPs back at the initial
    iterate (set_state_tensor(solved), set_state_tensor(V0, take=mask), unchecked), so the step starts from the
    same state in both legs.
(b) A cold solve_all: plain (ipmz_batch_solve), skip with check_every 1, skip with check_every 4, and skip with
    check_every 4 on a replayed graph.  The iterate restarts with load_tensors(c=) before every timed solve.
(c) The same four after a warm start: c scaled by 1.01, the iterate set from the previous solution with
    --warm-floor (1e-2: the floor that won every row of the warm start's table in DESIGN.md).

(b) and (c) also record the iterations solve_all reports, the QPs converged and, for the skip legs, the mean and the
maximum of the per-QP step counts (step_counts()): the work the skipped launches did not do.  The final iterates of
the four legs are compared bitwise before any time is reported.  There is no CPU fallback.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ipm-zoo_amd"))
sys.path.insert(0, HERE)

FRACTIONS = (0.0, 0.5, 0.9, 1.0)
SOLVE_LEGS = (("plain", dict()),
              ("skip_check1", dict(skip_converged=True, check_every=1)),
              ("skip_check4", dict(skip_converged=True, check_every=4)),
              ("skip_check4_graph", dict(skip_converged=True, check_every=4, graph=True)))


def median(v):
    return sorted(v)[len(v) // 2]


def stats(v):
    return {"ms_median": median(v), "ms_spread_max_minus_min": max(v) - min(v)}


def timed(torch, stream, f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    out = f()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), out


def step_legs(torch, I, stream, g, batch, reps, V0, solved):
    rows = []
    for f in FRACTIONS:
        active = batch - int(round(f * batch))
        take = torch.zeros(batch, dtype=torch.int32, device="cuda")
        take[:active] = 1
        legs = {"flag_off": 0, "flag_on": I.STEP_SKIP_CONVERGED}
        ms = {k: [] for k in legs}
        unconverged = None
        for rep in range(reps + 1):  # (rep 0: the warm-up of both legs)
            for name, flags in legs.items():
                g.set_state_tensor(solved, check=False)
                g.set_state_tensor(V0, take=take, check=False)
                if unconverged is None:
                    unconverged = int((g.batch_scalars()[:, I.SC["converged"]] == 0.0).sum())
                t, _ = timed(torch, stream, lambda: g.step(flags))
                if rep:
                    ms[name].append(t)
        rec = {"fraction_converged": f, "unconverged_at_the_step": unconverged,
               **{k: stats(v) for k, v in ms.items()}}
        rows.append(rec)
        print(json.dumps(rec), flush=True)
    return rows


def solve_legs(torch, I, stream, g, reps, max_iter, prepare):
    """prepare(): puts the batch at the start of the solve; then every leg of SOLVE_LEGS, alternated."""
    ms = {k: [] for k, _ in SOLVE_LEGS}
    facts, final = {}, {}
    for rep in range(reps + 1):
        for name, kw in SOLVE_LEGS:
            prepare()
            t, (its, conv) = timed(torch, stream, lambda: g.solve_all(max_iter, **kw))
            if rep:
                ms[name].append(t)
                continue
            facts[name] = {"iterations": its, "converged": conv, "last_step_graph": int(g.last_step_graph())}
            if kw.get("skip_converged"):
                sc = g.step_counts()
                facts[name].update(step_count_mean=float(sc.mean()), step_count_max=int(sc.max()),
                                   step_count_min=int(sc.min()))
            final[name] = g.state_tensor().clone()
    for name, v in final.items():
        if not torch.equal(v.view(torch.int64), final["plain"].view(torch.int64)):
            sys.exit(f"skip_converged_bench: the final iterates of leg {name} differ from the plain solve's")
    out = {k: {**facts[k], **stats(v)} for k, v in ms.items()}
    out["final_iterates_bitwise_equal"] = True
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", default="256:48:16", help="n:m:p (C4's QPs)")
    ap.add_argument("--batches", default="1024,128", help="batch sizes (C4, and one rank's shard of 8)")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--warm-floor", type=float, default=1e-2)
    ap.add_argument("--out", default=None, help="write one JSON document here")
    a = ap.parse_args()
    n, m, p = (int(x) for x in a.shape.split(":"))
    import torch
    if not torch.cuda.is_available():
        sys.exit("skip_converged_bench: no GPU visible (there is no CPU fallback)")
    import ipmz_amd as I
    from load_bench import make_data

    ctx = I.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    doc = {"tool": "tools/skip_converged_bench.py", "device": torch.cuda.get_device_name(0),
           "method": "one process; device events around the step (a) or the whole solve_all call (b, c); every leg "
                     "warmed up once, legs alternated, median and max - min of --reps times; the flag-off / plain leg "
                     "of the same run is the reference; data of tools/load_bench.py make_data",
           "results": []}
    for batch in (int(x) for x in a.batches.split(",")):
        data = make_data(torch, n, m, p, batch)
        torch.cuda.synchronize()
        g = I.Batch(n, m, p, batch, ctx)
        if not g.can_skip_converged():
            sys.exit("skip_converged_bench: this shape and batch cannot skip converged QPs")
        g.load_tensors(**data)
        V0 = g.state_tensor().clone()
        rec = {"n": n, "m": m, "p": p, "N": g.N, "batch": batch, "reps": a.reps, "warm_floor": a.warm_floor}
        its, conv = g.solve_all(a.max_iter)
        if conv != batch:
            sys.exit(f"skip_converged_bench: {batch - conv} QPs did not converge")
        rec["first_solve_iterations"] = its
        prev = g.state_tensor().clone()
        rec["step"] = step_legs(torch, I, stream, g, batch, a.reps, V0, prev)
        rec["cold_solve"] = solve_legs(torch, I, stream, g, a.reps, a.max_iter, lambda: g.load_tensors(c=data["c"]))
        c2 = (1.01 * data["c"]).contiguous()
        torch.cuda.synchronize()

        def warm():
            g.load_tensors(c=c2)
            g.set_state_tensor(prev, floor=a.warm_floor)

        rec["warm_solve"] = solve_legs(torch, I, stream, g, a.reps, a.max_iter, warm)
        g.close()
        doc["results"].append(rec)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Centering on the central path (ipmz_batch_center): what one iteration costs beside one Newton step, and how many
iterations a converged solve needs.

    python tools/center_bench.py [--batch 256:48:16:1024] [--single 8192:2048:1024] [--kappas 1e-2,1e-4,1e-6]
                                 [--out profiles/center/bench.json]

For every configuration (QP i = the generator's seed + i) the solver is solved to convergence once and that iterate
kept on the device.  Legs, alternated in one process after a warm-up of every leg, each from that same iterate (put
back with set_state_tensor before the leg, outside the timed region) and timed with device events around the call:

  step      one ipmz_qp_step (flags 0): the step is untouched by the centering, so this is its number
  center0   center(kappa, max_iter = 0): the test, the evaluation, the host's look -- no iteration
  center1   center(kappa, max_iter = 1): the same plus ONE iteration (right-hand side, assembly, factor, solve,
            back-substitution, step length, gated update, test)

iteration = center1 - center0, per repetition.  An iteration is a step minus one solve, plus one residual pass with
its norm and one summary.  Then, per kappa, the whole call from the converged iterate: iterations per QP, QPs
centered, milliseconds.  Medians over the repetitions, max - min as the spread.  The phase timers of one step
(ipmz_qp_set_timing) are recorded for the case that an iteration costs more than 1.5 steps.  One JSON object per
configuration on stdout and, with --out, one JSON document.  There is no CPU fallback.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ipm-zoo_amd"))

TOL, CAP = 1e-10, 30


def run(torch, I, ctx, stream, n, m, p, batch, kappas, reps):
    g = I.Batch(n, m, p, batch, ctx) if batch > 1 else I.Optimizer(n, m, p, ctx)
    g.generate(1234)
    if batch > 1:
        steps, nconv = g.solve_all(100)
    else:
        steps, _ = g.solve(100)
        nconv = int(g.scalars()["converged"] == 1.0)
    if nconv != batch:
        sys.exit(f"center_bench: {batch - nconv} of {batch} QPs did not converge")
    Z = g.state_tensor(0).clone()

    def reset():
        g.set_state_tensor(Z, check=False)

    def timed(f):
        reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out = f()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), out

    k0 = kappas[0]
    legs = {"step": lambda: g.step(), "center0": lambda: g.center(k0, TOL, 0), "center1": lambda: g.center(k0, TOL, 1)}
    for f in legs.values():  # warm-up of every leg (the centering's buffers are allocated here)
        timed(f)
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, f in legs.items():
            ms[k].append(timed(f)[0])
    ms["iteration"] = [b - a for a, b in zip(ms["center0"], ms["center1"])]
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    whole = []
    for kappa in kappas:
        t, its, cnt = [], None, None
        for _ in range(reps):
            dt, (its, cnt) = timed(lambda: g.center(kappa, TOL, CAP))
            t.append(dt)
        whole.append({"kappa": kappa, "iterations_min": int(its.min()), "iterations_max": int(its.max()),
                      "iterations_mean": float(its.mean()), "centered": cnt, "call_ms_median": sorted(t)[len(t) // 2],
                      "call_ms_spread_max_minus_min": max(t) - min(t)})
    reset()
    ctx.set_stream(None)  # (the phase events are recorded on the context's own stream)
    g.set_timing(True)
    g.step()
    phases = g.phase_times()
    g.set_timing(False)
    ctx.set_stream(stream.cuda_stream)
    rec = {"n": n, "m": m, "p": p, "N": g.N, "L": g.state_len, "batch": batch, "reps": reps, "solve_steps": steps,
           "kappa_of_the_legs": k0, "call_ms_median": med,
           "call_ms_spread_max_minus_min": {k: max(v) - min(v) for k, v in ms.items()},
           "iteration_over_step": med["iteration"] / med["step"], "from_a_converged_solve": whole,
           "one_step_phase_ms": phases}
    print(json.dumps(rec), flush=True)
    g.close()
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", default="256:48:16:1024", help="n:m:p:batch (C4's batch); empty: skip")
    ap.add_argument("--single", default="8192:2048:1024", help="n:m:p (C3's size); empty: skip")
    ap.add_argument("--kappas", default="1e-2,1e-4,1e-6")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--single-reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="write one JSON document here")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("center_bench: no GPU visible (there is no CPU fallback)")
    import ipmz_amd as I

    ctx = I.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    kappas = [float(x) for x in a.kappas.split(",")]
    doc = {"tool": "tools/center_bench.py", "device": torch.cuda.get_device_name(0),
           "method": "median of device-event times around each call, legs alternated in one process after a warm-up "
                     "of every leg, every leg from the same converged iterate; max - min as the spread",
           "legs": {"step": "one ipmz_qp_step, flags 0", "center0": "ipmz_batch_center with max_iter 0",
                    "center1": "ipmz_batch_center with max_iter 1", "iteration": "center1 - center0 per repetition"},
           "tol": TOL, "max_iter": CAP, "results": []}

    def dump():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")

    if a.batch:
        n, m, p, batch = (int(x) for x in a.batch.split(":"))
        doc["results"].append(run(torch, I, ctx, stream, n, m, p, batch, kappas, a.reps))
        dump()
    if a.single:
        n, m, p = (int(x) for x in a.single.split(":"))
        doc["results"].append(run(torch, I, ctx, stream, n, m, p, 1, kappas, a.single_reps))
        dump()


if __name__ == "__main__":
    main()

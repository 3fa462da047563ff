#!/usr/bin/env python3
"""The device warm start (ipmz_batch_set_state_device: Optimizer.set_state_tensor), measured two ways.

    python tools/warm_start_bench.py [--shape 256:64:0] [--batches 1024,128] [--reps 7] [--out FILE]

(a) The call against the only way in before it, the host loop of ipmz_batch_set_state (one call per QP: a copy
    from host memory, an evaluation of the batch and a synchronize each).  The iterate is the batch's own after
    three steps, on the device for the new call and already on the host for the loop.  Medians of device-event
    times around each leg, legs alternated in one process after a warm-up of every leg; the legs' iterates,
    residuals and scalars are compared bitwise before any time is taken.

      device_unchecked  set_state_tensor(V, check=False): the scatter and the evaluation, enqueued
      device_checked    set_state_tensor(V): the check kernel and a synchronize for its verdict first
      host_loop         set_state(q, V[q]) for every q

(b) A cold re-solve against a warm one.  The batch is solved once; then c is perturbed by a relative 1e-3, 1e-2
    and 1e-1 and the batch solved again: cold (load_tensors(c=) leaves build_environment's iterate), and warm from
    the previous solution with floor in {0, 1e-6, 1e-4, 1e-2} (load_tensors(c=), set_state_tensor(prev, floor=),
    solve_all).  Per combination: the iterations solve_all reports, how many QPs converged within --max-iter, and
    the median host-clock time of the whole re-solve (load, set, solve) ending synchronized.  A warm start the
    check refuses is recorded as such.  Every row is reported, the ones where the warm start loses included.

There is no CPU fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ipm-zoo_amd"))
sys.path.insert(0, HERE)

RELS = (1e-3, 1e-2, 1e-1)
FLOORS = (0.0, 1e-6, 1e-4, 1e-2)


def median(v):
    return sorted(v)[len(v) // 2]


def call_legs(torch, I, ctx, stream, g, batch, reps):
    for _ in range(3):
        g.step()
    V = g.state_tensor().clone()
    Vh = V.cpu().numpy()
    legs = {"device_unchecked": lambda: g.set_state_tensor(V, check=False),
            "device_checked": lambda: g.set_state_tensor(V),
            "host_loop": lambda: [g.set_state(q, Vh[q]) for q in range(batch)]}
    snaps = {}
    for name, f in legs.items():  # the warm-up, and the legs agree before any time is reported
        f()
        snaps[name] = (g.state_tensor(0).clone(), g.state_tensor(3).clone(), g.batch_scalars())
    ref = snaps["host_loop"]
    for name, s in snaps.items():
        if not (torch.equal(s[0].view(torch.int64), ref[0].view(torch.int64)) and
                torch.equal(s[1].view(torch.int64), ref[1].view(torch.int64)) and
                np.array_equal(s[2].view(np.uint64), ref[2].view(np.uint64))):
            sys.exit(f"warm_start_bench: batch {batch}: leg {name} differs from the host loop")

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        f()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    ms = {k: [] for k in legs}
    for _ in range(reps):
        for name, f in legs.items():
            ms[name].append(timed(f))
    med = {k: median(v) for k, v in ms.items()}
    return {"ms_median": med, "ms_spread_max_minus_min": {k: max(v) - min(v) for k, v in ms.items()},
            "host_loop_over_device_checked": med["host_loop"] / med["device_checked"],
            "host_loop_over_device_unchecked": med["host_loop"] / med["device_unchecked"], "legs_bitwise_equal": True}


def resolve_legs(torch, I, ctx, g, data, batch, reps, max_iter):
    g.load_tensors(**data)
    its0, conv0 = g.solve_all(max_iter)
    ctx.sync()
    prev = g.state_tensor().clone()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4321)
    u = torch.rand(data["c"].shape, generator=gen, dtype=torch.float64, device="cuda") * 2 - 1
    rows = []
    for rel in RELS:
        c2 = (data["c"] * (1.0 + rel * u)).contiguous()
        torch.cuda.synchronize()
        for floor in (None,) + FLOORS:  # None: the cold re-solve
            rec = {"c_relative_perturbation": rel, "start": "cold" if floor is None else "warm", "floor": floor}
            wall = []
            for _ in range(reps):
                ctx.sync()
                t0 = time.perf_counter()
                g.load_tensors(c=c2)
                try:
                    if floor is not None:
                        g.set_state_tensor(prev, floor=floor)
                except I.IpmzError as e:
                    rec["refused"] = str(e)
                    break
                its, conv = g.solve_all(max_iter)
                ctx.sync()
                wall.append((time.perf_counter() - t0) * 1e3)
                rec.update(iterations=its, converged=conv)
            if wall:
                rec.update(wall_ms_median=median(wall), wall_ms_spread_max_minus_min=max(wall) - min(wall))
            rows.append(rec)
            print(json.dumps(rec), flush=True)
    return {"first_solve": {"iterations": its0, "converged": conv0}, "max_iter": max_iter, "rows": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", default="256:64:0", help="n:m:p (C4's QPs)")
    ap.add_argument("--batches", default="1024,128", help="batch sizes (C4, and one rank's shard of 8)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--out", default=None, help="write one JSON document here")
    a = ap.parse_args()
    n, m, p = (int(x) for x in a.shape.split(":"))
    import torch
    if not torch.cuda.is_available():
        sys.exit("warm_start_bench: no GPU visible (there is no CPU fallback)")
    import ipmz_amd as I
    from load_bench import make_data

    ctx = I.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    doc = {"tool": "tools/warm_start_bench.py", "device": torch.cuda.get_device_name(0),
           "method": {"call": "median of device-event times around each leg, legs alternated in one process after a "
                              "warm-up of every leg; the legs compared bitwise before any time is taken",
                      "resolve": "iterations and converged count of solve_all, median host-clock time of load_tensors(c=) "
                                 "[+ set_state_tensor(prev, floor=)] + solve_all ending synchronized; c perturbed by "
                                 "c * (1 + rel * u), u uniform in (-1, 1); data of tools/load_bench.py make_data"},
           "results": []}
    for batch in (int(x) for x in a.batches.split(",")):
        data = make_data(torch, n, m, p, batch)
        torch.cuda.synchronize()
        g = I.Batch(n, m, p, batch, ctx)
        g.load_tensors(**data)
        rec = {"n": n, "m": m, "p": p, "batch": batch, "state_len": g.state_len, "reps": a.reps}
        rec["call"] = call_legs(torch, I, ctx, stream, g, batch, a.reps)
        print(json.dumps({k: rec[k] for k in ("batch", "call")}), flush=True)
        rec["resolve"] = resolve_legs(torch, I, ctx, g, data, batch, max(3, a.reps // 2), a.max_iter)
        g.close()
        doc["results"].append(rec)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()

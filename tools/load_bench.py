#!/usr/bin/env python3
"""Getting a batch of QPs into a solver and its states out again: the host
path (ipmz_batch_load_host per QP, ipmz_batch_get_state per QP) against the
device-resident one (ipmz_batch_load_device, ipmz_batch_copy_state).

    python tools/load_bench.py [--shape 256:64:0] [--batches 1024,128] [--reps 7] [--out FILE]

The data are float64 CUDA tensors (what a caller of the device path has).  For
every batch size, legs alternated in one process after a warm-up of every leg,
each timed with the host clock around a call that ends synchronized:

  host_load      tensors -> .cpu() -> load_one x B -> initialize(): the only way in before
  device_load    load_tensors of the same tensors, Q / A / C per QP
  device_shared  load_tensors with Q / A / C given once for the batch (QP stride 0)
  device_vectors load_tensors(c=, b_eq= or l_x=): the parametric re-load
  initialize     initialize() alone: what every load ends with
  host_state     state(q) x B
  device_state   state_tensor(0)

Medians over the repetitions and max - min as the spread.  The copy kernels' own
times come from a rocprofv3 --kernel-trace run of this tool with --trace-only
(two device loads per batch size, the second one read), added to the document
with --summarize; their achieved bytes/s is the bytes the copy must move
(every supplied element read once and written once) over that time.  There is
no CPU fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ipm-zoo_amd"))

HBM_PEAK_TBS = 8.0  # bench.py / BASELINE.md "Peaks"


def pack_bytes(n, m, p, batch, shared):
    """Read + written by the copy kernels: the matrices are read once when shared, once per QP otherwise."""
    mat, vec = (n + m + p) * n, 3 * n + 2 * m + p
    return 8 * (batch * (mat + vec) + (mat if shared else batch * mat) + batch * vec)


def make_data(torch, n, m, p, batch):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)

    def rnd(*shape):
        return torch.rand(shape, generator=gen, dtype=torch.float64, device="cuda") * 2 - 1

    Q = rnd(batch, n, n) / n
    Q = 0.5 * (Q + Q.transpose(1, 2)) + torch.eye(n, dtype=torch.float64, device="cuda")
    d = dict(Q=Q.contiguous(), c=rnd(batch, n), l_x=-torch.ones((batch, n), dtype=torch.float64, device="cuda"),
             u_x=torch.ones((batch, n), dtype=torch.float64, device="cuda"))
    if m:
        d.update(A_ineq=rnd(batch, m, n) / n ** 0.5, l_A_ineq=-torch.ones((batch, m), dtype=torch.float64, device="cuda"),
                 u_A_ineq=torch.ones((batch, m), dtype=torch.float64, device="cuda"))
    if p:
        d.update(A_eq=rnd(batch, p, n) / n ** 0.5, b_eq=0.1 * rnd(batch, p))
    return d


def run(torch, I, ctx, n, m, p, batch, reps, trace_only):
    data = make_data(torch, n, m, p, batch)
    shared = dict(data)
    for k in ("Q", "A_ineq", "A_eq"):
        if k in shared:
            shared[k] = data[k][0].contiguous()
    vectors = {"c": data["c"], ("b_eq" if p else "l_x"): data["b_eq" if p else "l_x"]}
    torch.cuda.synchronize()
    g = I.Batch(n, m, p, batch, ctx)

    def host_load():
        h = {k: v.cpu().numpy() for k, v in data.items()}
        for q in range(batch):
            g.load_one(q, I.Data(**{k: v[q] for k, v in h.items()}))
        g.initialize()

    def host_state():
        return [g.state(q) for q in range(batch)]

    legs = {"host_load": host_load, "device_load": lambda: g.load_tensors(**data),
            "device_shared": lambda: g.load_tensors(**shared), "device_vectors": lambda: g.load_tensors(**vectors),
            "initialize": g.initialize, "host_state": host_state, "device_state": lambda: g.state_tensor(0)}
    if trace_only:
        for _ in range(2):  # the second launch of each kernel is the warm one
            g.load_tensors(**data)
            g.load_tensors(**shared)
            g.state_tensor(0)
        g.close()
        return None
    # warm-up of every leg; the two ways in and the two ways out agree before any time is reported
    host_load()
    ref = torch.from_numpy(np.stack(host_state())).cuda()
    g.load_tensors(**data)
    if not torch.equal(g.state_tensor(0), ref) or not torch.equal(g.state_tensor(3)[0].cpu(),
                                                                   torch.from_numpy(g.state(0, 3))):
        sys.exit(f"load_bench: batch {batch}: the device load / read-back differs from the host one")
    for f in legs.values():
        f()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for name, f in legs.items():
            ctx.sync()
            t0 = time.perf_counter()
            f()
            ctx.sync()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    rec = {"n": n, "m": m, "p": p, "batch": batch, "state_len": g.state_len, "reps": reps, "call_ms_median": med,
           "call_ms_spread_max_minus_min": {k: max(v) - min(v) for k, v in ms.items()},
           "host_over_device_load": med["host_load"] / med["device_load"],
           "host_over_device_shared_load": med["host_load"] / med["device_shared"],
           "host_over_device_state": med["host_state"] / med["device_state"],
           "device_load_minus_initialize_ms": med["device_load"] - med["initialize"],
           "pack_bytes_model": {"per_qp": pack_bytes(n, m, p, batch, False), "shared": pack_bytes(n, m, p, batch, True)},
           "host_copy_calls_model": batch * (4 + (3 if m else 0) + (2 if p else 0)), "host_synchronizes_model": batch + 1}
    print(json.dumps(rec), flush=True)
    g.close()
    return rec


def summarize_trace(path, configs):
    """The warm launches of a --trace-only run from the profiler's kernel trace CSV: per batch size the copy
    kernels of the per-QP load and of the shared load, the bound check and the read-back."""
    import csv
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if "k_io_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))

    def us(r):
        return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3

    out, at = [], 0
    for n, m, p, batch in configs:
        # per iteration: 2 loads x (validate, one matrix kernel per present matrix, vectors) + 1 gather
        nm = 1 + (1 if m else 0) + (1 if p else 0)
        per_load = 1 + nm + 1
        it = 2 * per_load + 1
        warm = rows[at + it:at + 2 * it]
        at += 2 * it
        names = [r["Kernel_Name"] for r in warm]
        assert len(warm) == it and "validate" in names[0] and "gather" in names[-1], names
        rec = {"n": n, "m": m, "p": p, "batch": batch, "validate_us": us(warm[0]), "gather_state_us": us(warm[-1])}
        for label, lo, shared in (("per_qp", 0, False), ("shared", per_load, True)):
            t = sum(us(r) for r in warm[lo + 1:lo + per_load])
            b = pack_bytes(n, m, p, batch, shared)
            rec[label] = {"pack_kernels_us": t, "pack_bytes_model": b, "pack_TBps": b / (t * 1e-6) / 1e12,
                          "fraction_of_hbm_peak": b / (t * 1e-6) / 1e12 / HBM_PEAK_TBS}
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", default="256:64:0", help="n:m:p (C4's QPs)")
    ap.add_argument("--batches", default="1024,128", help="batch sizes (C4, and one rank's shard of 8)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--trace-only", action="store_true", help="two device loads and read-backs per batch size and "
                                                              "nothing else, for a profiler run")
    ap.add_argument("--out", default=None, help="write one JSON document here")
    ap.add_argument("--summarize", default=None, metavar="KERNEL_TRACE_CSV",
                    help="no GPU work: add the kernel times of a --trace-only profiler run (same --shape / --batches) "
                         "to the document at --out")
    a = ap.parse_args()
    n, m, p = (int(x) for x in a.shape.split(":"))
    batches = [int(x) for x in a.batches.split(",")]
    if a.summarize:
        with open(a.out) as f:
            doc = json.load(f)
        doc["kernel_trace"] = {"source": "rocprofv3 --kernel-trace of this tool with --trace-only, a run of its own; "
                                         "the second launch of every kernel",
                               "results": summarize_trace(a.summarize, [(n, m, p, b) for b in batches])}
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        for r in doc["kernel_trace"]["results"]:
            print(json.dumps(r))
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("load_bench: no GPU visible (there is no CPU fallback)")
    import ipmz_amd as I

    ctx = I.Context(0)
    doc = {"tool": "tools/load_bench.py", "device": torch.cuda.get_device_name(0),
           "method": "median of host-clock times around each leg, the context synchronized before and after, legs "
                     "alternated in one process after a warm-up of every leg",
           "legs": {"host_load": "tensors -> .cpu() -> load_one x B -> initialize()",
                    "device_load": "load_tensors, Q / A / C per QP", "device_shared": "load_tensors, Q / A / C shared",
                    "device_vectors": "load_tensors of two vector blocks (parametric re-load)",
                    "initialize": "initialize() alone", "host_state": "state(q) x B", "device_state": "state_tensor(0)"},
           "peaks": {"hbm_TBps": HBM_PEAK_TBS}, "results": []}
    for batch in batches:
        rec = run(torch, I, ctx, n, m, p, batch, a.reps, a.trace_only)
        if rec:
            doc["results"].append(rec)
        if a.out and not a.trace_only:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()

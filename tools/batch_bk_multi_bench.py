#!/usr/bin/env python3
"""Batched multi-right-hand-side Bunch-Kaufman KKT solve
(ipmz_batch_kkt_solve_bk, EqualityHandling::None batches): its three paths
against each other, after tools/batch_multi_bench.py.

    python tools/batch_bk_multi_bench.py [--shapes 256:64:0:1024,...] [--nrhs 1,2,3,4,...] [--out FILE]

For every shape n:m:p:batch (QP i = the generator's seed + i, the initial
iterate) and every nrhs, legs alternated in one process after a warm-up of the
whole shape and timed with device events around the call:

  base         the call with nrhs = 0: assembly + batched factor + the info read
               (no prepare: nothing is solved)
  default      the public call (looped below the crossover, else fused where a
               QP's slab fits the LDS, else 256-column panels)
  fused        debug bit 65536: the one-launch solve from 2 rows on (only where
               it is eligible; otherwise this leg is the 256-column panel chain
               and is reported as such)
  w128 / w256 / w512   debug bits 65536 + 262144 / both / 131072: the panel
               chain with the QP on a grid dimension, at that width
  loop         nrhs < the crossover: the default leg (one launch of the step's
               single-vector batched solve per row, the parent's kernels).  Every
               row is one more launch of the same kernel in stream order, so for
               larger nrhs the loop is row_ms * nrhs with row_ms from the
               directly measured counts; such figures are marked extrapolated.

The solve alone is time(nrhs) - time(0) of the call: assembly, factor and the
final synchronization are common to every leg.  For the blocked legs it holds
the once-per-call prepare (transpose, scan, L', untranspose, inverse diagonal
blocks), which the loop does not need; prepare_ms reports it on its own,
measured with ipmz_bk_prepare_solve_batch on caller-owned storage of the same
order and batch (identity pivots, as the generated QPs factor), and
solve_without_prepare_ms = solve_ms - prepare_ms.  Every blocked leg is checked
against the looped rows (|x - x_ref|_inf < 1e-10 max(1, |x_ref|_inf)) before
any time is reported.  One JSON object per (shape, nrhs) on stdout and, with
--out, one JSON document.  There is no CPU fallback.

Algorithmic bytes per QP: the strict lower triangle of L once per sweep (2
sweeps) -- the loop reads it 2 nrhs times -- plus B once in and once out
(fused), or the panel chain's B traffic of tools/solve_multi_bench.py.  Flops:
2 N^2 nrhs per QP.  Peaks: bench.py's.  Shapes: C4's (n 256, m 64) with
EqualityHandling::None at batch 1024 and 128, N = 832 x 128, N = 1040 x 64.
"""
import argparse
import json
import math
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ipm-zoo_amd"))

FP64_MFMA_PEAK_TFLOPS = 78.6  # bench.py / BASELINE.md "Peaks"
HBM_PEAK_TBS = 8.0
TOL = 1e-10
MULTI_BLOCKED, MULTI_W512, MULTI_W128 = 65536, 131072, 262144  # kernels.h IPMZ_DEBUG_MULTI_*
DEFAULT_SHAPES = "256:64:0:1024,256:64:0:128,640:160:32:128,800:200:40:64"
DEFAULT_NRHS = "1,2,3,4,6,8,12,16,32,64,128"


def crossover():
    with open(os.path.join(HERE, "..", "ipm-zoo_amd", "csrc", "capi.cpp")) as f:
        return int(re.search(r"static constexpr int BK_BATCH_MULTI_CROSSOVER = (\d+);", f.read()).group(1))


def prepare_ms(torch, ctx, stream, N, batch, reps):
    """Median time of ipmz_bk_prepare_solve_batch alone (unit lower factors, identity pivots)."""
    ld = N + (N & 1)
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    F = torch.rand((batch, N, ld), generator=g, dtype=torch.float64, device="cuda") * 0.01
    F += torch.eye(N, ld, dtype=torch.float64, device="cuda")
    piv = torch.arange(N, dtype=torch.int32, device="cuda").repeat(batch, 1).contiguous()
    wsb = ctx.bk_batch_solve_workspace_bytes(N, batch)
    ws = torch.zeros(wsb // 8 + 1, dtype=torch.float64, device="cuda")
    ms = []
    for i in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        ctx.bk_prepare_solve_batch(N, batch, F.data_ptr(), ld, N * ld, piv.data_ptr(), N, ws.data_ptr(), wsb)
        e1.record(stream)
        e1.synchronize()
        if i >= 2:
            ms.append(e0.elapsed_time(e1))
    return sorted(ms)[len(ms) // 2], max(ms) - min(ms)


def panel_bytes(N, nrhs, w):
    b = 0
    for p0 in range(0, N, w):
        p1 = min(p0 + w, N)
        b += 16 * nrhs * (2 * (p1 - p0) + (N - p1) + p0)
    return b + 16 * nrhs * N


def run_shape(torch, I, ctx, stream, n, m, p, batch, nrhs_list, min_seconds, cross):
    bt = I.Batch(n, m, p, batch, ctx, equality_handling=I.EQ_NONE)
    bt.generate(1234)
    N = bt.N
    ldb = N + (N & 1)
    g = torch.Generator(device="cuda")
    g.manual_seed(99)
    nmax = max(nrhs_list)
    B0 = torch.rand((batch, nmax, ldb), generator=g, dtype=torch.float64, device="cuda") * 2 - 1
    B = torch.empty_like(B0)
    sB = nmax * ldb

    def once(bits, nrhs):
        B.copy_(B0)
        I.debug_inject(bits)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        try:
            e0.record(stream)
            info, _ = bt.kkt_solve_all_bk(B.data_ptr(), nrhs, ldb, sB)
            e1.record(stream)
            e1.synchronize()
        finally:
            I.debug_inject(0)
        if info != 0:
            sys.exit(f"batch_bk_multi_bench: factor info {info}")
        return e0.elapsed_time(e1)

    legs = {"default": 0, "fused": MULTI_BLOCKED, "w128": MULTI_BLOCKED | MULTI_W128,
            "w256": MULTI_BLOCKED | MULTI_W128 | MULTI_W512, "w512": MULTI_BLOCKED | MULTI_W512}
    # warm-up of the whole shape, and correctness: every blocked leg against the looped rows
    once(0, 0)
    B.copy_(B0)
    for r in range(nmax):  # one looped row per call, in place (nrhs = 1 is always the loop)
        bt.kkt_solve_all_bk(B.data_ptr() + 8 * ldb * r, 1, ldb, sB)
    X_ref = B.clone()
    scale = X_ref[:, :, :N].abs().amax(dim=2).clamp(min=1.0)
    errs = {}
    for name, bits in legs.items():
        once(bits, nmax)
        err = ((B[:, :, :N] - X_ref[:, :, :N]).abs().amax(dim=2) / scale).max().item()
        errs[name] = err
        if not (err < TOL) or not torch.isfinite(B[:, :, :N]).all().item():
            sys.exit(f"batch_bk_multi_bench: N={N} batch={batch} leg {name}: error {err:.3e} against the looped rows")
    for nrhs in nrhs_list:
        for bits in legs.values():
            once(bits, nrhs)

    est = max(once(0, 0), 1e-3)
    reps = int(max(7, min(math.ceil(1e3 * min_seconds / est), 60)))
    prep, prep_spread = prepare_ms(torch, ctx, stream, N, batch, reps)
    out = []
    for nrhs in nrhs_list:
        ms = {k: [] for k in ["base", *legs]}
        for _ in range(reps):
            ms["base"].append(once(0, 0))
            for name, bits in legs.items():
                ms[name].append(once(bits, nrhs))
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        solve = {k: med[k] - med["base"] for k in legs}
        spread = {k: (max(v) - min(v)) for k, v in ms.items()}
        l_once = 8 * N * (N - 1) // 2 * 2 * batch
        flops = 2.0 * N * N * nrhs * batch
        bytes_ = {"loop": l_once * nrhs + 16 * nrhs * N * batch, "fused": l_once + 16 * nrhs * N * batch,
                  "w128": l_once + panel_bytes(N, nrhs, 128) * batch, "w256": l_once + panel_bytes(N, nrhs, 256) * batch,
                  "w512": l_once + panel_bytes(N, nrhs, 512) * batch}
        rec = {"n": n, "m": m, "p": p, "N": N, "batch": batch, "nrhs": nrhs, "reps": reps,
               "call_ms_median": med, "call_ms_spread_max_minus_min": spread,
               "solve_ms": solve, "default_is_loop": nrhs < cross, "prepare_ms": prep,
               "prepare_ms_spread_max_minus_min": prep_spread,
               "solve_without_prepare_ms": {k: solve[k] - prep for k in legs if not (k == "default" and nrhs < cross)},
               "max_rel_err_vs_loop_at_nrhs_max": errs, "flops": flops, "algorithmic_bytes": bytes_,
               "TBps": {k: bytes_[k] / (solve[k] * 1e-3) / 1e12 for k in ("fused", "w128", "w256", "w512")
                        if solve[k] > 0},
               "TFLOPs": {k: flops / (solve[k] * 1e-3) / 1e12 for k in legs if solve[k] > 0}}
        if nrhs < cross:
            rec["loop_solve_ms"] = solve["default"]
            rec["loop_TBps"] = bytes_["loop"] / (solve["default"] * 1e-3) / 1e12 if solve["default"] > 0 else None
        out.append(rec)
    # the loop's cost per row from the directly measured counts, and the extrapolated loop elsewhere
    direct = [r for r in out if r["nrhs"] < cross]
    row_ms = sum(r["loop_solve_ms"] for r in direct) / max(sum(r["nrhs"] for r in direct), 1) if direct else None
    loop_spread = max((r["call_ms_spread_max_minus_min"]["default"] for r in direct), default=None)
    for r in out:
        r["loop_row_ms"] = row_ms
        r["loop_spread_ms"] = loop_spread
        if row_ms is not None and "loop_solve_ms" not in r:
            r["loop_solve_ms"] = row_ms * r["nrhs"]
            r["loop_extrapolated"] = True
        if r.get("loop_solve_ms"):
            r["ratio_loop_over"] = {k: r["loop_solve_ms"] / r["solve_ms"][k] for k in ("fused", "w128", "w256", "w512")
                                    if r["solve_ms"][k] > 0}
        print(json.dumps(r), flush=True)
    bt.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="n:m:p:batch,...")
    ap.add_argument("--nrhs", default=DEFAULT_NRHS)
    ap.add_argument("--min-seconds", type=float, default=0.05, help="repetitions per leg: this long of base calls (7..60)")
    ap.add_argument("--out", default=None, help="write one JSON document here")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("batch_bk_multi_bench: no GPU visible (there is no CPU fallback)")
    import ipmz_amd as I

    ctx = I.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    cross = crossover()
    nrhs_list = [int(x) for x in a.nrhs.split(",")]
    doc = {"tool": "tools/batch_bk_multi_bench.py", "device": torch.cuda.get_device_name(0),
           "lds_per_workgroup_bytes": torch.cuda.get_device_properties(0).shared_memory_per_block
           if hasattr(torch.cuda.get_device_properties(0), "shared_memory_per_block") else None,
           "method": "solve_ms = median call time(nrhs) - median call time(0); assembly, factor and the final "
                     "synchronization are common to every leg; legs alternated inside one process after a warm-up "
                     "of every leg of the shape; device events around the call",
           "loop": "directly measured for nrhs < BK_BATCH_MULTI_CROSSOVER (the default leg); otherwise loop_row_ms * nrhs, "
                   "marked loop_extrapolated (every row is one more launch of the same kernel in stream order)",
           "fused_leg": "the one-launch solve where a QP's slab fits the LDS (N <= 832 at nbi 64); for larger N this "
                        "leg is the 256-column panel chain",
           "prepare": "solve_ms of a blocked leg holds the once-per-call prepare; prepare_ms is "
                      "ipmz_bk_prepare_solve_batch alone on caller-owned storage of the same order and batch",
           "BK_BATCH_MULTI_CROSSOVER_at_run": cross,
           "peaks": {"hbm_TBps": HBM_PEAK_TBS, "fp64_mfma_TFLOPs": FP64_MFMA_PEAK_TFLOPS}, "results": []}
    for spec in a.shapes.split(","):
        n, m, p, batch = (int(x) for x in spec.split(":"))
        doc["results"] += run_shape(torch, I, ctx, stream, n, m, p, batch, nrhs_list, a.min_seconds, cross)
        if a.out:  # (after every shape: a later failure keeps what was measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()

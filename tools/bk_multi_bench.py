#!/usr/bin/env python3
"""Multi-right-hand-side Bunch-Kaufman solve against the looped single-vector solves.

    python tools/bk_multi_bench.py [--sizes 2560,11264] [--nrhs 2,8,16,64,256] [--no-loop] [--out FILE]

For every order N (one seeded KKT matrix with a zero trailing block generated
on the device, one ipmz_bk_factor, one ipmz_bk_prepare_solve) and every nrhs,
legs alternated in one process and timed with device events after a warm-up:

  loop           nrhs ipmz_bk_solve calls on the rows of B: what a user had
                 before the multi solve (every call rebuilds the transpose, L'
                 and the solve's operators, synchronizes and frees them)
  prepared_loop  nrhs ipmz_bk_solve_multi calls of one row each on the prepared
                 workspace: the looped path of the multi solve, the yardstick
                 of the crossover
  multi          one ipmz_bk_solve_multi (the public call: blocked from the
                 crossover on, looped below it)
  blocked        the same call with debug bit 65536 (the blocked kernels from
                 nrhs = 2 on): where the crossover comes from

Every leg starts from the same B (restored outside the timed span); every
leg's rows are checked against the loop's
(|x - x_ref|_inf < 1e-10 max(1, |x_ref|_inf)) before any time is reported.
One JSON object per (N, nrhs) on stdout (and appended to --out).  Each order
runs in a child process under its own time limit; there is no CPU fallback.
--no-loop leaves the slow first leg out (crossover scans): the reference rows
are then the prepared loop's.
"""
import argparse
import json
import math
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ipm-zoo_amd"))

TOL = 1e-10
MULTI_BLOCKED = 65536  # kernels.h IPMZ_DEBUG_MULTI_BLOCKED
CHILD_TIMEOUT_S = 420


def _kkt_device(torch, N, seed):
    """[[H, B^T], [B, 0]] (lower triangle): H symmetric with a weak diagonal, so
    the factor interchanges and takes 2x2 pivots."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    n = (3 * N) // 4
    K = torch.zeros((N, N), dtype=torch.float64, device="cuda")
    H = torch.rand((n, n), generator=g, dtype=torch.float64, device="cuda") * 2 - 1
    H = H + H.T
    H.diagonal().mul_(0.01)
    K[:n, :n] = torch.tril(H)
    del H
    K[n:, :n] = torch.rand((N - n, n), generator=g, dtype=torch.float64, device="cuda") * 2 - 1
    return K


def child(N, nrhs_list, min_seconds, with_loop, out):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bk_multi_bench: no GPU visible (there is no CPU fallback)")
    import ipmz_amd as I

    ctx = I.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    F = _kkt_device(torch, N, 4321 + N)
    piv = torch.zeros(N, dtype=torch.int32, device="cuda")
    info = ctx.bk_factor(N, F.data_ptr(), N, piv.data_ptr())
    if info != 0:
        sys.exit(f"bk_multi_bench: factor info {info}")
    p = piv.cpu().numpy()
    pairs = int((p < 0).sum()) // 2
    swaps = int(((p >= 0) & (p != np.arange(N))).sum())
    wsb = ctx.bk_solve_workspace_bytes(N)
    ws = torch.zeros(wsb // 8 + 1, dtype=torch.float64, device="cuda")
    fp, pp, wp = F.data_ptr(), piv.data_ptr(), ws.data_ptr()
    ctx.bk_prepare_solve(N, fp, N, pp, wp, wsb)
    ctx.sync()

    def leg_loop(B, nrhs):
        for r in range(nrhs):
            ctx.bk_solve(N, fp, N, pp, B.data_ptr() + 8 * N * r)

    def leg_prepared_loop(B, nrhs):
        for r in range(nrhs):
            ctx.bk_solve_multi(N, fp, N, pp, wp, B.data_ptr() + 8 * N * r, N, 1)

    def leg_multi(mask):
        def run(B, nrhs):
            I.debug_inject(mask)
            try:
                ctx.bk_solve_multi(N, fp, N, pp, wp, B.data_ptr(), N, nrhs)
            finally:
                I.debug_inject(0)
        return run

    legs = [("loop", leg_loop)] if with_loop else []
    legs += [("prepared_loop", leg_prepared_loop), ("multi", leg_multi(0)), ("blocked", leg_multi(MULTI_BLOCKED))]
    g = torch.Generator(device="cuda")
    g.manual_seed(99)
    for nrhs in nrhs_list:
        B0 = torch.rand((nrhs, N), generator=g, dtype=torch.float64, device="cuda") * 2 - 1
        B = torch.empty_like(B0)

        def once(fn):
            B.copy_(B0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn(B, nrhs)
            e1.record(stream)
            e1.synchronize()
            ctx.sync()  # the solve's sticky error word
            return e0.elapsed_time(e1)

        # correctness first (also the warm-up)
        once(legs[0][1])
        X_ref = B.clone()
        scale = X_ref.abs().amax(dim=1).clamp(min=1.0)
        errs = {}
        for name, fn in legs[1:]:
            once(fn)
            err = ((B - X_ref).abs().amax(dim=1) / scale).max().item()
            errs[name] = err
            if not (err < TOL) or not torch.isfinite(B).all().item():
                sys.exit(f"bk_multi_bench: N={N} nrhs={nrhs} leg {name}: error {err:.3e} against the looped solve")
        est = {name: once(fn) for name, fn in legs}
        # the fastest leg runs min_seconds in total, unless the slowest one would then take more than ~4 s
        reps = math.ceil(1e3 * min_seconds / max(min(est.values()), 1e-3))
        reps = int(max(5, min(reps, 4e3 / max(est.values()))))
        ms = {name: [] for name, _ in legs}
        for _ in range(reps):
            for name, fn in legs:
                ms[name].append(once(fn))
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        pl = sorted(ms["prepared_loop"])
        spread_ms = pl[-1] - pl[0]
        # max - min is at the mercy of one slow repetition out of hundreds: the 5th .. 95th percentile span beside it
        p05, p95 = pl[int(0.05 * (len(pl) - 1))], pl[int(math.ceil(0.95 * (len(pl) - 1)))]
        rec = {
            "N": N, "nrhs": nrhs, "reps": reps, "panel": I.SOLVE_MULTI_PANEL, "pairs_2x2": pairs, "interchanges": swaps,
            "prepared_loop_ms": med["prepared_loop"], "prepared_loop_ms_min": min(pl), "prepared_loop_ms_max": max(pl),
            "prepared_loop_spread": spread_ms / med["prepared_loop"],
            "prepared_loop_ms_p05": p05, "prepared_loop_ms_p95": p95,
            "blocked_beats_prepared_loop_beyond_p05_p95": med["prepared_loop"] - med["blocked"] > p95 - p05,
            "multi_ms": med["multi"], "multi_ms_min": min(ms["multi"]), "multi_ms_max": max(ms["multi"]),
            "blocked_ms": med["blocked"], "blocked_ms_min": min(ms["blocked"]), "blocked_ms_max": max(ms["blocked"]),
            "ratio_prepared_loop_over_multi": med["prepared_loop"] / med["multi"],
            "ratio_prepared_loop_over_blocked": med["prepared_loop"] / med["blocked"],
            "blocked_beats_prepared_loop_beyond_spread": med["prepared_loop"] - med["blocked"] > spread_ms,
            "multi_not_slower_than_prepared_loop_within_spread": med["multi"] - med["prepared_loop"] <= spread_ms,
            "max_rel_err_vs_reference_rows": errs,
        }
        if with_loop:
            rec.update({"loop_ms": med["loop"], "loop_ms_min": min(ms["loop"]), "loop_ms_max": max(ms["loop"]),
                        "ratio_loop_over_multi": med["loop"] / med["multi"],
                        "ratio_loop_over_blocked": med["loop"] / med["blocked"]})
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="2560,11264")
    ap.add_argument("--nrhs", default="2,8,16,64,256")
    ap.add_argument("--min-seconds", type=float, default=0.3, help="each leg repeats until it ran this long in total")
    ap.add_argument("--no-loop", action="store_true", help="leave the ipmz_bk_solve loop out (crossover scans)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    nrhs_list = [int(x) for x in a.nrhs.split(",")]
    if a.child is not None:
        child(a.child, nrhs_list, a.min_seconds, not a.no_loop, a.out)
        return
    for N in [int(x) for x in a.sizes.split(",")]:
        # a fresh process per order, under its own time limit; nothing more
        # is started after one fails
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(N), "--nrhs", a.nrhs, "--min-seconds",
               str(a.min_seconds)] + (["--no-loop"] if a.no_loop else []) + (["--out", a.out] if a.out else [])
        try:
            r = subprocess.run(cmd, timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            sys.exit(f"bk_multi_bench: N={N} exceeded {CHILD_TIMEOUT_S} s")
        if r.returncode != 0:
            sys.exit(f"bk_multi_bench: N={N} failed with exit status {r.returncode}")


if __name__ == "__main__":
    main()

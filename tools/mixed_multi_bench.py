#!/usr/bin/env python3
"""Mixed-precision multi-right-hand-side solve against the looped ipmz_mixed_solve.

    python tools/mixed_multi_bench.py [--sizes 2560,16384] [--nrhs 2,8,16,64,256] [--out FILE]

For every order N (one seeded quasi-definite K generated on the device as
tools/solve_multi_bench.py does, one ipmz_mixed_factor) and every nrhs, legs
alternated in one process after a warm-up, tol = 1e-12, max_refine = 20:

  loop      nrhs ipmz_mixed_solve calls on the rows of B (stat = NULL, so
            nothing waits between the vectors) -- the only way to get this
            result without the multi solve, so it is the yardstick
  multi     one ipmz_mixed_solve_multi (the public call: blocked from the
            crossover on, looped below it)
  blocked   the same call with debug bit 65536 (the blocked path from
            nrhs = 2 on): where the crossover comes from
  blocked_w512, blocked_w128  ... with 512- / 128-column panels in the fp32
            solve (debug bits 131072 / 262144): the panel width A/B

The multi call blocks the host (it reads a stop word after every pass), so
every leg is timed as host wall time from the first call to the end of a
stream synchronize.  Every leg starts from the same B (restored outside the
timed span); the multi and blocked results are checked against the loop's rows
(|x - x_ref|_inf < 1e-10 max(1, |x_ref|_inf)) and every row's reported ratio
against tol before any time is reported.  One JSON object per (N, nrhs) on
stdout (and appended to --out).  Each order runs in a child process under its
own time limit; there is no CPU fallback.

--trace (with --child N): only the factor, one warm-up and five blocked calls
per nrhs, for a kernel trace of the blocked path:
    rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- \
        python tools/mixed_multi_bench.py --child 16384 --nrhs 64 --trace
"""
import argparse
import ctypes
import json
import math
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ipm-zoo_amd"))
sys.path.insert(0, HERE)

TOL_X = 1e-10
IR_TOL, IR_MAX = 1e-12, 20
MULTI_BLOCKED, MULTI_W512, MULTI_W128 = 65536, 131072, 262144  # kernels.h IPMZ_DEBUG_MULTI_*
CHILD_TIMEOUT_S = 540


def child(N, nrhs_list, min_seconds, out, trace=False):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("mixed_multi_bench: no GPU visible (there is no CPU fallback)")
    import ipmz_amd as I
    from solve_multi_bench import _qd_device

    ctx = I.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    K = _qd_device(torch, N, 1234 + N)
    wsb = ctx.mixed_workspace_bytes(N)
    ws = torch.zeros(wsb // 8 + 1, dtype=torch.float64, device="cuda")
    info = ctx.mixed_factor(N, K.data_ptr(), N, ws.data_ptr(), wsb)
    if info != 0:
        sys.exit(f"mixed_multi_bench: factor info {info}")
    kp, wp = K.data_ptr(), ws.data_ptr()
    VP = ctypes.c_void_p
    stats = {}

    def leg_loop(B, nrhs, mws, mwsb):
        for r in range(nrhs):
            rc = I.lib.ipmz_mixed_solve(ctx.h, N, VP(kp), N, VP(wp), VP(B.data_ptr() + 8 * N * r), IR_TOL, IR_MAX, None)
            if rc:
                sys.exit(f"mixed_multi_bench: ipmz_mixed_solve returned {rc}")

    def leg_multi(name, mask):
        def run(B, nrhs, mws, mwsb):
            I.debug_inject(mask)
            try:
                stats[name] = ctx.mixed_solve_multi(N, kp, N, wp, B.data_ptr(), N, nrhs, mws.data_ptr(), mwsb, IR_TOL,
                                                    IR_MAX)
            finally:
                I.debug_inject(0)
        return run

    legs = [("loop", leg_loop), ("multi", leg_multi("multi", 0)), ("blocked", leg_multi("blocked", MULTI_BLOCKED)),
            ("blocked_w512", leg_multi("blocked_w512", MULTI_BLOCKED | MULTI_W512)),
            ("blocked_w128", leg_multi("blocked_w128", MULTI_BLOCKED | MULTI_W128))]
    g = torch.Generator(device="cuda")
    g.manual_seed(99)
    for nrhs in nrhs_list:
        B0 = torch.rand((nrhs, N), generator=g, dtype=torch.float64, device="cuda") * 2 - 1
        B = torch.empty_like(B0)
        mwsb = ctx.mixed_multi_workspace_bytes(N, nrhs)
        mws = torch.zeros(mwsb, dtype=torch.uint8, device="cuda")

        def once(fn):
            B.copy_(B0)
            stream.synchronize()
            t0 = time.perf_counter()
            fn(B, nrhs, mws, mwsb)
            stream.synchronize()
            return 1e3 * (time.perf_counter() - t0)

        if trace:
            print(json.dumps({"N": N, "nrhs": nrhs, "blocked_ms": [once(legs[2][1]) for _ in range(6)][1:]}), flush=True)
            continue
        # correctness first (also the warm-up)
        once(leg_loop)
        X_ref = B.clone()
        scale = X_ref.abs().amax(dim=1).clamp(min=1.0)
        errs, corr = {}, {}
        for name, fn in legs[1:]:
            once(fn)
            err = ((B - X_ref).abs().amax(dim=1) / scale).max().item()
            errs[name] = err
            st = stats[name]
            corr[name] = int(st[:, 1].max())
            if not (err < TOL_X) or not torch.isfinite(B).all().item() or not np.all(st[:, 0] <= IR_TOL):
                sys.exit(f"mixed_multi_bench: N={N} nrhs={nrhs} leg {name}: error {err:.3e} against the looped solve, "
                         f"worst ratio {st[:, 0].max():.3e}")
        est = {name: once(fn) for name, fn in legs}
        # the fastest leg runs min_seconds in total, unless the slowest one would then take more than ~5 s
        reps = math.ceil(1e3 * min_seconds / max(min(est.values()), 1e-3))
        reps = int(max(5, min(reps, 5e3 / max(est.values()))))
        ms = {name: [] for name, _ in legs}
        for _ in range(reps):
            for name, fn in legs:
                ms[name].append(once(fn))
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        rec = {
            "N": N, "nrhs": nrhs, "reps": reps, "tol": IR_TOL, "max_refine": IR_MAX, "timing": "host wall, ms",
            "loop_ms": med["loop"], "loop_ms_min": min(ms["loop"]), "loop_ms_max": max(ms["loop"]),
            "loop_spread": (max(ms["loop"]) - min(ms["loop"])) / med["loop"],
            "multi_ms": med["multi"], "multi_ms_min": min(ms["multi"]), "multi_ms_max": max(ms["multi"]),
            "blocked_ms": med["blocked"], "blocked_ms_min": min(ms["blocked"]), "blocked_ms_max": max(ms["blocked"]),
            "blocked_w512_ms": med["blocked_w512"], "blocked_w128_ms": med["blocked_w128"],
            "ratio_loop_over_multi": med["loop"] / med["multi"],
            "ratio_loop_over_blocked": med["loop"] / med["blocked"],
            "multi_not_slower_than_loop_within_spread": med["multi"] <= max(ms["loop"]),
            "max_rel_err_vs_loop": errs, "max_corrections": corr,
        }
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="2560,16384")
    ap.add_argument("--nrhs", default="2,8,16,64,256")
    ap.add_argument("--min-seconds", type=float, default=0.3, help="each leg repeats until it ran this long in total")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--trace", action="store_true", help="with --child N: blocked calls only (see above)")
    a = ap.parse_args()
    nrhs_list = [int(x) for x in a.nrhs.split(",")]
    if a.child is not None:
        child(a.child, nrhs_list, a.min_seconds, a.out, a.trace)
        return
    for N in [int(x) for x in a.sizes.split(",")]:
        # a fresh process per order, under its own time limit; nothing more
        # is started after one fails
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(N), "--nrhs", a.nrhs, "--min-seconds",
               str(a.min_seconds)] + (["--out", a.out] if a.out else [])
        try:
            r = subprocess.run(cmd, timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            sys.exit(f"mixed_multi_bench: N={N} exceeded {CHILD_TIMEOUT_S} s")
        if r.returncode != 0:
            sys.exit(f"mixed_multi_bench: N={N} failed with exit status {r.returncode}")


if __name__ == "__main__":
    main()

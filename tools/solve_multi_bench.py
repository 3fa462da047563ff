#!/usr/bin/env python3
"""Multi-right-hand-side LDL^T solve against the looped single-vector solve.

    python tools/solve_multi_bench.py [--sizes 2560,11264] [--nrhs 2,8,64,256] [--out FILE]

For every order N (one seeded quasi-definite K generated on the device, one
ipmz_ldlt_factor) and every nrhs, legs alternated in one process and timed
with device events after a warm-up:

  loop      nrhs ipmz_ldlt_solve calls on the rows of B -- the only way to get
            this result without the multi solve, so it is the yardstick
  multi     one ipmz_ldlt_solve_multi (the public call: blocked from the
            crossover on, looped below it)
  blocked   the same call with debug bit 65536 (the blocked kernels from
            nrhs = 2 on): where the crossover comes from
  blocked_w512, blocked_w128  ... with 512- / 128-column panels (debug bits
            131072 / 262144): the panel width A/B

Every leg starts from the same B (restored outside the timed span); the multi
and blocked results are checked against the loop's rows
(|x - x_ref|_inf < 1e-10 max(1, |x_ref|_inf)) before any time is reported.
One JSON object per (N, nrhs) on stdout (and appended to --out).  Each order
runs in a child process under its own time limit; there is no CPU fallback.

Algorithmic bytes: the strict lower triangle of L once per sweep (2 sweeps)
plus the blocked algorithm's B traffic (each panel solve reads and writes its
nrhs x w slab, each update reads and writes the rest of B once, the diagonal
scaling reads and writes B once).  Flops: 2 N^2 nrhs.  Peaks: bench.py's.
"""
import argparse
import json
import math
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ipm-zoo_amd"))

FP64_MFMA_PEAK_TFLOPS = 78.6  # bench.py / BASELINE.md "Peaks"
HBM_PEAK_TBS = 8.0
TOL = 1e-10
MULTI_BLOCKED, MULTI_W512, MULTI_W128 = 65536, 131072, 262144  # kernels.h IPMZ_DEBUG_MULTI_*
CHILD_TIMEOUT_S = 420


def _qd_device(torch, N, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    K = torch.rand((N, N), generator=g, dtype=torch.float64, device="cuda") * 2 - 1
    n1 = (3 * N + 3) // 4
    K[:n1, :n1] /= n1
    K[n1:, :n1] /= math.sqrt(n1)
    K[n1:, n1:] = 0
    K = torch.tril(K)  # only the lower triangle is read
    d = torch.rand(N, generator=g, dtype=torch.float64, device="cuda") + 0.5
    d[n1:] *= -1
    d[:n1] += 1
    K.diagonal().copy_(d)
    return K


def _bytes_model(N, nrhs, w):
    l_bytes = 2 * 8 * N * (N - 1) // 2
    b_bytes = 0
    for p0 in range(0, N, w):
        p1 = min(p0 + w, N)
        rest = (N - p1) + p0  # forward update columns + backward update columns of this panel
        b_bytes += 16 * nrhs * (2 * (p1 - p0) + rest)  # two panel solves (read + write) and two updates
    b_bytes += 16 * nrhs * N  # the diagonal scaling
    return l_bytes, b_bytes


def child(N, nrhs_list, min_seconds, out):
    import torch
    if not torch.cuda.is_available():
        sys.exit("solve_multi_bench: no GPU visible (there is no CPU fallback)")
    import ipmz_amd as I

    ctx = I.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    K = _qd_device(torch, N, 1234 + N)
    D = torch.zeros(N, dtype=torch.float64, device="cuda")
    wsb = ctx.workspace_bytes(N)
    ws = torch.zeros(wsb // 8 + 1, dtype=torch.float64, device="cuda")
    info = ctx.ldlt_factor(N, K.data_ptr(), N, D.data_ptr(), ws.data_ptr(), wsb)
    if info != 0:
        sys.exit(f"solve_multi_bench: factor info {info}")
    kp, dp, wp = K.data_ptr(), D.data_ptr(), ws.data_ptr()
    W = I.SOLVE_MULTI_PANEL

    def leg_loop(B, nrhs):
        for r in range(nrhs):
            ctx.ldlt_solve(N, kp, N, dp, wp, B.data_ptr() + 8 * N * r)

    def leg_multi(mask):
        def run(B, nrhs):
            I.debug_inject(mask)
            try:
                ctx.ldlt_solve_multi(N, kp, N, dp, wp, B.data_ptr(), N, nrhs)
            finally:
                I.debug_inject(0)
        return run

    legs = [("loop", leg_loop), ("multi", leg_multi(0)), ("blocked", leg_multi(MULTI_BLOCKED)),
            ("blocked_w512", leg_multi(MULTI_BLOCKED | MULTI_W512)),
            ("blocked_w128", leg_multi(MULTI_BLOCKED | MULTI_W128))]
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
            ctx.sync()  # the solve's sticky error words
            return e0.elapsed_time(e1)

        # correctness first (also the warm-up)
        once(leg_loop)
        X_ref = B.clone()
        scale = X_ref.abs().amax(dim=1).clamp(min=1.0)
        errs = {}
        for name, fn in legs[1:]:
            once(fn)
            err = ((B - X_ref).abs().amax(dim=1) / scale).max().item()
            errs[name] = err
            if not (err < TOL) or not torch.isfinite(B).all().item():
                sys.exit(f"solve_multi_bench: N={N} nrhs={nrhs} leg {name}: error {err:.3e} against the looped solve")
        est = {name: once(fn) for name, fn in legs}
        # the fastest leg runs min_seconds in total, unless the slowest one would then take more than ~6 s
        reps = math.ceil(1e3 * min_seconds / max(min(est.values()), 1e-3))
        reps = int(max(5, min(reps, 6e3 / max(est.values()))))
        ms = {name: [] for name, _ in legs}
        for _ in range(reps):
            for name, fn in legs:
                ms[name].append(once(fn))
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        l_bytes, b_bytes = _bytes_model(N, nrhs, W)
        flops = 2.0 * N * N * nrhs
        t_hbm = (l_bytes + b_bytes) / (HBM_PEAK_TBS * 1e12)
        t_mfma = flops / (FP64_MFMA_PEAK_TFLOPS * 1e12)
        t = med["blocked"] * 1e-3
        rec = {
            "N": N, "nrhs": nrhs, "reps": reps, "panel": W,
            "loop_ms": med["loop"], "loop_ms_min": min(ms["loop"]), "loop_ms_max": max(ms["loop"]),
            "loop_spread": (max(ms["loop"]) - min(ms["loop"])) / med["loop"],
            "multi_ms": med["multi"], "blocked_ms": med["blocked"], "blocked_w512_ms": med["blocked_w512"],
            "blocked_w128_ms": med["blocked_w128"],
            "ratio_loop_over_multi": med["loop"] / med["multi"],
            "ratio_loop_over_blocked": med["loop"] / med["blocked"],
            "multi_not_slower_than_loop_within_spread": med["multi"] <= max(ms["loop"]),
            "max_rel_err_vs_loop": errs,
            "blocked_bytes": l_bytes + b_bytes, "blocked_bytes_L": l_bytes, "blocked_bytes_B": b_bytes,
            "blocked_TBps": (l_bytes + b_bytes) / t / 1e12, "blocked_TFLOPs": flops / t / 1e12,
            "bound": "hbm" if t_hbm >= t_mfma else "fp64_mfma",
            "blocked_share_of_bound": max(t_hbm, t_mfma) / t,
            "peaks": {"hbm_TBps": HBM_PEAK_TBS, "fp64_mfma_TFLOPs": FP64_MFMA_PEAK_TFLOPS},
        }
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="2560,11264")
    ap.add_argument("--nrhs", default="2,8,64,256")
    ap.add_argument("--min-seconds", type=float, default=0.3, help="each leg repeats until it ran this long in total")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    nrhs_list = [int(x) for x in a.nrhs.split(",")]
    if a.child is not None:
        child(a.child, nrhs_list, a.min_seconds, a.out)
        return
    for N in [int(x) for x in a.sizes.split(",")]:
        # a fresh process per order, under its own time limit; nothing more
        # is started after one fails
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(N), "--nrhs", a.nrhs, "--min-seconds",
               str(a.min_seconds)] + (["--out", a.out] if a.out else [])
        try:
            r = subprocess.run(cmd, timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            sys.exit(f"solve_multi_bench: N={N} exceeded {CHILD_TIMEOUT_S} s")
        if r.returncode != 0:
            sys.exit(f"solve_multi_bench: N={N} failed with exit status {r.returncode}")


if __name__ == "__main__":
    main()

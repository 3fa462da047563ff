#!/usr/bin/env python3
"""Forward-mode sensitivities of the residuals (ipmz_batch_data_jvp) against what a user writes without it.

    python tools/data_jvp_bench.py [--shape 256:48:16:1024] [--reps 15] [--out profiles/data_jvp/bench.json]

One configuration (default C4: n 256, m 48, p 16, batch 1024, the default formulation, the iterate after two
steps, standard-normal tangents of all nine blocks), two layouts -- per-QP tangents with ntan = 4 (about 2.7 GB of
tangents) and tangents shared by the batch with ntan = 16 -- and for each two legs alternated in one process after a
warm-up of both, timed with device events:

  jvp    (a) the new call, Optimizer.data_jvp_tensors: one fresh R and one ipmz_batch_data_jvp
  torch  (b) torch.einsum / slicing over state_tensor(0) and the tangents producing the same R (the state is read
         once before the timed region, which favours this leg)

Before any time is reported the two legs' results are compared (1e-10 relative to max(1, |b|inf)).  Medians over the
repetitions and max - min as the spread.  The per-QP layout is bandwidth-bound: the bytes model is batch ntan (n^2 +
m n + p n + 3 n + 2 m + p) 8, reported as a fraction of the HBM peak.  There is no CPU fallback.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ipm-zoo_amd"))

HBM_PEAK_TBS = 8.0  # bench.py / BASELINE.md "Peaks"
LAYOUTS = (("per_qp", 4), ("shared", 16))
DIMS = {"Q": ("n", "n"), "A_ineq": ("m", "n"), "A_eq": ("p", "n"), "c": ("n",), "l_x": ("n",), "u_x": ("n",),
        "l_A_ineq": ("m",), "u_A_ineq": ("m",), "b_eq": ("p",)}


def bytes_model(n, m, p, batch, ntan):
    return batch * ntan * (n * n + m * n + p * n + 3 * n + 2 * m + p) * 8


def torch_leg(torch, S, D, n, m, p, shared, ld):
    """R of the default form (SlackedSlacks, both bounds, Regularization) by hand: the Newton order x, lambda_A,
    lambda_C, s, p, lambda_g, lambda_h, lambda_y, lambda_z, g, h, y, z."""
    off, o = {}, 0
    for name, k in (("x", n), ("lambda_A", m), ("lambda_C", p), ("s", m), ("p", p), ("lambda_g", m), ("lambda_h", m),
                    ("lambda_y", n), ("lambda_z", n)):
        off[name] = slice(o, o + k)
        o += k
    x, la, lc = S[:, off["x"]], S[:, off["lambda_A"]], S[:, off["lambda_C"]]
    mv, mtv = ("tij,bj->bti", "tij,bi->btj") if shared else ("btij,bj->bti", "btij,bi->btj")
    B = S.shape[0]
    T = D["c"].shape[0 if shared else 1]
    R = torch.zeros((B, T, ld), dtype=torch.float64, device=S.device)
    R[:, :, off["x"]] = D["c"] + torch.einsum(mv, D["Q"], x) + torch.einsum(mtv, D["A_ineq"], la) + \
        torch.einsum(mtv, D["A_eq"], lc)
    R[:, :, off["lambda_A"]] = torch.einsum(mv, D["A_ineq"], x)
    R[:, :, off["lambda_C"]] = torch.einsum(mv, D["A_eq"], x) - D["b_eq"]
    R[:, :, off["lambda_y"]] = D["l_x"]
    R[:, :, off["lambda_z"]] = -D["u_x"]
    R[:, :, off["lambda_g"]] = D["l_A_ineq"]
    R[:, :, off["lambda_h"]] = -D["u_A_ineq"]
    return R


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", default="256:48:16:1024", help="n:m:p:batch (C4)")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None, help="write one JSON document here")
    a = ap.parse_args()
    n, m, p, batch = (int(x) for x in a.shape.split(":"))
    import torch
    if not torch.cuda.is_available():
        sys.exit("data_jvp_bench: no GPU visible (there is no CPU fallback)")
    import ipmz_amd as I

    ctx = I.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    g = I.Batch(n, m, p, batch, ctx)
    g.generate(1234)
    g.step()
    g.step()
    L = g.state_len
    ld = L + (L & 1)
    S = g.state_tensor(0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(99)
    dims = dict(n=n, m=m, p=p)

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out = f()
        e1.record(stream)
        e1.synchronize()
        del out
        return e0.elapsed_time(e1)

    doc = {"tool": "tools/data_jvp_bench.py", "device": torch.cuda.get_device_name(0),
           "method": "median of device-event times around each leg, the two legs alternated in one process after a "
                     "warm-up of both; results compared before any time is taken",
           "legs": {"jvp": "Optimizer.data_jvp_tensors (ipmz_batch_data_jvp)",
                    "torch": "torch.einsum / slicing over state_tensor(0) and the tangents, the state read before the "
                             "timed region"},
           "peaks": {"hbm_TBps": HBM_PEAK_TBS}, "results": []}
    for layout, ntan in LAYOUTS:
        shared = layout == "shared"
        lead = (ntan,) if shared else (batch, ntan)
        D = {k: torch.randn(lead + tuple(dims[s] for s in d), generator=gen, dtype=torch.float64, device="cuda")
             for k, d in DIMS.items()}
        legs = {"jvp": lambda: g.data_jvp_tensors(D), "torch": lambda: torch_leg(torch, S, D, n, m, p, shared, ld)}
        ra, rb = legs["jvp"](), legs["torch"]()
        torch.cuda.synchronize()
        worst = ((ra[:, :, :L] - rb[:, :, :L]).abs().amax(dim=2) / rb[:, :, :L].abs().amax(dim=2).clamp(min=1.0)).max().item()
        if not worst <= 1e-10:
            sys.exit(f"data_jvp_bench: {layout}: the two legs differ by {worst:.3e} relative")
        del ra, rb
        for f in legs.values():
            f()
        ms = {k: [] for k in legs}
        for _ in range(a.reps):
            for name, f in legs.items():
                ms[name].append(timed(f))
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        rec = {"n": n, "m": m, "p": p, "batch": batch, "L": L, "layout": layout, "ntan": ntan, "reps": a.reps,
               "tangent_bytes": sum(t.numel() for t in D.values()) * 8,
               "ms_median": med, "ms_spread_max_minus_min": {k: max(v) - min(v) for k, v in ms.items()},
               "jvp_over_torch": med["jvp"] / med["torch"], "legs_differ_by": worst}
        if not shared:
            rec["bytes_model"] = bytes_model(n, m, p, batch, ntan)
            rec["jvp_call_fraction_of_hbm_peak"] = rec["bytes_model"] / (med["jvp"] * 1e-3) / 1e12 / HBM_PEAK_TBS
        doc["results"].append(rec)
        print(json.dumps(rec), flush=True)
        del D, legs
        torch.cuda.empty_cache()
    g.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""A sha256 per output array of the three calls that take a QP's data blocks in device memory -- load_tensors
(ipmz_batch_load_device), data_grad_tensors (ipmz_batch_data_vjp), data_jvp_tensors (ipmz_batch_data_jvp) -- at
fixed seeds, as one JSON document: two builds computed the same bits exactly when their documents are equal
(profiles/data_blocks/bitwise.json is the document of the build that introduced this tool and of its parent).

    python tools/data_blocks_dump.py [--tree DIR] [--out FILE]

--tree: the checkout whose ipm-zoo_amd package and library are loaded (default: this one); the case tables are
always this checkout's tests/*_cases.py.
"""
import argparse
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=REPO)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path[:0] = [os.path.join(tree, "ipm-zoo_amd"), os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")]
    import numpy as np
    import torch
    import ipmz_amd as I
    import oracle
    import batch_form_cases as fc
    import data_jvp_cases as jc
    import data_vjp_cases as dc

    assert os.path.abspath(I.__file__).startswith(tree), I.__file__
    ctx = I.Context(0)
    doc = {}

    def put(key, a):
        if isinstance(a, torch.Tensor):
            torch.cuda.synchronize()
            a = a.cpu().numpy()
        assert key not in doc, key
        doc[key] = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()

    def dev(a):
        return torch.from_numpy(np.array(a, dtype=np.float64)).cuda()

    def solver(c, B, kw, steps=1, seed=1000):
        s = I.Optimizer(*c, ctx, **kw) if B == 1 else I.Batch(*c, B, ctx, **kw)
        s.generate(seed)
        for _ in range(steps):
            s.step()
        return s

    # -- load: per-QP blocks, shared blocks, per-QP blocks at an odd element offset (no 16-byte accesses) --------
    c, B = (131, 5, 3), 5
    qps = [oracle.gen_qp(*c, 2000 + b) for b in range(B)]
    for form in ("box", "eqss"):
        for layout in ("per_qp", "shared", "odd_offset"):
            s = I.Batch(*c, B, ctx, **fc.FORMS[form].kw)
            blocks = {}
            for name, k in dc.KEYS.items():
                a = np.asarray(qps[0][k]) if layout == "shared" else np.stack([np.asarray(q[k]) for q in qps])
                if layout == "odd_offset":
                    flat = torch.zeros(a.size + 1, dtype=torch.float64, device="cuda")
                    flat[1:] = dev(a).reshape(-1)
                    blocks[name] = flat[1:].view(a.shape)
                else:
                    blocks[name] = dev(a)
            s.load_tensors(**blocks)
            for w in range(4):
                put(f"load/{form}/{layout}/state{w}", s.state_tensor(w))
            put(f"load/{form}/{layout}/kkt0", s.kkt_of(0))

    # -- gradients -----------------------------------------------------------------------------------------------
    def grads(tag, c, B, kw):
        s = solver(c, B, kw)
        W = dev(dc.cotangents(s.state_len, B))
        for layout, shared in (("per_qp", ()), ("shared", tuple(dc.present(*c)))):
            if layout == "shared" and B == 1:
                continue
            for name, t in s.data_grad_tensors(W, shared=shared).items():
                put(f"vjp/{tag}/{layout}/{name}", t)

    for case in dc.BATCH_CASES + [dc.LOOP_SHAPE + (257,)]:
        grads("box/" + "x".join(map(str, case)), case[:3], case[3], {})
    for form in ("sl", "naive"):  # ("box" above is SlackedSlacks)
        grads(form + "/S1x3", fc.S1, 3, fc.FORMS[form].kw)

    # -- tangents ------------------------------------------------------------------------------------------------
    def tangents(tag, c, B, ntan, kw):
        s = solver(c, B, kw)
        L = s.state_len
        for layout in ("per_qp", "shared"):
            if layout == "shared" and B == 1:
                continue
            D = jc.tangents(*c, ntan, B if layout == "per_qp" else None)
            put(f"jvp/{tag}/{layout}", s.data_jvp_tensors({k: dev(a) for k, a in D.items()})[:, :, :L])

    for c in jc.SHAPES:
        for B in jc.BATCHES:
            for ntan in (1, 3):
                tangents("box/" + "x".join(map(str, c + (B, ntan))), c, B, ntan, {})
    for name, c, B, ntan, _ in jc.LOOPS:
        if name != "rows_gy":
            tangents("box/" + name, c, B, ntan, {})
    for form in ("box", "sl", "naive"):
        tangents(form + "/S1x3x3", fc.S1, 3, 3, fc.FORMS[form].kw)

    text = json.dumps({"arrays": len(doc), "sha256": doc}, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(f"{len(doc)} arrays, sha256 of the document: {hashlib.sha256(text.encode()).hexdigest()}")


if __name__ == "__main__":
    main()

"""Column groups with whole short rows: which T (and G) pays?

    python scripts/whole_rows_ab.py [--shape reddit] [--groups 2,3,4]
                                    [--whole 0,8,16,32,64,96] [--rounds 8] [--step]

For every (G, T): S split into G column groups with rows of at most T
nonzeros kept whole in group 0 (DeviceCSR.column_groups(G, T)); one hop at the
shape's width in the engine's padded buffers is then G launches, group 0 plain
and groups 1.. with SPMM_ACCUMULATE, whose light items stop at the plan's
count of rows with nonzeros.  "G/T0-all" is the pure split with accumulate
launches over every row (no count), i.e. the schedule before the whole-row
rule; --all-rows adds the same form for other T.  Interleaved rounds; every point checked bit-identical to the first.
--step also times the K-hop propagate() of the shape (unpadded X_0, as
bench.py runs it) with the two knobs forced.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sgc_amd import graphs  # noqa: E402
from sgc_amd.propagate import (SPMM_ACCUMULATE, SPMM_X_PADDED, SPMM_Y_PADDED,  # noqa: E402
                               DeviceCSR, propagate, spmm)

prop_mod = importlib.import_module("sgc_amd.propagate")


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def report(tag, shape, F, names, ms, outs):
    first = names[0]
    for k in names:
        print(json.dumps({"what": tag, "shape": shape, "F": F, "point": k,
                          "bit_identical": bool(torch.equal(outs[k], outs[first])),
                          "median_ms": round(float(np.median(ms[k])), 4),
                          "min_ms": round(float(np.min(ms[k])), 4),
                          "max_ms": round(float(np.max(ms[k])), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="reddit")
    ap.add_argument("--groups", default="2,3,4")
    ap.add_argument("--whole", default="0,8,16,32,64,96")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--all-rows", default="",
                    help="T values also run with accumulate launches over every row")
    ap.add_argument("--step", action="store_true", help="also the K-hop propagate()")
    a = ap.parse_args()
    Gs = [int(g) for g in a.groups.split(",")]
    Ts = [int(t) for t in a.whole.split(",")]
    spec = graphs.SHAPES[a.shape]
    F, K = spec["features"], spec["hops"]
    # synthetic_graph(shape, seed=0) in its two stages, reporting each
    u, v = graphs.rmat_pairs(spec["n"], spec["edges"], seed=0)
    print(json.dumps({"what": "pairs drawn", "edges": int(u.shape[0])}), flush=True)
    S = graphs.aug_norm_csr_from_pairs(spec["n"], u, v)
    del u, v
    print(json.dumps({"what": "graph", "n": S.n, "nnz": S.nnz}), flush=True)
    n = S.n
    csr = DeviceCSR.from_host_arrays(S.row_ptr, S.col_idx, S.val, device="cuda")
    ld = (F + 31) // 32 * 32
    X = torch.zeros((n, ld), device="cuda")
    X[:, :F] = torch.randn((n, F), generator=torch.Generator().manual_seed(1)).cuda()
    Y = torch.empty((n, ld), device="cuda")

    points = {}
    for G in Gs:
        for T in sorted({0} | {int(t) for t in a.all_rows.split(",") if t}):
            # the same split with accumulate launches over every row (no count)
            parts = [DeviceCSR(n, n, c.row_ptr, c.col_idx, c.val, c.status)
                     for c in csr.column_groups(G, T)]
            for c in parts:
                c.plan(0, n, None, None, F)
                for key, pl in list(c._plans.items()):
                    if isinstance(pl, prop_mod.Plan):
                        c._plans[key] = pl._replace(n_nonempty=-1)
            points[f"G{G}/T{T}-all"] = parts
        for T in Ts:
            points[f"G{G}/T{T}"] = csr.column_groups(G, T)
    for name, parts in points.items():
        rows = [int(c.plan(0, n, None, None, F).accumulate_light_items or 0) for c in parts[1:]]
        print(json.dumps({"what": "accumulate light items", "point": name, "items": rows}),
              flush=True)

    def hop(parts):
        for g, c in enumerate(parts):
            spmm(c, X[:, :F], 0, n, out=Y[:, :F],
                 flags=SPMM_X_PADDED | SPMM_Y_PADDED | (SPMM_ACCUMULATE if g else 0))
    names = list(points)
    outs, ms = {}, {k: [] for k in names}
    for k in names:
        hop(points[k])
        torch.cuda.synchronize()
        outs[k] = Y[:, :F].clone()
    for _ in range(a.rounds):
        for k in names:
            ms[k].append(timed(lambda: hop(points[k])))
    report("one hop", a.shape, F, names, ms, outs)
    del outs

    if a.step:
        X0 = X[:, :F].contiguous()
        out = torch.empty((n, F), device="cuda")
        names = [(G, T) for G in Gs for T in Ts]
        outs, ms = {}, {k: [] for k in names}

        def step(G, T):
            prop_mod.COLUMN_GROUPS, prop_mod.GROUP_WHOLE_ROWS = G, T
            propagate(csr, X0, K, out=out)
        for k in names:
            step(*k)
            torch.cuda.synchronize()
            outs[k] = out.clone()
        for _ in range(a.rounds):
            for k in names:
                ms[k].append(timed(lambda: step(*k)))
        report(f"K={K} step", a.shape, F, names, ms, outs)


if __name__ == "__main__":
    main()

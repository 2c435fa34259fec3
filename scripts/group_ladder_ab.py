"""Column groups by row length (the "length ladder"): heavy rows cut at all G
column cuts, medium rows at Gc coarse cuts, short rows whole.  Which (G, Gc, H,
T) pays?

    python scripts/group_ladder_ab.py --bound [--shape reddit] [--bound-groups 2,3,4,6,8]
    python scripts/group_ladder_ab.py --points 2:2:0:32,8:2:512:32,... [--widths 602,304]
                                      [--step] [--rounds 8] [--loops 10]

--bound (no ladder involved): the pure split column_groups(G, 0), every launch
an accumulate launch whose light items are cut to zero (n_nonempty = the plan's
heavy count, as the cost bound of scripts/short_wide_ab.py), so one hop runs
only its heavy and hub items.  The difference from G = 2 is the most a finer
cut of the heavy rows can save per hop, before the extra launches' cost.
--points G:Gc:H:T[,...]: one hop at each width in the engine's padded buffers
(group 0 plain, groups 1.. accumulate, as propagate() launches them), and with
--step the K-hop propagate() of the shape with the knobs forced.  The first
point is the reference every other point is compared with, bit for bit.
Interleaved rounds; a sample is the mean of --loops back-to-back runs.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sgc_amd import _lib, graphs  # noqa: E402
from sgc_amd.propagate import (SPMM_ACCUMULATE, SPMM_X_PADDED, SPMM_Y_PADDED,  # noqa: E402
                               DeviceCSR, propagate, spmm, x_flags)

prop_mod = importlib.import_module("sgc_amd.propagate")


def timed(fn, loops):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(loops):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / loops


def interleaved(names, run, rounds, loops, result):
    """Warm every point (keeping its result), then time them in turn."""
    outs, ms = {}, {k: [] for k in names}
    for k in names:
        run(k)
        torch.cuda.synchronize()
        outs[k] = result().clone() if result else None
    for _ in range(rounds):
        for k in names:
            ms[k].append(timed(lambda: run(k), loops))
    return outs, ms


def report(tag, shape, F, names, ms, outs, extra=None):
    first = names[0]
    base = float(np.median(ms[first]))
    for k in names:
        v = np.asarray(ms[k])
        rec = {"what": tag, "shape": shape, "F": F, "point": str(k),
               "bit_identical": (bool(torch.equal(outs[k], outs[first]))
                                 if outs and outs[k] is not None else None),
               "median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4),
               "max_ms": round(float(v.max()), 4), "sigma_ms": round(float(v.std()), 4),
               "median_minus_first_ms": round(float(np.median(v)) - base, 4)}
        if extra:
            rec.update(extra.get(k, {}))
        print(json.dumps(rec), flush=True)


def buffers(n, F):
    ld = (F + 31) // 32 * 32
    X = torch.zeros((n, ld), device="cuda")
    X[:, :F] = torch.randn((n, F), generator=torch.Generator().manual_seed(1)).cuda()
    return X, torch.zeros((n, ld), device="cuda")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="reddit")
    ap.add_argument("--bound", action="store_true")
    ap.add_argument("--bound-groups", default="2,3,4,6,8")
    ap.add_argument("--points", default="", help="G:Gc:H:T,... (the first is the reference)")
    ap.add_argument("--widths", default="", help="one-hop widths (default: the shape's)")
    ap.add_argument("--step", action="store_true", help="also the K-hop propagate()")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--loops", type=int, default=10)
    a = ap.parse_args()
    spec = graphs.SHAPES[a.shape]
    F0, K = spec["features"], spec["hops"]
    widths = [int(w) for w in a.widths.split(",") if w] or [F0]
    u, v = graphs.rmat_pairs(spec["n"], spec["edges"], seed=0)
    S = graphs.aug_norm_csr_from_pairs(spec["n"], u, v)
    del u, v
    n = S.n
    print(json.dumps({"what": "graph", "shape": a.shape, "n": n, "nnz": S.nnz}), flush=True)
    csr = DeviceCSR.from_host_arrays(S.row_ptr, S.col_idx, S.val, device="cuda")
    lib = _lib.load()
    stream = _lib.stream_handle(csr.device)

    if a.bound:
        F = F0
        X, Y = buffers(n, F)
        Gs = [int(g) for g in a.bound_groups.split(",")]
        launches, extra = {}, {}
        for G in Gs:
            parts = csr.column_groups(G, 0)
            plans = [c.plan(0, n, None, None, F) for c in parts]
            launches[G] = list(zip(parts, plans))
            extra[G] = {"heavy_items": [pl.n_heavy for pl in plans],
                        "hub_items": [pl.n_hub for pl in plans],
                        "heavy_threshold": [pl.threshold for pl in plans]}

        def bound_hop(G):
            for c, pl in launches[G]:
                flags = (SPMM_X_PADDED | SPMM_Y_PADDED | SPMM_ACCUMULATE | pl.hub_flags() |
                         x_flags(X[:, :F]))
                _lib.check(lib.sgc_spmm_csr_f32_ex2(
                    _lib.ptr(c.row_ptr), _lib.ptr(c.col_idx), _lib.ptr(c.val), 0, n,
                    _lib.ptr(X), X.stride(0), _lib.ptr(Y), Y.stride(0), F, _lib.ptr(pl.rows),
                    pl.n_heavy, pl.n_hub, pl.threshold, flags, pl.n_heavy, stream),
                    "spmm (bound)")
        _, ms = interleaved(Gs, bound_hop, a.rounds, a.loops, None)
        report("cost bound: one hop's heavy + hub items alone, pure split, light items cut",
               a.shape, F, Gs, ms, None, extra)
        for G in Gs:
            del launches[G]
        csr.drop_groups()
        del X, Y

    points = [tuple(int(x) for x in p.split(":")) for p in a.points.split(",") if p]
    if not points:
        return
    name = {p: "G%d/Gc%d/H%d/T%d" % p for p in points}
    for F in widths:
        X, Y = buffers(n, F)
        prop_mod.COLUMN_GROUPS = 1  # spmm() launches exactly the parts given here
        parts = {p: csr.column_groups(p[0], p[3], p[2], p[1]) for p in points}
        extra = {}
        for p in points:
            plans = [c.plan(0, n, None, None, F) for c in parts[p]]
            extra[name[p]] = {"heavy_items": [pl.n_heavy for pl in plans],
                              "light_items": [pl.n_nonempty - pl.n_heavy for pl in plans]}

        def hop(k):
            for g, c in enumerate(parts[k]):
                spmm(c, X[:, :F], 0, n, out=Y[:, :F],
                     flags=SPMM_X_PADDED | SPMM_Y_PADDED | (SPMM_ACCUMULATE if g else 0))
        outs, ms = interleaved(points, hop, a.rounds, a.loops, lambda: Y[:, :F])
        report("one hop (G/Gc/H/T)", a.shape, F, [name[p] for p in points],
               {name[p]: ms[p] for p in points}, {name[p]: outs[p] for p in points}, extra)
        del outs, X, Y, parts

    if a.step:
        F = F0
        X0 = torch.randn((n, F), generator=torch.Generator().manual_seed(1)).cuda()
        out = torch.empty((n, F), device="cuda")

        def step(p):
            (prop_mod.COLUMN_GROUPS, prop_mod.GROUP_COARSE_GROUPS, prop_mod.GROUP_COARSE_ROWS,
             prop_mod.GROUP_WHOLE_ROWS) = p
            propagate(csr, X0, K, out=out)
        outs, ms = interleaved(points, step, a.rounds, a.loops, lambda: out)
        report(f"K={K} step (G/Gc/H/T)", a.shape, F, [name[p] for p in points],
               {name[p]: ms[p] for p in points}, {name[p]: outs[p] for p in points})


if __name__ == "__main__":
    main()

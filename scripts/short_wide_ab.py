"""Wide items for short rows (sgc_set_tuning "short_wide"): what do the short
rows' per-slice waves cost, and which Ts pays?

    python scripts/short_wide_ab.py [--shape reddit] [--ts 0,4,8,12,16,24,32] [--groups 1,2]
                                    [--rounds 8] [--widths 602,304] [--no-bound] [--no-step]

1. Cost bound (no wide items involved): one accumulate launch over the un-split
   CSR at the shape's width into a scratch Y, in the engine's padded buffers,
   with the light items stopped (sgc_spmm_csr_f32_ex2's n_nonempty) at the true
   count and at the first light row of at most 8 / 16 / 32 nonzeros.  The
   difference is what those rows' per-slice waves cost: an upper bound on what
   wide items can gain per launch.
2. One hop at each width (padded buffers) for every Ts, with G = 1 and with the
   column groups; "first" = the wide workgroups at the head of the grid.
3. The K-hop propagate() of the shape (unpadded X_0, as bench.py runs it).
Interleaved rounds; every point checked bit-identical to the first.
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


def tune(key, value):
    _lib.check(_lib.load().sgc_set_tuning(key.encode(), int(value)), f"set_tuning {key}")


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def report(tag, shape, F, names, ms, outs, extra=None):
    first = names[0]
    for k in names:
        rec = {"what": tag, "shape": shape, "F": F, "point": str(k),
               "bit_identical": bool(torch.equal(outs[k], outs[first])) if outs else None,
               "median_ms": round(float(np.median(ms[k])), 4),
               "min_ms": round(float(np.min(ms[k])), 4),
               "max_ms": round(float(np.max(ms[k])), 4)}
        if extra:
            rec.update(extra.get(k, {}))
        print(json.dumps(rec), flush=True)


def interleaved(names, run, rounds, result):
    """Warm every point (keeping its result), then time them in turn."""
    outs, ms = {}, {k: [] for k in names}
    for k in names:
        run(k)
        torch.cuda.synchronize()
        outs[k] = result().clone()
    for _ in range(rounds):
        for k in names:
            ms[k].append(timed(lambda: run(k)))
    return outs, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="reddit")
    ap.add_argument("--ts", default="0,4,8,12,16,24,32")
    ap.add_argument("--groups", default="1,2")
    ap.add_argument("--widths", default="", help="one-hop widths (default: the shape's, and 304)")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--no-bound", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    Ts = [int(t) for t in a.ts.split(",")]
    Gs = [int(g) for g in a.groups.split(",")]
    spec = graphs.SHAPES[a.shape]
    F0, K = spec["features"], spec["hops"]
    widths = [int(w) for w in a.widths.split(",") if w] or [F0, 304]
    u, v = graphs.rmat_pairs(spec["n"], spec["edges"], seed=0)
    S = graphs.aug_norm_csr_from_pairs(spec["n"], u, v)
    del u, v
    n = S.n
    print(json.dumps({"what": "graph", "n": n, "nnz": S.nnz}), flush=True)
    csr = DeviceCSR.from_host_arrays(S.row_ptr, S.col_idx, S.val, device="cuda")
    lib = _lib.load()
    stream = _lib.stream_handle(csr.device)

    def buffers(F):
        ld = (F + 31) // 32 * 32
        X = torch.zeros((n, ld), device="cuda")
        X[:, :F] = torch.randn((n, F), generator=torch.Generator().manual_seed(1)).cuda()
        return X, torch.zeros((n, ld), device="cuda")

    if not a.no_bound:
        F = F0
        X, Y = buffers(F)
        pl = csr.plan(0, n, None, None, F)
        cuts = {"all rows with nonzeros": pl.n_nonempty}
        for t, above in zip((8, 16, 32), pl.above[1:]):
            cuts[f"rows above {t} only"] = max(above, pl.n_heavy)
        tune("short_wide", 0)
        flags = (SPMM_X_PADDED | SPMM_Y_PADDED | SPMM_ACCUMULATE | pl.hub_flags() |
                 x_flags(X[:, :F]))

        def launch(name):
            _lib.check(lib.sgc_spmm_csr_f32_ex2(
                _lib.ptr(csr.row_ptr), _lib.ptr(csr.col_idx), _lib.ptr(csr.val), 0, n,
                _lib.ptr(X), X.stride(0), _lib.ptr(Y), Y.stride(0), F, _lib.ptr(pl.rows),
                pl.n_heavy, pl.n_hub, pl.threshold, flags, cuts[name], stream), "spmm (bound)")
        names = list(cuts)
        _, ms = interleaved(names, launch, a.rounds, lambda: Y[:1])
        report("cost bound: accumulate launch, G = 1, light items cut", a.shape, F, names, ms,
               None, {k: {"light_items": cuts[k] - pl.n_heavy} for k in names})
        del X, Y

    for F in widths:
        X, Y = buffers(F)
        prop_mod.COLUMN_GROUPS = 1  # spmm() launches exactly the parts given here
        for G in Gs:
            parts = csr.groups_or_self(G)

            def hop(point):
                ts, first = point
                tune("short_wide", ts)
                tune("short_wide_first", first)
                for g, c in enumerate(parts):
                    spmm(c, X[:, :F], 0, n, out=Y[:, :F],
                         flags=SPMM_X_PADDED | SPMM_Y_PADDED | (SPMM_ACCUMULATE if g else 0))
            names = [(t, 0) for t in Ts] + [(16, 1)]
            outs, ms = interleaved(names, hop, a.rounds, lambda: Y[:, :F])
            report(f"one hop, G = {G} (Ts, first)", a.shape, F, names, ms, outs)
            del outs
        del X, Y

    if not a.no_step:
        F = F0
        X0 = torch.randn((n, F), generator=torch.Generator().manual_seed(1)).cuda()
        out = torch.empty((n, F), device="cuda")
        for G in Gs:
            def step(ts):
                tune("short_wide", ts)
                tune("short_wide_first", 0)
                prop_mod.COLUMN_GROUPS = G
                propagate(csr, X0, K, out=out)
            outs, ms = interleaved(Ts, step, a.rounds, lambda: out)
            report(f"K={K} step, G = {G} (Ts)", a.shape, F, Ts, ms, outs)
            del outs
    tune("short_wide", -1)
    tune("short_wide_first", 0)
    print(json.dumps({"what": "wide launches taken", "n": int(lib.sgc_get_tuning(b"short_wide_launches"))}))


if __name__ == "__main__":
    main()

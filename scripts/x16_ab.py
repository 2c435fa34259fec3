"""Interleaved A/B of the feature storage type: float32 vs bfloat16 vs float16.

    python scripts/x16_ab.py [--shapes reddit,rmat,pubmed] [--rounds 10] [--steps 5]
                             [--check device|cpu|none] [--log profiles/x16/x16_ab.log]

The K-hop propagate() call at each BASELINE shape (synthetic graphs of
sgc_amd/graphs.py), the three feature types interleaved in one process: every
round times `--steps` calls of each type with events, the order rotating per
round; round 0 is the warm-up (plans, code objects, launch list) and is
dropped.  Per type: median, min, max and inter-quartile range of the rounds in
ms per hop (the call's time / K, the X_0 re-layout included), edges/s, and the
ratio to float32 in the same run beside the spread, so "faster" can be read
against the run's own noise.

Each 16-bit result is checked once, by SHA-256 of its raw bits, against the
emulation X_{k+1} = fp32_spmm(S, X_k.float()).to(T): --check device runs
fp32_spmm as the library's fp32 kernel (bit-exact with the CPU twin, itself
tested) and converts on the device; --check cpu runs the CPU twin and torch's
CPU conversion (minutes at RMAT shape).  One JSON line per shape, appended to
--log.
"""
import argparse
import hashlib
import importlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sgc_amd import graphs  # noqa: E402

P = importlib.import_module("sgc_amd.propagate")  # the module (sgc_amd.propagate is also a function name)

TYPES = [("float32", torch.float32), ("bfloat16", torch.bfloat16), ("float16", torch.float16)]


def sha_bits(t):
    raw = t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)
    return hashlib.sha256(raw.cpu().numpy().tobytes()).hexdigest()


def emulate(csr, S, X16, K, where):
    """K hops of fp32_spmm(S, X.float()).to(T)."""
    if where == "cpu":
        c = P.DeviceCSR.from_host_arrays(S.row_ptr, S.col_idx, S.val, device="cpu")
        X = X16.cpu()
        for _ in range(K):
            X = P.spmm(c, X.float()).to(X16.dtype)
        return X
    X = X16
    for _ in range(K):
        X = P.spmm(csr, X.float().contiguous()).to(X16.dtype)
    torch.cuda.synchronize()
    return X


def stats(ms):
    q1, med, q3 = np.percentile(ms, [25, 50, 75])
    return {"median": float(med), "min": float(min(ms)), "max": float(max(ms)),
            "iqr": float(q3 - q1)}


def run_shape(shape, a):
    spec = graphs.SHAPES[shape]
    S = graphs.synthetic_graph(shape, seed=0)
    K, F = spec["hops"], spec["features"]
    X32 = torch.from_numpy(graphs.synthetic_features(shape, S.n, F, seed=1)).cuda()
    csr = P.DeviceCSR.from_host_arrays(S.row_ptr, S.col_idx, S.val, device="cuda")
    nnz = int(csr.nnz)
    X = {name: X32 if dt == torch.float32 else X32.to(dt) for name, dt in TYPES}
    checks = {}
    for name, dt in TYPES[1:]:
        if a.check == "none":
            break
        got = sha_bits(P.propagate(csr, X[name], K))
        checks[name] = got == sha_bits(emulate(csr, S, X[name], K, a.check))
    times = {name: [] for name, _ in TYPES}
    for r in range(a.rounds + 1):
        order = TYPES[r % 3:] + TYPES[:r % 3]
        for name, _ in order:
            P.propagate(csr, X[name], K)
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.steps):
                P.propagate(csr, X[name], K)
            e.record()
            torch.cuda.synchronize()
            if r:
                times[name].append(s.elapsed_time(e) / a.steps / K)
    rec = {"shape": shape, "n": S.n, "nnz": nnz, "F": F, "K": K, "rounds": a.rounds,
           "steps": a.steps, "check": a.check, "emulation_sha_equal": checks,
           "device": torch.cuda.get_device_name(0)}
    base = stats(times["float32"])
    for name, _ in TYPES:
        st = stats(times[name])
        rec[name] = {"ms_per_hop": {k: round(v, 4) for k, v in st.items()},
                     "edges_per_s": round(nnz / (st["median"] * 1e-3), 1),
                     "speedup_vs_float32": round(base["median"] / st["median"], 4),
                     "rounds_ms_per_hop": [round(t, 4) for t in times[name]]}
    # the run's own round-to-round spread, as a fraction of the fp32 median
    rec["float32_spread"] = round((base["max"] - base["min"]) / base["median"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="reddit,rmat,pubmed")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--check", default="device", choices=["device", "cpu", "none"])
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    for shape in a.shapes.split(","):
        line = json.dumps(run_shape(shape, a))
        print(line, flush=True)
        if a.log:
            os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
            with open(a.log, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

"""Interleaved A/B of the fused training loops on 16-bit features.

    python scripts/train_x16_ab.py [--rows 152410] [--features 602] [--classes 41]
                                   [--rounds 3] [--steps 2] [--epochs 100]
                                   [--log profiles/train_x16/ab.log]

Reddit-train shape (the data and teacher labels of scripts/lbfgs_train_ab.py),
`--steps` steps of LBFGS(lr=1) from the same initial weights, the variants
alternating in one process, the order swapping per round; round 0 is the
warm-up and is dropped.  Rows:

    f32          LBFGS.run_steps on X.float()       (sgc_train_lbfgs_f32)
    bf16, fp16   LBFGS.run_steps on the 16-bit X    (sgc_train_lbfgs_x16)
    literal_bf16 the literal loop of step() calls on the bf16 X -- what
                 run_steps ran on 16-bit features before sgc_train_lbfgs_x16

Per row: total ms (wall, synchronised; median, min, max of the rounds), the
closures consumed and the final loss.  Condition: the bf16
median lies below the f32 median by more than the f32 row's own spread
(max - min) over the rounds.  Then the single fused step (propagate.linear_xent:
fp32, bf16, fp16; device events over 20 calls, median of the rounds), and at
the three citation train shapes `--epochs` epochs of Adam.run_epochs on bf16
features against the literal loop on the same features (report only).  One
JSON line, appended to --log.
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sgc_amd import _lib  # noqa: E402
from sgc_amd.models import SGC  # noqa: E402
from sgc_amd.optim import Adam, LBFGS  # noqa: E402
from sgc_amd.propagate import X16_DTYPES, linear_xent, warmup  # noqa: E402

CITATION = {"cora": (140, 1433, 7), "citeseer": (120, 3703, 6), "pubmed": (60, 500, 3)}


def stats(ms):
    return {"median": round(float(np.median(ms)), 3), "min": round(min(ms), 3),
            "max": round(max(ms), 3), "rounds_ms": [round(v, 3) for v in ms]}


def lbfgs(kind, init, xs, y, steps):
    """-> (ms, func_evals, final loss on X.float())."""
    x = xs["bf16" if kind == "literal_bf16" else kind]
    model = SGC(x.shape[1], init["W.weight"].shape[0]).to(x.device)
    model.load_state_dict(init)
    model.train()
    opt = LBFGS(model.parameters(), lr=1)

    def closure():
        opt.zero_grad()
        loss = F.cross_entropy(model(x), y)
        loss.backward()
        return loss
    torch.cuda.synchronize()
    t = time.perf_counter()
    if kind == "literal_bf16":
        for _ in range(steps):
            opt.step(closure)
    else:
        opt.run_steps(model, x, y, steps)
        assert all(p.grad is None for p in model.parameters()), kind  # the fused path ran
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t) * 1e3
    with torch.no_grad():
        loss = float(F.cross_entropy(model(xs["f32"]), y))
    return ms, opt.state[opt._params[0]]["func_evals"], loss


def step_us(x, W, b, y, calls=20):
    linear_xent(x, W, b, y)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    lib = _lib.load()
    M, K = x.shape
    C = W.shape[0]
    loss = torch.empty((), device=x.device)
    dW, db = torch.empty_like(W), torch.empty_like(b)
    s = _lib.stream_handle(x.device)
    if x.dtype == torch.float32:
        n = lib.sgc_linear_xent_workspace(M, K, C)
        ws = torch.empty(n, dtype=torch.uint8, device=x.device)

        def call():
            _lib.check(lib.sgc_linear_xent_f32(_lib.ptr(x), x.stride(0), _lib.ptr(W), _lib.ptr(b),
                                               _lib.ptr(y), M, K, C, _lib.ptr(loss), _lib.ptr(dW),
                                               _lib.ptr(db), None, C, _lib.ptr(ws), n, s), "f32")
    else:
        n = lib.sgc_linear_xent_x16_workspace(M, K, C)
        ws = torch.empty(n, dtype=torch.uint8, device=x.device)
        dt = X16_DTYPES[x.dtype]

        def call():
            _lib.check(lib.sgc_linear_xent_x16(_lib.ptr(x), dt, x.stride(0), _lib.ptr(W),
                                               _lib.ptr(b), _lib.ptr(y), M, K, C, _lib.ptr(loss),
                                               _lib.ptr(dW), _lib.ptr(db), _lib.ptr(ws), n, s), "x16")
    call()
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(calls):
        call()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / calls


def adam(kind, init, x, y, epochs):
    model = SGC(x.shape[1], init["W.weight"].shape[0]).to(x.device)
    model.load_state_dict(init)
    opt = Adam(model.parameters(), lr=0.2, weight_decay=5e-4)
    torch.cuda.synchronize()
    t = time.perf_counter()
    if kind == "run_epochs":
        out = opt.run_epochs(model, x, y, epochs)
        assert model.W.weight.grad is None
    else:
        for _ in range(epochs):
            model.train()
            opt.zero_grad()
            out = F.cross_entropy(model(x), y)
            out.backward()
            opt.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, float(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=152410)
    ap.add_argument("--features", type=int, default=602)
    ap.add_argument("--classes", type=int, default=41)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    warmup(dev)
    M, K, C = a.rows, a.features, a.classes
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn(M, K, generator=g).to(dev)
    teacher = torch.randn(C, K, generator=g).to(dev) / K ** 0.5
    y = (x @ teacher.t() + 0.5 * torch.randn(M, C, generator=g).to(dev)).argmax(1)
    # every row trains on the same values: the bf16-rounded features (fp16 holds them exactly
    # only where they are in its range; reported, not compared)
    xs = {"bf16": x.bfloat16()}
    xs["f32"] = xs["bf16"].float()
    xs["fp16"] = x.half()
    torch.manual_seed(0)
    init = {k: v.clone() for k, v in SGC(K, C).to(dev).state_dict().items()}
    with open(_lib.LIB_PATH, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    rec = {"rows": M, "features": K, "classes": C, "steps": a.steps, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "library_sha256": sha}
    kinds = ["f32", "bf16", "fp16", "literal_bf16"]
    runs = {k: [] for k in kinds}
    for r in range(a.rounds + 1):
        for kind in (kinds if r % 2 == 0 else kinds[::-1]):
            out = lbfgs(kind, init, xs, y, a.steps)
            if r:
                runs[kind].append(out)
    rec["lbfgs"] = {k: dict(total_ms=stats([o[0] for o in runs[k]]), closures_consumed=runs[k][0][1],
                            final_loss=runs[k][0][2]) for k in kinds}
    f32, bf = rec["lbfgs"]["f32"]["total_ms"], rec["lbfgs"]["bf16"]["total_ms"]
    rec["f32_spread_ms"] = round(f32["max"] - f32["min"], 3)
    rec["bf16_gain_ms"] = round(f32["median"] - bf["median"], 3)
    rec["bf16_faster_than_f32_by_more_than_its_spread"] = \
        rec["bf16_gain_ms"] > rec["f32_spread_ms"]
    print("lbfgs:", json.dumps(rec["lbfgs"]), file=sys.stderr, flush=True)
    W, b = init["W.weight"], init["W.bias"]
    us = {k: [] for k in ("f32", "bf16", "fp16")}
    for r in range(a.rounds + 1):
        for k in (list(us) if r % 2 == 0 else list(us)[::-1]):
            v = step_us(xs[k], W, b, y)
            if r:
                us[k].append(v)
    rec["fused_step_us"] = {k: stats(v) for k, v in us.items()}
    print("step:", json.dumps(rec["fused_step_us"]), file=sys.stderr, flush=True)
    rec["adam"] = {}
    for name, (m, k, c) in CITATION.items():
        gen = torch.Generator().manual_seed(1)
        xa = ((torch.rand(m, k, generator=gen) < 0.01).float() * 0.1).to(dev).bfloat16()
        ya = torch.randint(0, c, (m,), generator=gen).to(dev)
        torch.manual_seed(0)
        ia = {kk: v.clone() for kk, v in SGC(k, c).to(dev).state_dict().items()}
        kinds_a = ["run_epochs", "literal"]
        ra = {kk: [] for kk in kinds_a}
        for r in range(a.rounds + 1):
            for kind in (kinds_a if r % 2 == 0 else kinds_a[::-1]):
                out = adam(kind, ia, xa, ya, a.epochs)
                if r:
                    ra[kind].append(out)
        rec["adam"][name] = {kk: dict(total_ms=stats([o[0] for o in ra[kk]]), last_loss=ra[kk][0][1])
                             for kk in kinds_a}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Interleaved A/B of the optimiser: torch.optim.LBFGS vs sgc_amd.optim.LBFGS.

    python scripts/lbfgs_ab.py [--rows 152410] [--features 602] [--classes 41]
                               [--rounds 5] [--epochs 2] [--log profiles/lbfgs/lbfgs_ab.log]

reddit.py's train_regression at Reddit-train shape (the data and teacher
labels of sgc_amd/classifier_bench.py): `--epochs` steps of LBFGS(lr=1) from
the same initial weights, the two optimisers alternating in one process, the
order swapping per round; round 0 is the warm-up and is dropped.  Both run the
reference closure unchanged (zero_grad, F.cross_entropy(model(x), y),
backward) and then the fused sgc_cross_entropy closure.

Per optimiser and closure: total ms (wall, synchronised; median, min, max of
the rounds), closures called and closures consumed (func_evals: the device
optimiser enqueues max_iter closures per step and ignores those after its
stop), the closures' own time (closures called x the median time of one
closure, timed back to back with events) and the difference: the optimiser's
share.  The baseline is torch's optimiser in the same run.  One JSON line,
appended to --log.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sgc_amd.models import SGC, sgc_cross_entropy  # noqa: E402
from sgc_amd.optim import LBFGS  # noqa: E402
from sgc_amd.propagate import warmup  # noqa: E402


def make_closure(model, opt, x, y, fused, calls):
    def closure():
        calls[0] += 1
        opt.zero_grad()
        loss = sgc_cross_entropy(model, x, y) if fused else F.cross_entropy(model(x), y)
        loss.backward()
        return loss
    return closure


def closure_ms(model, x, y, fused, reps=20, inner=10):
    """Median time of one closure, `inner` back to back per event pair."""
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    c = make_closure(model, opt, x, y, fused, [0])
    for _ in range(3):
        c()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(inner):
            c()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e) / inner)
    return float(np.median(ms))


def train(cls, init, x, y, epochs, fused):
    """-> (ms, closures called, func_evals, n_iter, final loss)."""
    model = SGC(x.shape[1], init["W.weight"].shape[0]).to(x.device)
    model.load_state_dict(init)
    opt = cls(model.parameters(), lr=1)
    calls = [0]
    closure = make_closure(model, opt, x, y, fused, calls)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(epochs):
        opt.step(closure)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t) * 1e3
    st = opt.state[opt._params[0]]
    with torch.no_grad():
        loss = float(F.cross_entropy(model(x), y))
    return ms, calls[0], st["func_evals"], st["n_iter"], loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=152410)
    ap.add_argument("--features", type=int, default=602)
    ap.add_argument("--classes", type=int, default=41)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    warmup(dev)
    M, K, C = a.rows, a.features, a.classes
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn(M, K, generator=g).to(dev)
    teacher = torch.randn(C, K, generator=g).to(dev) / K ** 0.5
    y = (x @ teacher.t() + 0.5 * torch.randn(M, C, generator=g).to(dev)).argmax(1)
    torch.manual_seed(0)
    init = {k: v.clone() for k, v in SGC(K, C).to(dev).state_dict().items()}
    rec = {"rows": M, "features": K, "classes": C, "epochs": a.epochs, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0)}
    # (device_poll4: poll_every=4, beside the two the comparison is about)
    kinds = [("torch", torch.optim.LBFGS), ("device", LBFGS),
             ("device_poll4", lambda params, lr: LBFGS(params, lr=lr, poll_every=4))]
    for fused in (False, True):
        model = SGC(K, C).to(dev)
        model.load_state_dict(init)
        per_closure = closure_ms(model, x, y, fused)
        runs = {name: [] for name, _ in kinds}
        for r in range(a.rounds + 1):
            for name, cls in (kinds if r % 2 == 0 else kinds[::-1]):
                out = train(cls, init, x, y, a.epochs, fused)
                if r:
                    runs[name].append(out)
        sub = {"closure_ms": round(per_closure, 4)}
        for name, _ in kinds:
            ms = [o[0] for o in runs[name]]
            _, called, evals, n_iter, loss = runs[name][0]
            total = float(np.median(ms))
            sub[name] = {"total_ms": {"median": round(total, 3), "min": round(min(ms), 3),
                                      "max": round(max(ms), 3)},
                         "closures_called": called, "closures_consumed": evals, "n_iter": n_iter,
                         "closures_own_ms": round(called * per_closure, 3),
                         "optimiser_share_ms": round(total - called * per_closure, 3),
                         "final_loss": loss, "rounds_ms": [round(v, 3) for v in ms]}
        sub["share_below_torch"] = sub["device"]["optimiser_share_ms"] < \
            sub["torch"]["optimiser_share_ms"]
        sub["total_not_above_torch"] = sub["device"]["total_ms"]["median"] <= \
            sub["torch"]["total_ms"]["median"]
        rec["fused_closure" if fused else "reference_closure"] = sub
    line = json.dumps(rec)
    print(line, flush=True)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Interleaved A/B of L-BFGS training: the stepwise paths vs LBFGS.run_steps.

    python scripts/lbfgs_train_ab.py [--rows 152410] [--features 602] [--classes 41]
                                     [--rounds 5] [--epochs 2]
                                     [--log profiles/lbfgs_train/ab.log]

reddit.py's train_regression at Reddit-train shape (the data and teacher
labels of scripts/lbfgs_ab.py): `--epochs` steps of LBFGS(lr=1) from the same
initial weights, all variants alternating in one process, the order swapping
per round; round 0 is the warm-up and is dropped.  Rows:

    torch            torch.optim.LBFGS, reference closure
    device           sgc_amd.optim.LBFGS, reference closure
    device_fused     the same, sgc_cross_entropy closure, poll_every None
    device_fused_p4  the same, poll_every 4
    run_steps        LBFGS.run_steps (sgc_train_lbfgs_f32)

Per row: total ms (wall, synchronised; median, min, max of the rounds), the
closures consumed (func_evals) and the final loss; with them the library's
sha256 and whether the fused median lies below the minimum of every stepwise
device row (the acceptance of DESIGN.md 4.11) and whether its final loss
equals the device_fused one bit for bit.  One JSON line, appended to --log.
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
from sgc_amd.models import SGC, sgc_cross_entropy  # noqa: E402
from sgc_amd.optim import LBFGS  # noqa: E402
from sgc_amd.propagate import warmup  # noqa: E402


def train(kind, init, x, y, epochs):
    """-> (ms, func_evals, n_iter, final loss)."""
    model = SGC(x.shape[1], init["W.weight"].shape[0]).to(x.device)
    model.load_state_dict(init)
    model.train()
    if kind == "torch":
        opt = torch.optim.LBFGS(model.parameters(), lr=1)
    else:
        opt = LBFGS(model.parameters(), lr=1, poll_every=4 if kind == "device_fused_p4" else None)
    fused = kind in ("device_fused", "device_fused_p4")

    def closure():
        opt.zero_grad()
        loss = sgc_cross_entropy(model, x, y) if fused else F.cross_entropy(model(x), y)
        loss.backward()
        return loss
    torch.cuda.synchronize()
    t = time.perf_counter()
    if kind == "run_steps":
        opt.run_steps(model, x, y, epochs)
    else:
        for _ in range(epochs):
            opt.step(closure)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t) * 1e3
    st = opt.state[opt._params[0]]
    with torch.no_grad():
        loss = float(F.cross_entropy(model(x), y))
    return ms, st["func_evals"], st["n_iter"], loss


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
    with open(_lib.LIB_PATH, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    rec = {"rows": M, "features": K, "classes": C, "epochs": a.epochs, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "library_sha256": sha}
    kinds = ["torch", "device", "device_fused", "device_fused_p4", "run_steps"]
    runs = {k: [] for k in kinds}
    for r in range(a.rounds + 1):
        for kind in (kinds if r % 2 == 0 else kinds[::-1]):
            out = train(kind, init, x, y, a.epochs)
            if r:
                runs[kind].append(out)
    for kind in kinds:
        ms = [o[0] for o in runs[kind]]
        _, evals, n_iter, loss = runs[kind][0]
        rec[kind] = {"total_ms": {"median": round(float(np.median(ms)), 3), "min": round(min(ms), 3),
                                  "max": round(max(ms), 3)},
                     "closures_consumed": evals, "n_iter": n_iter, "final_loss": loss,
                     "rounds_ms": [round(v, 3) for v in ms]}
    stepwise = ["device", "device_fused", "device_fused_p4"]
    rec["fused_median_below_every_stepwise_min"] = all(
        rec["run_steps"]["total_ms"]["median"] < rec[k]["total_ms"]["min"] for k in stepwise)
    rec["final_loss_equals_stepwise"] = \
        rec["run_steps"]["final_loss"] == rec["device_fused"]["final_loss"]
    line = json.dumps(rec)
    print(line, flush=True)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Interleaved A/B of the citation training loop: torch.optim.Adam vs
sgc_amd.optim.Adam's step() and run_epochs() on both schedules.

    python scripts/adam_ab.py [--epochs 100] [--rounds 5] [--log profiles/adam/adam_ab.log]

citation.py's train_regression (lr 0.2, weight decay 5e-6) from the same
initial weights at the three citation train shapes, the synthetic Planetoid
shape and 3000 x 602 x 41, the variants alternating in one process with the
order swapping per round; round 0 is the warm-up and is dropped.

  a  torch          the reference loop with torch.optim.Adam on the existing kernels
  b  device_step    the same loop with sgc_amd.optim.Adam.step
  c  run_general    run_epochs, adam_kernel = 1
  d  run_small      run_epochs, adam_kernel = 2 (shapes the small schedule takes)
     run_auto       run_epochs, adam_kernel = 0: what a caller gets

Each figure is the wall time of `--epochs` epochs with one synchronise at the
end (ms: median, min, max of the rounds).  One JSON line per shape, appended to
--log.
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

from sgc_amd import _lib  # noqa: E402
from sgc_amd.models import SGC  # noqa: E402
from sgc_amd.optim import Adam  # noqa: E402
from sgc_amd.propagate import warmup  # noqa: E402

SHAPES = [("cora", 140, 1433, 7), ("citeseer", 120, 3703, 6), ("pubmed", 60, 500, 3),
          ("synthetic", 100, 300, 5), ("reddit_like", 3000, 602, 41)]


def loop(model, opt, x, y, epochs):
    for _ in range(epochs):
        model.train()
        opt.zero_grad()
        loss = F.cross_entropy(model(x), y)
        loss.backward()
        opt.step()


def train(kind, init, x, y, epochs):
    """-> (ms, final loss, schedule that ran)."""
    lib = _lib.load()
    model = SGC(x.shape[1], init["W.weight"].shape[0]).to(x.device)
    model.load_state_dict(init)
    cls = torch.optim.Adam if kind == "torch" else Adam
    opt = cls(model.parameters(), lr=0.2, weight_decay=5e-6)
    lib.sgc_set_tuning(b"adam_kernel", {"run_general": 1, "run_small": 2}.get(kind, 0))
    torch.cuda.synchronize()
    t = time.perf_counter()
    if kind in ("torch", "device_step"):
        loop(model, opt, x, y, epochs)
    else:
        opt.run_epochs(model, x, y, epochs)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t) * 1e3
    ran = int(lib.sgc_get_tuning(b"adam_kernel_last")) if kind.startswith("run_") else 0
    lib.sgc_set_tuning(b"adam_kernel", 0)
    with torch.no_grad():
        loss = float(F.cross_entropy(model(x), y))
    return ms, loss, ran


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    warmup(dev)
    limit = int(_lib.load().sgc_get_tuning(b"adam_small_max_rows"))
    for name, M, K, C in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(0)
        y = torch.randint(0, C, (M,), generator=g)
        cent = torch.randn(C, K, generator=g) * 0.05
        x = ((torch.rand(M, K, generator=g) < 0.01).float() * 0.1 + cent[y].abs() * 0.2).to(dev)
        y = y.to(dev)
        torch.manual_seed(0)
        init = {k: v.clone() for k, v in SGC(K, C).to(dev).state_dict().items()}
        kinds = ["torch", "device_step", "run_general"] + (["run_small"] if M <= limit else []) + \
            ["run_auto"]
        runs = {k: [] for k in kinds}
        for r in range(a.rounds + 1):
            for kind in (kinds if r % 2 == 0 else kinds[::-1]):
                out = train(kind, init, x, y, a.epochs)
                if r:
                    runs[kind].append(out)
        rec = {"shape": name, "rows": M, "features": K, "classes": C, "epochs": a.epochs,
               "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
        for kind in kinds:
            ms = [o[0] for o in runs[kind]]
            rec[kind] = {"ms": {"median": round(float(np.median(ms)), 3), "min": round(min(ms), 3),
                                "max": round(max(ms), 3)},
                         "final_loss": runs[kind][0][1], "schedule": runs[kind][0][2]}
        rec["auto_faster_than_torch"] = rec["run_auto"]["ms"]["median"] < rec["torch"]["ms"]["median"]
        line = json.dumps(rec)
        print(line, flush=True)
        if a.log:
            os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
            with open(a.log, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()

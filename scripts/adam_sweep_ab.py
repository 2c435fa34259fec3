"""Interleaved A/B of the weight-decay sweep: B sequential Adam.run_epochs
calls against one AdamSweep.run_epochs, and B model.evaluate calls against one
ModelBank.evaluate.

    python scripts/adam_sweep_ab.py [--epochs 100] [--rounds 7] [--log profiles/adam_sweep/ab.log]

Training, at the three citation train shapes for B in {1, 8, 60} models
(lr 0.2, log-uniform decays, the same initial weights on both sides), the two
sides alternating in one process with the order swapping per round; round 0 is
the warm-up and is dropped:

  a  sequential   B calls of sgc_amd.optim.Adam.run_epochs, adam_kernel = 0
                  (what a caller had before the sweep existed)
  b  sweep        one sgc_amd.tuning.AdamSweep.run_epochs, as a caller gets it
  b1 sweep_fused  the same with adam_sweep_form = 1: launch 2 re-sums the partial
                  logits and redoes the softmax in every K-block's workgroup
  b2 sweep_split  the same with adam_sweep_form = 2: softmax once per model, then
                  dW over K-block x model (three launches per epoch)

Each figure is the wall time of `--epochs` epochs of all B models with one
synchronise at the end (ms: median, min, max of the rounds).  "spread" is the
larger of the two sides' max - min; (b) counts as faster (slower) only when the
medians differ by more than it.

Evaluation, 60 models on 500 validation rows of each dataset's width: 60 calls
of model.evaluate against one bank.evaluate, the same alternation (us).

One JSON line per measurement, appended to --log.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sgc_amd import _lib  # noqa: E402
from sgc_amd.models import SGC  # noqa: E402
from sgc_amd.optim import Adam  # noqa: E402
from sgc_amd.propagate import warmup  # noqa: E402
from sgc_amd.tuning import AdamSweep, ModelBank, sample_weight_decays  # noqa: E402

SHAPES = [("pubmed", 60, 500, 3), ("cora", 140, 1433, 7), ("citeseer", 120, 3703, 6)]
BATCHES = (1, 8, 60)
VAL_ROWS = 500


def data(M, K, C, dev):
    g = torch.Generator(device="cpu").manual_seed(0)
    y = torch.randint(0, C, (M,), generator=g)
    cent = torch.randn(C, K, generator=g) * 0.05
    x = ((torch.rand(M, K, generator=g) < 0.01).float() * 0.1 + cent[y].abs() * 0.2).to(dev)
    return x, y.to(dev)


def models_from(inits, K, C, dev):
    out = []
    for init in inits:
        m = SGC(K, C).to(dev)
        m.load_state_dict(init)
        out.append(m)
    return out


def stats(xs, digits=3):
    return {"median": round(float(np.median(xs)), digits), "min": round(min(xs), digits),
            "max": round(max(xs), digits)}


def verdict(a, b):
    """(spread, 'faster' | 'slower' | 'within spread') of b against a."""
    spread = max(max(a) - min(a), max(b) - min(b))
    d = float(np.median(a)) - float(np.median(b))
    return spread, ("faster" if d > spread else "slower" if -d > spread else "within spread")


def train_ab(name, M, K, C, B, epochs, rounds, dev):
    lib = _lib.load()
    x, y = data(M, K, C, dev)
    torch.manual_seed(0)
    inits = [{k: v.clone() for k, v in SGC(K, C).to(dev).state_dict().items()} for _ in range(B)]
    wds = [float(w) for w in sample_weight_decays(B)]
    kinds = ("sequential", "sweep", "sweep_fused", "sweep_split")
    runs = {k: [] for k in kinds}
    finals, ran = {}, {}
    for r in range(rounds + 1):
        for kind in (kinds if r % 2 == 0 else kinds[::-1]):
            models = models_from(inits, K, C, dev)
            if kind == "sequential":
                opts = [Adam(m.parameters(), lr=0.2, weight_decay=w) for m, w in zip(models, wds)]
            else:
                sweep = AdamSweep(ModelBank(models), 0.2, wds)
            lib.sgc_set_tuning(b"adam_sweep_form", {"sweep_fused": 1, "sweep_split": 2}.get(kind, 0))
            torch.cuda.synchronize()
            t = time.perf_counter()
            if kind == "sequential":
                for m, o in zip(models, opts):
                    o.run_epochs(m, x, y, epochs)
            else:
                sweep.run_epochs(x, y, epochs)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t) * 1e3
            lib.sgc_set_tuning(b"adam_sweep_form", 0)
            if r:
                runs[kind].append(ms)
            finals[kind] = torch.stack([m.W.weight.detach() for m in models])
            ran[kind] = int(lib.sgc_get_tuning(b"adam_kernel_last")) if kind == "sequential" \
                else 10 * int(lib.sgc_get_tuning(b"adam_sweep_last")) + \
                int(lib.sgc_get_tuning(b"adam_sweep_form_last"))
    spread, word = verdict(runs["sequential"], runs["sweep"])
    form_spread, form_word = verdict(runs["sweep_fused"], runs["sweep_split"])
    med_a, med_b = (float(np.median(runs[k])) for k in ("sequential", "sweep"))
    return {"what": "train", "shape": name, "rows": M, "features": K, "classes": C, "models": B,
            "epochs": epochs, "rounds": rounds, "sequential_ms": stats(runs["sequential"]),
            "sweep_ms": stats(runs["sweep"]), "spread_ms": round(spread, 3),
            "sweep_fused_ms": stats(runs["sweep_fused"]), "sweep_split_ms": stats(runs["sweep_split"]),
            "split_against_fused": form_word, "form_spread_ms": round(form_spread, 3),
            "sweep_us_per_epoch": round(med_b * 1e3 / epochs, 2),
            "sequential_us_per_epoch_per_model": round(med_a * 1e3 / epochs / B, 2),
            "sweep_over_sequential": round(med_b / med_a, 4), "sweep_is": word,
            "schedule": ran, "same_bits": all(bool(torch.equal(finals["sequential"], finals[k])) for k in kinds)}


def eval_ab(name, K, C, B, samples, dev):
    x, y = data(VAL_ROWS, K, C, dev)
    torch.manual_seed(1)
    models = [SGC(K, C).to(dev) for _ in range(B)]
    bank = ModelBank(models)
    runs = {"per_model": [], "bank": []}
    accs = {}
    for r in range(samples + 1):
        for kind in (("per_model", "bank") if r % 2 == 0 else ("bank", "per_model")):
            torch.cuda.synchronize()
            t = time.perf_counter()
            evs = [m.evaluate(x, y) for m in models] if kind == "per_model" else bank.evaluate(x, y)
            torch.cuda.synchronize()
            if r:
                runs[kind].append((time.perf_counter() - t) * 1e6)
            accs[kind] = [float(e.accuracy()) for e in evs]
    spread, word = verdict(runs["per_model"], runs["bank"])
    return {"what": "evaluate", "shape": name, "rows": VAL_ROWS, "features": K, "classes": C,
            "models": B, "samples": samples, "per_model_us": stats(runs["per_model"], 1),
            "bank_us": stats(runs["bank"], 1), "spread_us": round(spread, 1),
            "bank_over_per_model": round(float(np.median(runs["bank"])) /
                                         float(np.median(runs["per_model"])), 4),
            "bank_is": word, "same_accuracies": accs["per_model"] == accs["bank"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--eval-samples", type=int, default=30)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    warmup(dev)

    def emit(rec):
        rec["device"] = torch.cuda.get_device_name(0)
        line = json.dumps(rec)
        print(line, flush=True)
        if a.log:
            os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
            with open(a.log, "a") as f:
                f.write(line + "\n")
    for name, M, K, C in SHAPES:
        for B in BATCHES:
            emit(train_ab(name, M, K, C, B, a.epochs, a.rounds, dev))
    for name, _, K, C in SHAPES:
        emit(eval_ab(name, K, C, 60, a.eval_samples, dev))


if __name__ == "__main__":
    main()
